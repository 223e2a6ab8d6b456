"""The reduced-radix routines of the MSM kernels on RAW limb vectors (`mg_fpr_raw_op`): products, squarings, fused products and
sub2<6> with large values in every limb -- the inputs the column accumulators and their flushes (fpr_dev.h column plan) are sized
for, which canonical values plus k p (mg_field_op) never produce. Expected values are exact Python integers:
  products   (t + (t (-p^-1) mod R') p) / R'  of t = a b [+ c d], R' = 2^(K LB): the interleaved reduction computes the same m
  sub2<6>    a + 6 p - b - 2 c
compared limb for limb: K - 1 masked limbs and the unmasked top limb.

The "kernel" cases run what the accumulate kernel calls (mul_t / sqr_t / mul_add_t<true>, sub2n). For the 29-bit fields that is the
single-chain coding of the products. For BLS12-381 Fq the shipped library builds the three products as the plain routines, so
there the case repeats "plain" and only sub2n differs; the single-chain coding of that field exists behind -DMG_CHAIN_FLUSHED
only, and this file has to be run again on such a twin of the library (MANTA_LIB) whenever that coding is touched."""
import numpy as np
import pytest

from manta_rs_amd import synth

pytestmark = pytest.mark.gpu

MODULUS = {"bn254_fr": synth.FR_MODULUS[0], "bn254_fq": synth.FQ_MODULUS[0], "bls381_fr": synth.FR_MODULUS[1],
           "bls381_fq": synth.FQ_MODULUS[1]}
LIMBS = {"bn254_fr": (9, 29), "bn254_fq": (9, 29), "bls381_fr": (9, 29), "bls381_fq": (13, 30)}  # (K, LB)


def value(limbs, LB):
    return sum(int(x) << (i * LB) for i, x in enumerate(limbs))


def split(v, K, LB):
    assert 0 <= v < 1 << ((K - 1) * LB + 32), "the top limb is one 32-bit word"
    return [(v >> (i * LB)) & ((1 << LB) - 1) for i in range(K - 1)] + [v >> ((K - 1) * LB)]


def unit(K, i, x):
    v = [0] * K
    v[i] = x
    return v


def limb_sets(K, LB, seed):
    """(structured vectors, per-pair vectors (e_i, e_j), random vectors) with limbs up to 2^LB - 1"""
    L = (1 << LB) - 1
    rng = np.random.default_rng(seed)
    structured = [[L] * K, [0] * K, [L if i % 2 == 0 else 0 for i in range(K)], [L if i % 2 else 0 for i in range(K)]]
    pairs = [(unit(K, i, L), unit(K, j, L)) for i in range(K) for j in range(K)]
    rand = [[int(x) for x in rng.integers(0, L + 1, K)] for _ in range(300)]
    return structured, pairs, rand


def operand_rows(field):
    """rows (a, b, c, d) of limb vectors for the products"""
    K, LB = LIMBS[field]
    st, pairs, rand = limb_sets(K, LB, 7 + K)
    rows = [(x, y, z, w) for x in st for y in st for z, w in ((st[0], st[0]), (st[1], st[2]), (y, x))]
    rows += [(ei, ej, ei, ej) for ei, ej in pairs] + [(ei, ej, st[1], st[1]) for ei, ej in pairs[::7]]
    rows += [(ei, ej, st[0], st[0]) for ei, ej in pairs[::5]]
    rows += [(rand[4 * i], rand[4 * i + 1], rand[4 * i + 2], rand[4 * i + 3]) for i in range(len(rand) // 4)]
    rows += [(r, st[0], st[0], r) for r in rand[:40]]
    # squarings: two limbs at a time isolate each doubled cross product
    L = (1 << LB) - 1
    for i in range(K):
        for j in range(i + 1, K):
            v = unit(K, i, L)
            v[j] = L
            rows.append((v, v, v, v))
    return rows


def sub2_rows(field):
    """rows (a, b, c) for a + 6p - b - 2c: a any limbs; b and c with every lower limb free and the top limbs kept small enough
    that b + 2c < 6p (the lower K - 1 limbs of b + 2c stay below 3 units of the top limb)"""
    K, LB = LIMBS[field]
    L = (1 << LB) - 1
    top6 = (6 * MODULUS[field]) >> ((K - 1) * LB)
    cap = (top6 - 3) // 3
    assert 0 < cap <= L
    st, pairs, rand = limb_sets(K, LB, 11 + K)
    clamp = lambda v: v[:K - 1] + [min(v[K - 1], cap)]
    rows = [([0] * K, clamp(st[0]), clamp(st[0])), (st[0], [0] * K, [0] * K)]  # the two corners: most negative / most positive limbs
    rows += [(x, clamp(y), clamp(z)) for x in st for y in st for z in st]
    rows += [(ei, clamp(ej), clamp(ei)) for ei, ej in pairs] + [(st[1], clamp(ei), clamp(ej)) for ei, ej in pairs]
    rows += [(rand[3 * i], clamp(rand[3 * i + 1]), clamp(rand[3 * i + 2])) for i in range(len(rand) // 3)]
    for a, b, c in rows:
        assert value(b, LB) + 2 * value(c, LB) < 6 * MODULUS[field]
    return rows


def arr(rows, col):
    return np.array([r[col] for r in rows], dtype=np.uint32)


@pytest.fixture(scope="module")
def expected():
    """per field: the operand rows and the exact results of the three products, computed once for both codings"""
    out = {}
    for field, (K, LB) in LIMBS.items():
        p, Rp = MODULUS[field], 1 << (K * LB)
        ninv = (-pow(p, -1, Rp)) % Rp
        rows = operand_rows(field)

        def redc(t):
            m = (t * ninv) % Rp
            assert (t + m * p) % Rp == 0
            return split((t + m * p) // Rp, K, LB)

        vals = [tuple(value(x, LB) for x in r) for r in rows]
        out[field] = dict(rows=rows,
                          mul=np.array([redc(a * b) for a, b, _, _ in vals], dtype=np.uint32),
                          sqr=np.array([redc(a * a) for a, _, _, _ in vals], dtype=np.uint32),
                          mul_add=np.array([redc(a * b + c * d) for a, b, c, d in vals], dtype=np.uint32))
    return out


@pytest.mark.parametrize("chain", [False, True], ids=["plain", "kernel"])
@pytest.mark.parametrize("field", sorted(LIMBS))
def test_raw_products_match_exact_integers(gpu, expected, field, chain):
    e = expected[field]
    rows = e["rows"]
    assert len(rows) <= 4000
    a, b, c, d = (arr(rows, i) for i in range(4))
    for op, args in (("mul", (a, b)), ("sqr", (a,)), ("mul_add", (a, b, c, d))):
        got = gpu.fpr_raw_op(field, op, *args, chain=chain)
        bad = np.nonzero((got != e[op]).any(axis=1))[0]
        assert bad.size == 0, (op, "first wrong row", int(bad[0]), rows[int(bad[0])], got[bad[0]].tolist(), e[op][bad[0]].tolist())


@pytest.mark.parametrize("field", sorted(LIMBS))
def test_raw_sub2_matches_exact_integers(gpu, field):
    K, LB = LIMBS[field]
    rows = sub2_rows(field)
    assert len(rows) <= 4000
    want = np.array([split(value(a, LB) + 6 * MODULUS[field] - value(b, LB) - 2 * value(c, LB), K, LB) for a, b, c in rows],
                    dtype=np.uint32)
    for chain in (False, True):  # the generic sub2, then the accumulate kernel's 32-bit form
        got = gpu.fpr_raw_op(field, "sub2_6", arr(rows, 0), arr(rows, 1), arr(rows, 2), chain=chain)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, ("first wrong row", int(bad[0]), rows[int(bad[0])], got[bad[0]].tolist(), want[bad[0]].tolist())


def sub2_12_rows(field):
    """rows (a, b, c) shaped like the operands of the generic additions over Fp2 (ec_dev.h add_body: X3 = R^2 + 12p - PPP - 2Q with
    components below 4p): values below 4p and 2p in normalised limbs, their extremes, and b + 2c right under 12p"""
    K, LB = LIMBS[field]
    p = MODULUS[field]
    rng = np.random.default_rng(23 + K)
    big = lambda bound: int.from_bytes(rng.bytes(64), "little") % bound
    edge = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 4 * p - 1, (1 << (LB * (K - 1))) - 1, 1 << (LB * (K - 1)), 4 * p - (1 << (LB - 1))]
    vals = [(a, b, c) for a in edge for b in edge for c in edge]
    vals += [(big(4 * p), big(4 * p), big(4 * p)) for _ in range(300)] + [(big(2 * p), big(2 * p), big(2 * p)) for _ in range(100)]
    vals += [(a, 4 * p - 1, 4 * p - 1) for a in edge] + [(big(4 * p), b, (12 * p - 1 - b) // 2) for b in edge]
    return [tuple(split(v, K, LB) for v in row) for row in vals]


@pytest.mark.parametrize("field", sorted(LIMBS))
def test_raw_sub2_12_on_the_operand_shapes_of_the_fp2_additions(gpu, field):
    """sub2n<12> alone, on normalised operands as the generic group operations would hand them over. (Inside those operations
    over BLS12-381 Fp2 the 32-bit form gave wrong sums for a reason not established, which is why they keep sub2; this pins down
    that the routine itself is exact on such inputs.)"""
    K, LB = LIMBS[field]
    rows = sub2_12_rows(field)
    assert len(rows) <= 4000
    want = np.array([split(value(a, LB) + 12 * MODULUS[field] - value(b, LB) - 2 * value(c, LB), K, LB) for a, b, c in rows],
                    dtype=np.uint32)
    for chain in (False, True):
        got = gpu.fpr_raw_op(field, "sub2_12", arr(rows, 0), arr(rows, 1), arr(rows, 2), chain=chain)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (chain, "first wrong row", int(bad[0]), rows[int(bad[0])], got[bad[0]].tolist(), want[bad[0]].tolist())


def test_raw_op_rejects_bad_arguments(gpu):
    a = np.zeros((4, 13), dtype=np.uint32)
    with pytest.raises(gpu.MantaGpuError):
        gpu._chk(gpu.LIB.mg_fpr_raw_op(3, 0, 0, gpu._p(a), None, None, None, gpu._sz(4), gpu._p(a)), "mul without b")
    with pytest.raises(gpu.MantaGpuError):
        gpu._chk(gpu.LIB.mg_fpr_raw_op(3, 5, 0, gpu._p(a), gpu._p(a), None, None, gpu._sz(4), gpu._p(a)), "unknown op")
    with pytest.raises(gpu.MantaGpuError):
        gpu._chk(gpu.LIB.mg_fpr_raw_op(9, 0, 0, gpu._p(a), gpu._p(a), None, None, gpu._sz(4), gpu._p(a)), "unknown field")
