"""The reduced-radix routines of the MSM kernels on RAW limb vectors (`mg_fpr_raw_op`): products, squarings, fused products and
sub2<6> with large values in every limb -- the inputs the column accumulators and their flushes (fpr_dev.h column plan) are sized
for, which canonical values plus k p (mg_field_op) never produce. Expected values are exact Python integers:
  products   (t + (t (-p^-1) mod R') p) / R'  of t = a b [+ c d], R' = 2^(K LB): the interleaved reduction computes the same m
  sub2<6>    a + 6 p - b - 2 c
compared limb for limb: K - 1 masked limbs and the unmasked top limb.

The "plain" cases run FpR::mul / sqr / mul_add: for BLS12-381 Fq one column walker (FpR::product) for the three products, for the
29-bit fields the interleaved bodies. The "kernel" cases run what the accumulate kernel calls (mul_t / sqr_t / mul_add_t<true>, sub2n): the single-chain coding of the
products, which is asm links for the 29-bit fields and the same walker with its multiply-adds pinned in C for BLS12-381 Fq
(MG_CHAIN_FLUSHED, default 1). A twin of the library built with -DMG_CHAIN_FLUSHED=0 (MANTA_LIB) makes that field's "kernel"
products the plain routines again; there only sub2n differs between the two cases.

The lazy-limb test feeds the products of the 29-bit fields what a carry-free subtraction (subl) leaves: limbs up to 3 * 2^LB."""
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


def reducer(field):
    """t -> the limbs of (t + (t (-p^-1) mod R') p) / R'"""
    K, LB = LIMBS[field]
    p, Rp = MODULUS[field], 1 << (K * LB)
    ninv = (-pow(p, -1, Rp)) % Rp

    def redc(t):
        m = (t * ninv) % Rp
        assert (t + m * p) % Rp == 0
        return split((t + m * p) // Rp, K, LB)

    return redc


@pytest.fixture(scope="module")
def expected():
    """per field: the operand rows and the exact results of the three products, computed once for both codings"""
    out = {}
    for field, (K, LB) in LIMBS.items():
        redc = reducer(field)
        rows = operand_rows(field)
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


LAZY_FIELDS = sorted(f for f, (K, LB) in LIMBS.items() if LB == 29)  # the fields whose plans hold no flush: the NTT butterfly feeds them subl<3> limbs


def lazy_limbs(field, a, b):
    """the limbs FpR::subl<3> leaves for normalised a, b < 2p: a_i + q_i - b_i with 3p in the redundant form q (each limb lends one
    unit of 2^LB to the limb below), no carry pass: limbs below 3 * 2^LB, value a + 3p - b < 5p"""
    K, LB = LIMBS[field]
    p = MODULUS[field]
    assert 0 <= a < 2 * p and 0 <= b < 2 * p
    m = split(3 * p, K, LB)
    q = [m[0] + (1 << LB)] + [m[i] + (1 << LB) - 1 for i in range(1, K - 1)] + [m[K - 1] - 1]
    r = [x + y - z for x, y, z in zip(split(a, K, LB), q, split(b, K, LB))]
    assert all(0 <= x < 3 << LB for x in r) and value(r, LB) == a + 3 * p - b
    return r


def lazy_rows(field):
    """rows (a, b, y, c, d, w) of integers below 2p: the products are lazy(a, b) * y and lazy(a, b) * y + lazy(c, d) * w"""
    K, LB = LIMBS[field]
    p = MODULUS[field]
    L = (1 << LB) - 1
    edge = [0, 1, p - 1, p, 2 * p - 1]
    top = min(L, (2 * p - 1) >> ((K - 1) * LB))
    full = ((top - 1) << ((K - 1) * LB)) | ((1 << ((K - 1) * LB)) - 1)  # every lower limb at its maximum, value below 2p
    single = [(L if i < K - 1 else top) << (i * LB) for i in range(K)]  # one limb at its maximum
    assert full < 2 * p and all(v < 2 * p for v in single)
    rows = [(a, b, y, b, a, edge[(k + 2) % 5]) for a in edge for b in edge for k, y in enumerate(edge)]
    rows += [(full, 0, full, full, 0, full), (0, full, full, full, 0, full), (full, 0, full, 0, full, 1), (2 * p - 1, 0, 2 * p - 1, 2 * p - 1, 0, 2 * p - 1)]
    rows += [(si, 0, sj, sj, 0, si) for si in single for sj in single]       # the largest lazy limb i against the largest limb j
    rows += [(0, si, full, full, si, single[K - 1 - i]) for i, si in enumerate(single)]  # ... and the smallest
    rng = np.random.default_rng(31 + K)
    rows += [tuple(int.from_bytes(rng.bytes(48), "little") % (2 * p) for _ in range(6)) for _ in range(200)]
    return rows


@pytest.mark.parametrize("chain", [False, True], ids=["plain", "kernel"])
@pytest.mark.parametrize("field", LAZY_FIELDS)
def test_raw_products_of_lazy_limb_operands_match_exact_integers(gpu, field, chain):
    """The plain and the fused product with the limbs of a carry-free subtraction (subl<3>, limbs up to 3 * 2^LB) as one operand
    of each pair and a normalised value below 2p as the other: operand bounds 5 * 2 + 5 * 2 <= RR_LIM, so the result is below 2p
    and its limbs are those of the exact reduction."""
    K, LB = LIMBS[field]
    redc = reducer(field)
    rows = lazy_rows(field)
    assert len(rows) < 1000
    x = np.array([lazy_limbs(field, a, b) for a, b, _, _, _, _ in rows], dtype=np.uint32)
    z = np.array([lazy_limbs(field, c, d) for _, _, _, c, d, _ in rows], dtype=np.uint32)
    y = np.array([split(r[2], K, LB) for r in rows], dtype=np.uint32)
    w = np.array([split(r[5], K, LB) for r in rows], dtype=np.uint32)
    assert int(x.max()) > 5 << (LB - 1), "no limb above 2.5 * 2^LB: the rows miss the case"
    p = MODULUS[field]
    lv = lambda a, b: a + 3 * p - b
    want = {"mul": np.array([redc(lv(a, b) * yy) for a, b, yy, _, _, _ in rows], dtype=np.uint32),
            "mul_add": np.array([redc(lv(a, b) * yy + lv(c, d) * ww) for a, b, yy, c, d, ww in rows], dtype=np.uint32)}
    for op, args in (("mul", (x, y)), ("mul_add", (x, y, z, w))):
        got = gpu.fpr_raw_op(field, op, *args, chain=chain)
        bad = np.nonzero((got != want[op]).any(axis=1))[0]
        assert bad.size == 0, (op, "first wrong row", int(bad[0]), rows[int(bad[0])], got[bad[0]].tolist(), want[op][bad[0]].tolist())


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
