"""Every building block of the GPU pairing (manta_rs_amd/csrc/pairing_coop.h, reached one at a time through `mg_pairing_op`)
against the plain-integer model of tests/pairing_tower_ref.py: exact equality of Montgomery limbs, no tolerance anywhere.

Whole pairings only ever hand these functions random-looking elements. Here they get what a Miller value never is: zeros, ones,
p - 1, limb-boundary words, one-hot and half-empty elements, lines with zero coefficients -- the inputs at which `reduce_top`
meets an exact multiple of p, `inv_euclid` takes its other tail and a wrong table entry of one lane shows in one coefficient.
Edge values are chosen as Montgomery representatives y (the words the arithmetic sees); the model works on y R^-1.

Model cost (measured, one CPU core, BN254 / BLS12-381): an inverse or a final exponentiation 0.1 / 0.15 s, a p-power 8 / 15 ms.
The p-powers behind the Frobenius maps (each level one p-power of the level below) and the cyclotomic inputs are computed once
per curve and shared by the tests that need them; the most expensive expected values, those of conj12, take 1.3 / 2.8 s."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import pairing_tower_ref as T
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu

CURVES = [0, 1]
BATCH = 64  # Fq12 elements per launch at most: one single-wavefront workgroup each


# ------------------------------------------------------------------------------------------------ inputs
def _rand_f2(t, rng):
    return (rng.field(t.p), rng.field(t.p))


def _rand_el(t, rng):
    return tuple(_rand_f2(t, rng) for _ in range(6))


@functools.lru_cache(maxsize=None)
def tower_inputs(curve):
    """(labels, elements) for MUL12, SQR12, ELL, FROB12_k and CONJ12"""
    t = T.tower(curve)
    rng = synth.XorShift(0x7031 + curve)
    out = []
    for y in t.edge_representatives():               # every component the same edge word
        v = t.mont_value(y)
        out.append(("all %#x" % y, ((v, v),) * 6))
    for slot in range(12):                            # one-hot: a single component, the values one and minus one
        for name, v in (("+1", 1), ("-1", t.p - 1)):
            vals = [0] * 12
            vals[slot] = v
            out.append(("one-hot slot %d %s" % (slot, name), t.from_slots(vals)))
    dense = [_rand_el(t, rng) for _ in range(6)]
    out.append(("even powers of w only", tuple(c if m % 2 == 0 else (0, 0) for m, c in enumerate(dense[0]))))
    out.append(("odd powers of w only", tuple(c if m % 2 == 1 else (0, 0) for m, c in enumerate(dense[1]))))
    out += [("dense random %d" % i, d) for i, d in enumerate(dense[2:])]
    assert len(out) <= BATCH
    return [n for n, _ in out], [e for _, e in out]


@functools.lru_cache(maxsize=None)
def frobenius_chain(curve, upto):
    """[a^(p^j) for a in tower_inputs] for j = 0 .. upto, each level one p-power of the level below (computed once)"""
    t = T.tower(curve)
    if upto == 0:
        return (tuple(tower_inputs(curve)[1]),)
    below = frobenius_chain(curve, upto - 1)
    return below + (tuple(t.pow(a, t.p) for a in below[-1]),)


@functools.lru_cache(maxsize=None)
def cyclotomic_inputs(curve):
    """model-made elements of the cyclotomic subgroup: the identity, from random a, from a one-hot a (which the easy part sends
    to the identity again: c w^k has c^(p^6 - 1) = 1 and w^(p^6 - 1) = -1) and from a two-term a"""
    t = T.tower(curve)
    rng = synth.XorShift(0xc1c + curve)
    one_hot = t.from_slots([0] * 7 + [t.p - 1] + [0] * 4)
    two_terms = t.from_slots([1, 0, 0, 0, 0, 0, t.p - 1, 0, 0, 0, 0, 0])  # 1 - w
    src = [("identity", t.one), ("from random 0", _rand_el(t, rng)), ("from random 1", _rand_el(t, rng)), ("from one-hot", one_hot),
           ("from 1 - w", two_terms)]
    els = [t.cyclotomic(a) for _, a in src]
    assert els[0] == t.one and els[3] == t.one and els[4] != t.one
    return [n for n, _ in src], els


def gpu_pairing_value(gpu, curve):
    """e(a G1, b G2) as the GPU computes it for a verifying key (a Miller loop and the final exponentiation): in the subgroup"""
    r = synth.FR_MODULUS[curve]
    lim = lambda k: synth.ints_to_limbs([k % r], 4)[0]
    G1, G2 = O.generator(curve, 1), O.generator(curve, 2)

    class Key:
        pass

    k = Key()
    k.alpha_g1, k.beta_g2 = O.g_mul(curve, 1, G1, lim(0x51f3a7)), O.g_mul(curve, 2, G2, lim(0x77e1d5))
    k.gamma_g2, k.delta_g2, k.gamma_abc_g1 = G2, G2, np.stack([G1])
    return T.tower(curve).from_bytes(gpu.VerifyingContext(curve, k).alpha_g1_beta_g2())


def run12(gpu, curve, op, a_elements, b_words=None):
    """an Fq12 operation over model elements, BATCH per launch -> [len, 12 N] words"""
    t = T.tower(curve)
    a = t.words(a_elements)
    outs = []
    for lo in range(0, len(a), BATCH):
        outs.append(gpu.pairing_op(curve, op, a[lo:lo + BATCH], None if b_words is None else b_words[lo:lo + BATCH]))
    return np.concatenate(outs)


def same(t, got, want_elements, labels, what):
    want = t.words(list(want_elements))
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, "%d wrong of %d, first:" % (bad.size, len(want)), labels[int(bad[0])], got[bad[0]].tolist(), want[bad[0]].tolist())


# ------------------------------------------------------------------------------------------------ Fq12: products
@pytest.mark.parametrize("curve", CURVES)
def test_mul12(gpu, curve):
    t = T.tower(curve)
    labels, els = tower_inputs(curve)
    n = len(els)
    rng = synth.XorShift(0x3121 + curve)
    dense = _rand_el(t, rng)
    pairs = [(labels[i] + " x " + labels[(i + 7) % n], els[i], els[(i + 7) % n]) for i in range(n)]  # edge x one-hot, one-hot x sparse, ...
    pairs += [(labels[i] + " x dense", els[i], dense) for i in range(n)] + [("dense x " + labels[i], dense, els[i]) for i in range(n)]
    a = _rand_el(t, rng)
    pairs += [("a x conj(a)", a, t.conj(a)), ("conj(a) x a", t.conj(a), a), ("a x 1/a", a, t.inv(a)), ("0 x 0", t.zero, t.zero)]
    got = run12(gpu, curve, "mul12", [x for _, x, _ in pairs], t.words([y for _, _, y in pairs]))
    same(t, got, [t.mul(x, y) for _, x, y in pairs], [l for l, _, _ in pairs], "mul12")
    assert t.elements(got[-2:-1]) == [t.one]   # a x 1/a


@pytest.mark.parametrize("curve", CURVES)
def test_sqr12_and_it_equals_mul12_of_the_same_operand(gpu, curve):
    t = T.tower(curve)
    labels, els = tower_inputs(curve)
    got = run12(gpu, curve, "sqr12", els)
    same(t, got, [t.mul(a, a) for a in els], labels, "sqr12")
    assert (got == run12(gpu, curve, "mul12", els, t.words(els))).all()   # limb for limb
    assert (gpu.pairing_op(curve, "sqr12", t.words(els[:1])) == got[:1]).all()   # n = 1


def lines(t):
    """(label, three Fq2 coefficients): random, one coefficient zero, all zero, coefficients from the edge list"""
    rng = synth.XorShift(0xe11 + t.curve)
    out = [("random %d" % i, [_rand_f2(t, rng) for _ in range(3)]) for i in range(3)]
    for z in range(3):
        out.append(("coefficient %d zero" % z, [(0, 0) if k == z else _rand_f2(t, rng) for k in range(3)]))
    out.append(("all three zero", [(0, 0)] * 3))
    edges = t.edge_representatives()
    for i, y in enumerate(edges):
        v, w = t.mont_value(y), t.mont_value(edges[(i + 5) % len(edges)])
        out.append(("edge %#x" % y, [(v, v), (w, v), (v, w)]))
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_ell(gpu, curve):
    """f times the line sum_t L_t w^LINE_J(t): the eighteen Fq2 products as one Fq product per lane and one lincomb behind it"""
    t = T.tower(curve)
    labels, els = tower_inputs(curve)
    ls = lines(t)
    rng = synth.XorShift(0xe12 + curve)
    dense = [_rand_el(t, rng) for _ in range(2)]
    cases = [(labels[i] + " | line " + ls[i % len(ls)][0], els[i], ls[i % len(ls)][1]) for i in range(len(els))]
    cases += [("dense %d | line %s" % (i % 2, l), dense[i % 2], c) for i, (l, c) in enumerate(ls)]
    cases += [(labels[i] + " | line random 0", els[i], ls[0][1]) for i in range(len(els))]
    lw = np.concatenate([t.f2_words(c).reshape(1, -1) for _, _, c in cases])
    got = run12(gpu, curve, "ell", [f for _, f, _ in cases], lw)
    same(t, got, [t.mul(f, t.line(c)) for _, f, c in cases], [l for l, _, _ in cases], "ell")


# ------------------------------------------------------------------------------------------------ Fq12: Frobenius maps
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("curve", CURVES)
def test_frob12(gpu, curve, k):
    t = T.tower(curve)
    labels, els = tower_inputs(curve)
    same(t, run12(gpu, curve, "frob12_%d" % k, els), frobenius_chain(curve, k)[k], labels, "frob12<%d>: a^(p^%d)" % (k, k))


@pytest.mark.parametrize("curve", CURVES)
def test_conj12(gpu, curve):
    t = T.tower(curve)
    labels, els = tower_inputs(curve)
    same(t, run12(gpu, curve, "conj12", els), frobenius_chain(curve, 6)[6], labels, "conj12: a^(p^6)")


# ------------------------------------------------------------------------------------------------ the cyclotomic subgroup
@pytest.mark.parametrize("curve", CURVES)
def test_cyc_sqr12(gpu, curve):
    t = T.tower(curve)
    labels, els = cyclotomic_inputs(curve)
    labels, els = labels + ["a GPU pairing value"], els + [gpu_pairing_value(gpu, curve)]
    got = run12(gpu, curve, "cyc_sqr12", els)
    same(t, got, [t.mul(a, a) for a in els], labels, "cyc_sqr12")
    assert (got == run12(gpu, curve, "sqr12", els)).all()


@pytest.mark.parametrize("curve", CURVES)
def test_exp_by_x(gpu, curve):
    """a^x with the sign of x as the curve has it (BN254: the width-4 NAF path with conjugations for the negative digits)"""
    t = T.tower(curve)
    labels, els = cyclotomic_inputs(curve)
    labels, els = labels + ["a GPU pairing value"], els + [gpu_pairing_value(gpu, curve)]
    same(t, run12(gpu, curve, "exp_by_x", els), [t.pow_x(a) for a in els], labels, "exp_by_x")


# ------------------------------------------------------------------------------------------------ inverse, final exponentiation
def unit_inputs(curve):
    """at most eight non-zero elements: one, minus one, one-hot, an element of Fq2, a cyclotomic one, random ones"""
    t = T.tower(curve)
    rng = synth.XorShift(0x1f + curve)
    out = [("one", t.one), ("minus one", ((t.p - 1, 0),) + ((0, 0),) * 5), ("one-hot u w^3", t.line([(0, 0), (0, 0), (0, 1)])),
           ("an element of Fq2", (_rand_f2(t, rng),) + ((0, 0),) * 5), ("cyclotomic", cyclotomic_inputs(curve)[1][1])]
    out += [("random %d" % i, _rand_el(t, rng)) for i in range(3)]
    return [n for n, _ in out], [e for _, e in out]


@pytest.mark.parametrize("curve", CURVES)
def test_inv12(gpu, curve):
    t = T.tower(curve)
    labels, els = unit_inputs(curve)
    assert len(els) <= 8 and t.zero not in els
    same(t, run12(gpu, curve, "inv12", els), [t.inv(a) for a in els], labels, "inv12: a^(p^12 - 2)")


@pytest.mark.parametrize("curve", CURVES)
def test_final_exp(gpu, curve):
    t = T.tower(curve)
    labels, els = unit_inputs(curve)
    assert len(els) <= 8 and t.zero not in els
    same(t, run12(gpu, curve, "final_exp", els), [t.final_exp(a) for a in els], labels, "final_exp: a^(c (p^12 - 1) / r)")


# ------------------------------------------------------------------------------------------------ Fq: the one-lane inversion
@pytest.mark.parametrize("curve", CURVES)
def test_fq_inv_euclid_takes_both_tails(gpu, curve):
    t = T.tower(curve)
    rng = synth.XorShift(0x1e + curve)
    ys = list(range(1, 17)) + [y for y in t.edge_representatives() if y > 16] + [1 << (t.bits - 1)]
    ys += [rng.field(t.p - 1) + 1 for _ in range(64)]
    assert 0 not in ys
    # census: the inputs reach the first step count, both sides of the boundary between the tails, and the most steps found
    ks = [t.almost_inverse_steps(y) for y in ys]
    top = 507 if curve == 0 else 761
    for k in (t.bits, 32 * t.N - 1, 32 * t.N, 32 * t.N + 1, top):
        assert k in ks, k
    assert max(ks) == top and min(ks) == t.bits
    got = np.concatenate([gpu.pairing_op(curve, "fq_inv_euclid", t.raw_words(ys[lo:lo + BATCH])) for lo in range(0, len(ys), BATCH)])
    want = t.fq_words([pow(t.mont_value(y), t.p - 2, t.p) for y in ys])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, ("first wrong: y, k", hex(ys[int(bad[0])]), ks[int(bad[0])], got[bad[0]].tolist(), want[bad[0]].tolist())


# ------------------------------------------------------------------------------------------------ Fq: lincomb and reduce_top
def sq_entry_rows(k):
    """the coefficient rows of pairing_coop.h's sq_entry (lane l: component l & 1 of coefficient l >> 1 of a square), xi = k + u"""
    rows = []
    for l in range(12):
        m, comp, row = l >> 1, l & 1, []
        for i in range(6):
            for j in range(i, 6):
                if (i + j) % 6 != m:
                    continue
                wrap = i + j >= 6
                if i == j:
                    if not wrap:
                        row += [2 if comp else 1]
                    else:
                        row += [2 * k, 1] if comp else [k, -2]
                elif not wrap:
                    row += [2, -2, -2] if comp else [2, -2]
                elif not comp:
                    row += [2 * k + 2, -2] + ([-(2 * k - 2)] if k > 1 else [])
                else:
                    row += [2 * k, -(2 * k + 2)] + ([-(2 * k - 2)] if k > 1 else [])
        assert len(row) <= 10
        rows.append((m, comp, row + [0] * (10 - len(row))))
    return rows


def lincomb_rows(t):
    """(label, ten Montgomery representatives, ten coefficients)"""
    p = t.p
    rng = synth.XorShift(0x11c + t.curve)
    edges = t.edge_representatives()
    rnd = lambda: [rng.field(p) for _ in range(10)]
    pad = lambda xs, fill=0: list(xs) + [fill] * (10 - len(xs))
    rows = [("all zero, edge operands", pad(edges[:10]), [0] * 10), ("all zero, random operands", rnd(), [0] * 10)]
    for pos in (0, 3, 9):
        for c in (255, -255):
            cf = [0] * 10
            cf[pos] = c
            rows.append(("single %d on p - 1 at %d" % (c, pos), [p - 1] * 10, cf))
            rows.append(("single %d on random at %d" % (c, pos), rnd(), cf))
    rows.append(("five +51 and five -51 on p - 1", [p - 1] * 10, [51, -51] * 5))
    rows.append(("five +51 then five -51 on p - 1", [p - 1] * 10, [51] * 5 + [-51] * 5))
    rows.append(("ten +25 on p - 1", [p - 1] * 10, [25] * 10))
    rows.append(("ten -25 on p - 1", [p - 1] * 10, [-25] * 10))
    for v in edges + rnd()[:4]:   # the same value with +c and -c: the result is 0 and t = 256 p exactly
        for c in (255, 1):
            rows.append(("+%d and -%d on %#x" % (c, c, v), pad([v, v], rng.field(p)), pad([c, -c])))
    for c in (1, 9, 20, 127):     # c (p - 1) + c 1 = c p: t = (256 + c) p exactly (c = 255 twice would pass the sum bound)
        rows.append(("%d (p - 1) + %d 1" % (c, c), pad([p - 1, 1], 5), pad([c, c])))
        rows.append(("-%d (p - 1) - %d 1" % (c, c), pad([p - 1, 1], 5), pad([-c, -c])))
        if 3 * c < 256:
            rows.append(("%d (p - 1) + %d 1 - %d 2 + %d 2" % (c, c, c, c), pad([p - 1, 1, 2, 2], 5), pad([c, c, -c, c])))
    rows.append(("255 (p - 1) - 255 1", pad([p - 1, 1]), pad([255, -255])))
    rows.append(("128 1 + 127 (p - 1) - 255 (p - 1)", pad([1, p - 1, p - 1]), pad([128, 127, -255])))
    for m, comp, cf in sq_entry_rows(t.u0):   # the squaring's own rows (the wrapped components carry xi), every product p - 1
        rows.append(("sq_entry coefficient %d component %d on p - 1" % (m, comp), [p - 1] * 10, cf))
        rows.append(("sq_entry coefficient %d component %d on random" % (m, comp), rnd(), cf))
    for y in edges:                            # every edge word under the largest and under mixed coefficients
        rows.append(("255 on %#x" % y, pad([y], p - 1), pad([255])))
        rows.append(("mixed on %#x" % y, pad([y, y, p - 1, y], 1), pad([100, 55, -200, 100, -55])))
    for i in range(60):                        # random coefficients, both sums below 256
        cf, pos, neg = [], 0, 0
        for _ in range(10):
            c = rng.below(103) - 51
            if pos + max(c, 0) >= 256 or neg + max(-c, 0) >= 256:
                c = 0
            pos, neg = pos + max(c, 0), neg + max(-c, 0)
            cf.append(c)
        rows.append(("random %d" % i, rnd(), cf))
    for _, ys, cf in rows:
        assert len(ys) == 10 and len(cf) == 10 and all(0 <= y < p for y in ys)
        assert sum(c for c in cf if c > 0) < 256 and sum(-c for c in cf if c < 0) < 256
    return rows


@pytest.mark.parametrize("curve", CURVES)
def test_fq_lincomb_reduces_every_small_multiple(gpu, curve):
    """one `lincomb` of ten operands: t = pos + 256 p - neg up to 511 p, reduced by reduce_top's float quotient estimate and one
    conditional subtraction; the rows put t on exact multiples of p, at both ends of its range and on the squaring's own rows"""
    t = T.tower(curve)
    rows = lincomb_rows(t)
    a = np.stack([t.raw_words(ys) for _, ys, _ in rows])
    cf = np.array([c for _, _, c in rows], dtype=np.int16)
    got = gpu.pairing_op(curve, "fq_lincomb", a, coeffs=cf)
    # a Montgomery representative is linear in its value: the expected word is the same combination of the words
    want = t.raw_words([sum(c * y for c, y in zip(c_, ys)) % t.p for _, ys, c_ in rows])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, ("%d wrong, first:" % bad.size, rows[int(bad[0])], got[bad[0]].tolist(), want[bad[0]].tolist())
    assert (gpu.pairing_op(curve, "fq_lincomb", a[:1], coeffs=cf[:1]) == got[:1]).all()   # n = 1


@pytest.mark.parametrize("curve", CURVES)
def test_fq_half_and_fq2_products_on_the_edge_list_crossed_with_itself(gpu, curve):
    t = T.tower(curve)
    p = t.p
    edges = t.edge_representatives()
    val = t.mont_value
    got = gpu.pairing_op(curve, "fq_half", t.raw_words(edges))
    want = t.fq_words([val(y) * pow(2, -1, p) % p for y in edges])
    assert (got == want).all(), [hex(y) for y, g, w in zip(edges, got, want) if (g != w).any()]
    n = len(edges)
    a = [(x, y) for x in edges for y in edges]
    b = [(y, edges[(i + 3) % n]) for i, x in enumerate(edges) for y in edges]
    av, bv = [(val(x), val(y)) for x, y in a], [(val(x), val(y)) for x, y in b]
    aw, bw = t.raw_words([v for c in a for v in c]).reshape(len(a), -1), t.raw_words([v for c in b for v in c]).reshape(len(b), -1)
    for what, bb, bbv in (("a b", bw, bv), ("a a", aw, av)):
        got = gpu.pairing_op(curve, "fq2_mul", aw, bb)
        want = t.f2_words([t.f2_mul(x, y) for x, y in zip(av, bbv)])
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, ("fq2_mul", what, [hex(v) for v in a[int(bad[0])]], got[bad[0]].tolist(), want[bad[0]].tolist())
    got = gpu.pairing_op(curve, "fq2_mul_xi", aw)
    want = t.f2_words([t.f2_mul_xi(x) for x in av])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, ("fq2_mul_xi", [hex(v) for v in a[int(bad[0])]], got[bad[0]].tolist(), want[bad[0]].tolist())


# ------------------------------------------------------------------------------------------------ refusals, next to a call that works
@pytest.mark.parametrize("curve", CURVES)
def test_pairing_op_refuses_coefficient_sums_of_256(gpu, curve):
    t = T.tower(curve)
    a = np.stack([t.raw_words([t.p - 1] * 10)])
    ok = gpu.pairing_op(curve, "fq_lincomb", a, coeffs=np.array([[255] + [0] * 8 + [-255]], dtype=np.int16))
    assert (ok == 0).all()
    for cf in ([255, 1] + [0] * 8, [-255, -1] + [0] * 8, [128] * 2 + [0] * 8, [-26] * 10, [256] + [0] * 9, [0] * 9 + [-256]):
        with pytest.raises(gpu.MantaGpuError) as e:
            gpu.pairing_op(curve, "fq_lincomb", a, coeffs=np.array([cf], dtype=np.int16))
        assert e.value.status == 1, cf
