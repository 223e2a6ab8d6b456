"""The single-chain coding of the BLS12-381 Fq products (13 x 30-bit limbs): what the accumulate kernel calls -- mul_t / sqr_t /
mul_add_t<true>, reached through `mg_fpr_raw_op` with chain=True, built as the shipped library builds them -- against exact Python
integers, and one small MSM through the accumulate kernel against the oracle.

The coding is the flushed product routine with every multiply-add pinned into one dependent chain (fpr_dev.h mad_link); where a
column flushes is the column plan (`mg_fpr_column_plan`). A flush in the wrong place, or a partial sum moved across one, shows only
on operands whose column sums reach 2^64 without the flush: the all-ones limb vectors. `test_operands_reach_the_planned_flushes`
checks, in exact integers, that the operands used here do reach 2^64, that they do so only in columns the plan flushes, and that
a 64-bit model of the routine that flushes where the plan says is exact on all of them.

Operand bounds (ec_dev.h, bounds comment of the mixed addition): products of values below 11p x 11p, 7p x 7p and the fused
7p x 11p + 4p x 3p. This field has LAZY_LIMBS = false (13 * 13 * 2^60 >= 2^64: a fused column of limbs below 3 * 2^30 does not fit
the accumulator, asserted below with the header's own formula), so subl / negl feed no product of it: the mixed addition takes
`sub` / `neg` there and every product operand has normalised limbs (10p x 10p, 6p x 6p, 6p x 10p + 4p x 2p). The values just under
each of these bounds are therefore given in normalised limbs; limbs of 3 * 2^30 - 1 are outside what either coding of this field
is built for and are not fed."""
import numpy as np
import pytest

import helpers as H
import oracle_lib as O
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu

FIELD = "bls381_fq"
K, LB = 13, 30
L = (1 << LB) - 1
P = synth.FQ_MODULUS[1]
RP = 1 << (K * LB)
NINV = (-pow(P, -1, RP)) % RP
FLUSH_CD, FLUSH_MP = 2, 4


def value(limbs):
    return sum(int(x) << (i * LB) for i, x in enumerate(limbs))


def split(v):
    assert 0 <= v < 1 << ((K - 1) * LB + 32)
    return [(v >> (i * LB)) & L for i in range(K - 1)] + [v >> ((K - 1) * LB)]


def redc(t):
    m = (t * NINV) % RP
    return split((t + m * P) // RP)


def operand_rows():
    """rows (a, b, c, d) of normalised limb vectors"""
    rng = np.random.default_rng(381)
    ones, zero, one, pm1 = [L] * K, [0] * K, split(1), split(P - 1)
    even, odd = [L if i % 2 == 0 else 0 for i in range(K)], [L if i % 2 else 0 for i in range(K)]
    st = [ones, zero, one, pm1, even, odd]
    under = {b: split(b * P - 1) for b in (2, 3, 4, 6, 7, 8, 10, 11)}  # just under each bound of the mixed addition
    rows = [(x, y, z, w) for x in st for y in st for z, w in ((ones, ones), (zero, one), (y, x), (pm1, ones))]
    rows += [(under[11], under[11], under[11], under[11]), (under[10], under[10], under[10], under[10]),
             (under[7], under[7], under[7], under[7]), (under[6], under[6], under[6], under[6]),
             (under[7], under[11], under[4], under[3]), (under[6], under[10], under[4], under[2]),
             (under[8], under[2], under[4], under[2]), (under[11], under[2], under[2], under[2])]
    rows += [(under[x], under[y], ones, ones) for x in under for y in under]
    rows += [(ones, under[x], under[y], ones) for x in under for y in under]
    # limbs close to 2^30 - 1 everywhere: large m as well as large a b, the fullest columns short of all-ones
    for spread in (12, 20, 28):
        rows += [tuple([int(L - x) for x in rng.integers(0, 1 << spread, K)] for _ in range(4)) for _ in range(192)]
    rows += [tuple([int(x) for x in rng.integers(0, L + 1, K)] for _ in range(4)) for _ in range(256)]
    return rows


def column_totals(a, b, c=None, d=None):
    """exact column sums (carry-in included) of the interleaved reduction, no flush and no 64-bit limit"""
    m, carry, out = [0] * K, 0, []
    for k in range(2 * K - 1):
        lo, hi = max(0, k - K + 1), min(k, K - 1)
        tot = carry + sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        if c is not None:
            tot += sum(c[i] * d[k - i] for i in range(lo, hi + 1))
        tot += sum(m[i] * PL[k - i] for i in range(lo, hi + 1) if not (k < K and i == k))
        if k < K:
            m[k] = ((tot & L) * (NINV & L)) & L
            tot += m[k] * PL[0]
        out.append(tot)
        carry = tot >> LB
    return out


PL = split(P)


def model_flushed(flush, a, b, c=None, d=None):
    """the flushed routine in 64-bit arithmetic (every sum taken mod 2^64), flushing where `flush` says"""
    W = (1 << 64) - 1
    m, acc, t = [0] * K, 0, [0] * K
    for k in range(2 * K - 1):
        lo, hi = max(0, k - K + 1), min(k, K - 1)
        spill = 0
        for i in range(lo, hi + 1):
            acc = (acc + a[i] * b[k - i]) & W
        if c is not None:
            if flush[k] & FLUSH_CD:
                spill, acc = spill + (acc >> LB), acc & L
            for i in range(lo, hi + 1):
                acc = (acc + c[i] * d[k - i]) & W
        if flush[k] & FLUSH_MP:
            spill, acc = spill + (acc >> LB), acc & L
        for i in range(lo, hi + 1):
            if not (k < K and i == k):
                acc = (acc + m[i] * PL[k - i]) & W
        if k < K:
            m[k] = ((acc & L) * (NINV & L)) & L
            acc = (acc + m[k] * PL[0]) & W
        else:
            t[k - K] = acc & L
        acc = ((acc >> LB) + spill) & W
    t[K - 1] = acc & 0xffffffff
    return t


@pytest.fixture(scope="module")
def expected():
    rows = operand_rows()
    vals = [tuple(value(x) for x in r) for r in rows]
    return dict(rows=rows,
                mul=np.array([redc(a * b) for a, b, _, _ in vals], dtype=np.uint32),
                sqr=np.array([redc(a * a) for a, _, _, _ in vals], dtype=np.uint32),
                mul_add=np.array([redc(a * b + c * d) for a, b, c, d in vals], dtype=np.uint32))


def test_operands_reach_the_planned_flushes(gpu, expected):
    assert K * 13 * (1 << (2 * LB)) >= 1 << 64  # fpr_dev.h LAZY_LIMBS is false for this field: only normalised limbs reach a product
    rows = expected["rows"]
    for kind in ("mul", "sqr", "mul_add"):
        plan = gpu.fpr_column_plan(FIELD, kind)
        assert plan["limb_bits"] == LB and plan["flushed_routines"] and len(plan["flush"]) == 2 * K - 1
        planned = {k for k, f in enumerate(plan["flush"]) if f}
        if kind != "mul_add":
            assert planned == set(range(10, 15))
        reached = set()
        for n, (a, b, c, d) in enumerate(rows):
            args = (a, b) if kind == "mul" else ((a, a) if kind == "sqr" else (a, b, c, d))
            reached |= {k for k, tot in enumerate(column_totals(*args)) if tot >> 64}
            assert model_flushed(plan["flush"], *args) == expected[kind][n].tolist(), (kind, n)
        print(kind, "columns past 2^64 without a flush:", sorted(reached), "planned:", sorted(planned))
        assert reached and reached <= planned, (kind, sorted(reached), sorted(planned))
        # and without the flushes the 64-bit model is wrong on the all-ones row: the flush is what these operands test
        args = (rows[0][0], rows[0][1]) if kind != "mul_add" else rows[0]
        assert rows[0][0] == [L] * K and model_flushed([0] * (2 * K - 1), *args) != model_flushed(plan["flush"], *args)


def test_chain_products_match_exact_integers(gpu, expected):
    rows = expected["rows"]
    assert 1000 <= len(rows) <= 4000
    a, b, c, d = (np.array([r[i] for r in rows], dtype=np.uint32) for i in range(4))
    for op, args in (("mul", (a, b)), ("sqr", (a,)), ("mul_add", (a, b, c, d))):
        got = gpu.fpr_raw_op(FIELD, op, *args, chain=True)
        bad = np.nonzero((got != expected[op]).any(axis=1))[0]
        assert bad.size == 0, (op, "first wrong row", int(bad[0]), rows[int(bad[0])], got[bad[0]].tolist(), expected[op][bad[0]].tolist())
        assert (got == gpu.fpr_raw_op(FIELD, op, *args, chain=False)).all(), op  # and the two codings agree limb for limb


def test_small_msm_through_the_accumulate_kernel(gpu):
    """n = 4 096 at window 8: 128 buckets per window, so every lane of the accumulate kernel walks runs of several entries and runs
    cross lane boundaries. A base repeated with an equal scalar doubles inside a bucket, one repeated with the opposite scalar
    cancels there."""
    n = 4096
    pts = H.random_points(1, 1, n, seed=4096)
    sc = synth.msm_scalars(1, n, "U", seed=8)
    r = synth.FR_MODULUS[1]
    for i in range(0, 64, 4):  # spread over the sorted stream: different digits in every window
        pts[100 + i + 1] = pts[100 + i]
        sc[100 + i + 1] = sc[100 + i]  # equal digit in every window: P + P
        pts[100 + i + 3] = pts[100 + i + 2]
        k = int(sum(int(x) << (64 * j) for j, x in enumerate(sc[100 + i + 2])))
        sc[100 + i + 3] = synth.ints_to_limbs([r - k], 4)[0]  # r - k is recoded as -k: the opposite digit in every window
    for j, (w, dg) in enumerate(((0, 1), (1, 127), (5, 77), (30, 3))):  # the same without relying on that recoding
        pts[2000 + 2 * j + 1] = pts[2000 + 2 * j]
        sc[2000 + 2 * j] = synth.ints_to_limbs([dg << (8 * w)], 4)[0]              # digit dg in window w
        sc[2000 + 2 * j + 1] = synth.ints_to_limbs([(256 - dg) << (8 * w)], 4)[0]  # digit -dg there, +1 in window w + 1
    want = O.msm(1, 1, pts, sc, algo=1)
    b = gpu.Bases(1, 1, pts)
    got = gpu.VariableBaseMSM.launch(b, gpu.DeviceBuffer.from_numpy(sc), n, window_bits=8).finish()
    assert (got == want).all()
