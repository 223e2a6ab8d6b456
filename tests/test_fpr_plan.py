"""The column plan of the reduced-radix products (fpr_dev.h `fpr_column_plan`, read through `mg_fpr_column_plan`) against exact
column bounds recomputed here with Python integers from params_gen.h's RR_P / RR_LB / RR_K. No GPU: the plan is a compile-time
table of the library.

A product adds the limb products of column k group by group into one 64-bit accumulator -- a*b, then c*d (fused product only),
then m*p -- and may move the accumulator's upper part aside ("flush") before a group. Worst cases, all limbs normalised:
carry-in = floor(worst total of column k-1 / 2^LB); a*b and c*d = n (2^LB - 1)^2 for the n products of the column (a squaring's
doubled cross products sum to the same); m*p = (2^LB - 1) * sum of the limbs of p the column touches; after a flush the
accumulator holds at most 2^LB - 1."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"bn254_fr": "Bn254FrCfg", "bn254_fq": "Bn254FqCfg", "bls381_fr": "Bls381FrCfg", "bls381_fq": "Bls381FqCfg"}
KINDS = ("mul", "sqr", "mul_add")
AB, CD, MP = 1, 2, 4  # flush before the a*b / c*d / m*p group


def _params():
    src = open(os.path.join(ROOT, "manta_rs_amd", "csrc", "params_gen.h")).read()
    out = {}
    for field, name in STRUCTS.items():
        body = src[src.index("struct %s {" % name):]
        body = body[:body.index("\n};")]
        lb = int(re.search(r"RR_LB = (\d+);", body).group(1))
        k = int(re.search(r"RR_K = (\d+);", body).group(1))
        limbs = [int(x, 16) for x in re.findall(r"0x[0-9a-f]+", re.search(r"RR_P\[\d+\] = \{(.*?)\}", body).group(1))]
        assert len(limbs) == k and all(x < 1 << lb for x in limbs)
        out[field] = (limbs, lb, k)
    return out


PARAMS = _params()


def groups(field, kind, k):
    """worst-case sums of the groups of column k, in the order the code adds them: [(flush bit, sum)]"""
    P, LB, K = PARAMS[field]
    L = (1 << LB) - 1
    lo, hi = (0, k) if k < K else (k - K + 1, K - 1)
    ab = (hi - lo + 1) * L * L
    mp = L * sum(P[k - i] for i in range(lo, hi + 1))
    return [(AB, ab)] + ([(CD, ab)] if kind == "mul_add" else []) + [(MP, mp)]


def exact_plan(field, kind):
    """flush before a group exactly when adding it could reach 2^64"""
    P, LB, K = PARAMS[field]
    L, carry, plan = (1 << LB) - 1, 0, []
    for k in range(2 * K - 1):
        acc, total, bits = carry, carry, 0
        for bit, g in groups(field, kind, k):
            if acc + g >= 1 << 64:
                bits |= bit
                acc = L
            acc += g
            total += g
        plan.append(bits)
        carry = total >> LB
    return plan


def replay(field, kind, plan):
    """the worst-case accumulator value of every column under `plan`"""
    P, LB, K = PARAMS[field]
    L, carry, peaks = (1 << LB) - 1, 0, []
    for k in range(2 * K - 1):
        acc, total, peak, spill = carry, carry, 0, 0
        for bit, g in groups(field, kind, k):
            if plan[k] & bit:
                spill += acc >> LB
                acc = L
            acc += g
            total += g
            peak = max(peak, acc)
        assert spill < 1 << 64
        peaks.append(peak)
        carry = total >> LB
    return peaks


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", sorted(STRUCTS))
def test_library_plan_flushes_exactly_where_the_bound_requires(field, kind):
    from manta_rs_amd import api
    P, LB, K = PARAMS[field]
    got = api.fpr_column_plan(field, kind)
    assert got["limb_bits"] == LB and len(got["flush"]) == 2 * K - 1 and (K, LB) == api.FPR_LIMBS[field]
    assert got["flush"] == exact_plan(field, kind)
    peaks = replay(field, kind, got["flush"])
    assert max(peaks) < 1 << 64  # replaying the library's plan with worst-case group sums never reaches 2^64
    assert got["peak"] == peaks  # ... and the library's own bookkeeping (its static_assert) saw the same values
    if kind != "mul_add":
        assert not any(b & CD for b in got["flush"])
    if LB < 30:  # 28- and 29-bit limbs: nothing flushes, the group-by-group routines are not even selected
        assert not any(got["flush"]) and not got["flushed_routines"]
    else:
        assert got["flushed_routines"]
        # dropping any one flush of the plan overflows its column: every flush is needed
        for k, bits in enumerate(got["flush"]):
            for bit in (AB, CD, MP):
                if bits & bit:
                    fewer = list(got["flush"])
                    fewer[k] &= ~bit
                    assert replay(field, kind, fewer)[k] >= 1 << 64, (k, bit)


def test_bls381_fq_flush_columns():
    from manta_rs_amd import api
    for kind in ("mul", "sqr"):
        flush = api.fpr_column_plan("bls381_fq", kind)["flush"]
        assert [k for k, b in enumerate(flush) if b] == [10, 11, 12, 13, 14]
        assert all(b in (0, MP) for b in flush)  # one flush, between the a*b and the m*p group
    fused = api.fpr_column_plan("bls381_fq", "mul_add")["flush"]
    assert sum(bin(b).count("1") for b in fused) == 18 and not any(b & AB for b in fused)
    # the count rule this plan replaced (flush when 2 n > 15, and before m*p when 3 n > 15) asked for 11 and 26
    n = [min(k + 1, 25 - k) for k in range(25)]
    assert sum(2 * x > 15 for x in n) == 11 and sum(2 * (2 * x > 15) + (2 * x <= 15 < 3 * x) for x in n) == 26


def test_plan_rejects_unknown_field_and_kind():
    from manta_rs_amd import api
    import ctypes
    cols = ctypes.c_int(0)
    assert api.LIB.mg_fpr_column_plan(7, 0, None, None, ctypes.byref(cols), None, None) != 0
    assert api.LIB.mg_fpr_column_plan(3, 3, None, None, ctypes.byref(cols), None, None) != 0
    assert api.LIB.mg_fpr_column_plan(3, 0, None, None, ctypes.byref(cols), None, None) == 0 and cols.value == 25
