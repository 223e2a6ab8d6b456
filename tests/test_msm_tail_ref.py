"""The plain-integer model of the bucket reduce (tests/msm_tail_ref.py) against the closed form, and the census of what the
degenerate inputs of tests/msm_degenerate_inputs.py make the tail additions meet -- for exactly the inputs
tests/test_gpu_msm_degenerate.py runs on the GPU; and the CPU oracle's own MSM on every one of those inputs against the
expected value the GPU results are compared with. No GPU here."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import msm_degenerate_inputs as D
import msm_tail_ref as T
import oracle_lib as O
from manta_rs_amd import synth

CURVES = [0, 1]
FRONT_MIN = 128  # MANTA_RED_MIN=128: front levels from 128 buckets on
KINDS = {7: T.TAIL_WINDOW_SUMS, 9: T.TAIL_X_SUMS, 13: T.TAIL_X_SUMS, 14: T.TAIL_TWO_LEVELS}


def test_classes_are_decided_in_the_order_of_the_adders():
    r = 101
    assert [T.classify(*p, r) for p in ((5, 0), (0, 0), (0, 5), (5, 5), (5, r + 5), (5, r - 5), (5, 6))] == \
        ["o_inf", "o_inf", "a_inf", "dbl", "dbl", "cancel", "general"]


@pytest.mark.parametrize("curve,group", [(0, 1), (1, 1), (0, 2), (1, 2)])
@pytest.mark.parametrize("kind", ["tails", "merge"])
def test_oracle_msm_equals_the_closed_form_on_every_input(curve, group, kind):
    """O.msm(algo=0) over the very arrays the GPU tests run -- every dictated, small-multiple, cancelling and one-point case of
    all four groups -- equals the expected value [sum k_i m_i mod r] G (zeros for a zero sum) that the GPU results are compared
    with. (The oracle's MSM is a pure function of its arguments; the cases run on a few host threads.)"""
    cases, data = D.inputs(curve, group, kind)

    def same(i):
        return bool((O.msm(curve, group, D.points(data["table"], cases[i].mults), data["sc%d" % i], algo=0) == data["want%d" % i]).all())

    with ThreadPoolExecutor(min(8, O.usable_cpus())) as pool:
        ok = list(pool.map(same, range(len(cases))))
    assert all(ok), [c.name for c, good in zip(cases, ok) if not good]
    assert len(cases) == len(D.merge_cases(curve) if kind == "merge" else D.dictated_cases(curve) + D.small_multiple_cases(curve))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("c", D.WIDTHS)
def test_window_sum_is_the_closed_form_for_every_vector_and_layout(curve, c):
    """sum_j (j + 1) v_j mod r from every tail layout, with and without front levels, by the host fold and by fold_windows;
    and some vectors that are not degenerate at all"""
    r = synth.FR_MODULUS[curve]
    rng = synth.XorShift(0x7A11 + c)
    B = 1 << (c - 1)
    vecs = dict(D.vectors(c), random=[rng.field(r) for _ in range(B)], sparse=[rng.field(r) if rng.below(5) == 0 else 0 for _ in range(B)])
    for name, v in vecs.items():
        want = T.closed_form(v, r)
        for min_items in (16384, FRONT_MIN):
            for device in (False, True):
                cs = T.Census(r)
                got, kind = T.window_sum(cs, v, 1, min_items, device)
                assert got == want, (name, min_items, device)
                if min_items == 16384:
                    assert kind == KINDS[c], name
        if name == "zero_total":
            assert want == 0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097, 8191])
def test_window_sum_at_sizes_that_are_no_multiple_of_a_tile_or_a_stretch(n):
    """the reduce over n items for n around the tile and stretch sizes (what the front levels hand on is lanes - 1 items)"""
    r = synth.FR_MODULUS[0]
    rng = synth.XorShift(n)
    v = [rng.field(r) for _ in range(n)]
    for min_items in (16384, FRONT_MIN):
        assert T.window_sum(T.Census(r), v, 1, min_items)[0] == T.closed_form(v, r)


@pytest.mark.parametrize("curve", CURVES)
def test_dictated_cases_fill_the_buckets_they_name(curve):
    """tables: only window 0 is non-zero and bucket j holds v_j; plain bases: windows 0 and 3 hold v, every other window is empty;
    and the whole modelled MSM (window sums, Horner chain) is the case's closed form [k] G"""
    r = synth.FR_MODULUS[curve]
    for case in D.dictated_cases(curve):
        wins = T.bucket_windows(curve, case.mults, case.scalars, case.c, bool(case.pre))
        v = [x % r for x in case.buckets]
        if case.pre:
            assert wins == [v], case.name
            assert case.k == T.closed_form(v, r), case.name
        else:
            assert wins[0] == v and wins[3] == v and not any(any(w) for i, w in enumerate(wins) if i not in (0, 3)), case.name
            assert case.k == T.closed_form(v, r) * (1 + (1 << (3 * case.c))) % r, case.name
        if case.c <= 9:
            assert T.msm(T.Census(r), curve, case.mults, case.scalars, case.c, bool(case.pre)) == case.k, case.name
        if "zero_total" in case.name:
            assert case.k == 0


@pytest.mark.parametrize("curve", CURVES)
def test_census_of_the_small_multiple_inputs(curve):
    """uniform scalars on the eight-point base cycle, plain bases: the modelled MSM is the closed form, and tile_reduce meets
    at least 100 doublings and 100 cancellations per (curve, c); the cancelling input sums to infinity"""
    r = synth.FR_MODULUS[curve]
    for case in D.small_multiple_cases(curve):
        cs = T.Census(r)
        assert T.msm(cs, curve, case.mults, case.scalars, case.c, False) == case.k, case.name
        if "cancels" in case.name:
            assert case.k == 0
        else:
            assert cs.count("tile_reduce", "dbl") >= 100 and cs.count("tile_reduce", "cancel") >= 100, (case.name, dict(cs.n))


@pytest.mark.parametrize("c", D.WIDTHS)
def test_census_of_the_dictated_vectors(c):
    """What each vector makes the scan kernels add, by construction.
    ones: before step d of the suffix scan lane l of a full tile holds min(d, 64 - l) G, so the pair (l, l + d) is a doubling for
    l <= 64 - 2d and general above: 65 - 2d doublings and d - 1 general pairs at d = 1, 2, .. 32 (63, 61, 57, 49, 33, 1) --
    doublings at EVERY scan level, of tile_reduce and, with T0 equal tile totals in lanes 1 .. T0 - 1, of part 0 of reduce_level1
    (max(0, T0 - 2d) of its T0 - 1 - d live pairs). Only the TREE sum over the suffix sums, the distinct multiples 64 - l, is
    general throughout, which is why `general == 0` cannot hold for the whole kernel; part 1 of reduce_level1 sums equal S_t, a
    power of two of them, and is doublings at every level."""
    r = synth.FR_MODULUS[0]
    B, T0 = 1 << (c - 1), (1 << (c - 1)) // 64
    vec = D.vectors(c)

    def census(name, min_items=16384):
        cs = T.Census(r)
        T.window_sum(cs, vec[name], 1, min_items)
        return cs

    first = lambda cs, k: sum(cs.count_at("tile_reduce", (t, "scan", 1), k) for t in range(T0))
    steps = (1, 2, 4, 8, 16, 32)

    def scan_counts(cs, stage, tile, full=64):
        """(dbl, general, cancel) per scan step of one tile of `full` equal items"""
        return [tuple(cs.count_at(stage, (tile, "scan", d), k) for k in ("dbl", "general", "cancel")) for d in steps]

    constant_tile = lambda full=64: [(max(0, full + 1 - 2 * d), min(d - 1, max(0, full - d)), 0) for d in steps]
    assert [x[0] for x in constant_tile()] == [63, 61, 57, 49, 33, 1]
    cs = census("ones")
    for t in range(T0):
        assert scan_counts(cs, "tile_reduce", t) == constant_tile(), t
        for d in steps:  # the tree sum adds the suffix sums (64 - l) G and (64 - l - d) G: d general pairs, no doubling
            assert cs.count_at("tile_reduce", (t, "tree", d), "general") == d == cs.live("tile_reduce", (t, "tree", d))
    assert first(cs, "dbl") == 63 * T0
    assert cs.count("tile_reduce", "cancel") == 0 and cs.count("reduce_level1", "cancel") == 0
    if KINDS[c] == T.TAIL_X_SUMS:
        d, part1 = T0 >> 1, 0
        while d >= 1:
            assert cs.count_at("reduce_level1", (1, "tree", d), "dbl") == d == cs.live("reduce_level1", (1, "tree", d))
            part1, d = part1 + d, d >> 1
        assert part1 == T0 - 1
        d = 1
        while d < T0:  # part 0: lanes 1 .. T0 - 1 hold the equal tile totals 64 G
            dbl, live = max(0, T0 - 2 * d), T0 - 1 - d + (d >= 2)  # (lane 0, empty at first, holds (d - 1) totals: general)
            assert cs.count_at("reduce_level1", (0, "scan", d), "dbl") == dbl, d
            assert cs.live("reduce_level1", (0, "scan", d)) == live and cs.count_at("reduce_level1", (0, "scan", d), "cancel") == 0, d
            d <<= 1
    if KINDS[c] == T.TAIL_TWO_LEVELS:  # the second level scans the equal tile totals A_1 .. A_127 (64 + 63 items) and the 128 equal S_t
        assert scan_counts(cs, "tile_reduce.level1", 0) == constant_tile() and scan_counts(cs, "tile_reduce.level1", 1) == constant_tile(63)
        assert scan_counts(cs, "tile_reduce.sums", 0) == constant_tile() == scan_counts(cs, "tile_reduce.sums", 1)

    cs = census("alternating")  # the first scan step is all cancellations, the rest of the scan adds infinities
    assert first(cs, "cancel") == 63 * T0 == sum(cs.live("tile_reduce", (t, "scan", 1)) for t in range(T0))
    assert all(cs.live("tile_reduce", (t, "scan", 1 << s)) == 0 for t in range(T0) for s in range(1, 6))
    assert cs.n["tile_reduce", "general"] == 0  # (the tree sum adds the odd lanes' suffix sums, all -G: doublings)

    cs = census("lane_mixed")  # all five classes inside every tile (= every wave) at the first scan step
    for t in range(T0):
        for k in T.CLASSES:
            assert cs.count_at("tile_reduce", (t, "scan", 1), k) >= 1, (t, k)

    if "tile_alternating" in vec:
        cs = census("tile_alternating")
        assert all(scan_counts(cs, "tile_reduce", t) == constant_tile() for t in range(T0))  # a constant +-1 inside every tile
        if KINDS[c] == T.TAIL_X_SUMS:  # cancellations in both parts of reduce_level1
            for part in (0, 1):
                assert sum(v for (s, w, k), v in cs.at.items() if s == "reduce_level1" and w[0] == part and k == "cancel") >= 1, part
        else:
            assert cs.count("tile_reduce.level1", "cancel") >= 1 and cs.count("tile_reduce.sums", "cancel") >= 1

    if "front_pattern" in vec:  # both chains of serial_reduce meet sum == acc and sum == -acc
        cs = census("front_pattern", FRONT_MIN)
        for chain in ("serial_reduce.acc", "serial_reduce.sum"):
            assert cs.n[chain, "dbl"] >= 1 and cs.n[chain, "cancel"] >= 1, (chain, dict(cs.n))

    for name in vec:  # with front levels every vector still reaches serial_reduce, and the zero total stays zero
        cs = census(name, FRONT_MIN)
        assert (cs.count("serial_reduce", "a_inf") > 0) == (B >= FRONT_MIN), name


def test_merge_and_small_multiple_cases_have_their_closed_forms():
    """the one-point inputs: k = sum of the scalars (all bases G), 0 where G and -G alternate under pairwise equal scalars"""
    for curve in CURVES:
        r = synth.FR_MODULUS[curve]
        for case in D.merge_cases(curve):
            if "negated" in case.name:
                assert case.k == 0, case.name
            else:
                assert case.k == sum(case.scalars) % r != 0, case.name
            if case.pre < 0:  # full tables: one digit, below 2^(c-1)
                assert len(set(case.scalars)) == 1 and 0 < case.scalars[0] < 32
    assert len(D.TAIL_KNOBS) + 1 <= 8 and len(D.MERGE_KNOBS) <= 8  # children alive at once
