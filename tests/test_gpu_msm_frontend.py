"""GPU parity of the MSM front end, stage by stage and exact: the digit kernel (msm_digits.h, through `mg_msm_digits`) and the
radix sort (sort.hip, through `mg_sort_pairs`) -- the kernels msm_launch runs -- against the plain-integer reference of
tests/msm_frontend_ref.py (itself checked without a GPU by tests/test_msm_frontend_ref.py). A failure names the pair.

What an MSM result cannot show and these tests do: the sort's stability (values = arange), where both stages write (the output
arrays start as sentinels; whatever lies past the pair count must still hold them), every radix pass count 1-4 with both
ping-pong parities, more than 256 tiles per histogram row, and each window of each scalar of the digit recoding.

The sort's precondition, which is the engine's: every key is below 2^end_bit (in masked mode: every effective key).
The order of the compacted pair stream is unspecified by design and not asserted: it is compared as a sorted multiset."""
import numpy as np
import pytest

import msm_frontend_ref as R
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu

KEY_SENTINEL, VAL_SENTINEL = 0xA5A5A5A5, 0x5A5A5A5A  # no key reaches 2^24, no base index 0x5A5A5A5A here
CS = {0: (2, 5, 8, 13, 16, 17), 1: (2, 5, 8, 13, 15, 16, 17)}
NS = (1, 63, 64, 65, 257, 1025)


# ---------------------------------------------------------------------------------------------------------------- inputs
def scalar_vector(curve, c, n, seed, canonical_only=False):
    """n integers: uniform (even seed) or witness-like scalars with the edge set mixed in. From three waves on: wave 0 holds ONE
    unreduced scalar among canonical ones, wave 1 canonical scalars only (all reduced edges), wave 2 every edge, unreduced ones
    included -- the reduction loop leaves wave-uniformly. Shorter vectors: every edge that fits, rotated by the seed."""
    r = synth.FR_MODULUS[curve]
    vec = [int(x) for x in synth.limbs_to_ints(synth.msm_scalars(curve, n, "W" if seed & 1 else "U", seed=1000 + seed))]
    red, unred = R.edge_scalars(curve, c), R.edge_scalars(curve, c, unreduced=True)[-5:]
    if canonical_only:
        unred = [u % r for u in unred]
    if n >= 192:
        vec[7] = unred[seed % 5]
        for t, e in enumerate(red):
            vec[64 + 2 * t] = e
        for t, e in enumerate(red + unred):
            vec[128 + t] = e
    else:
        every = red + unred
        for t in range(min((n + 1) // 2, len(every))):
            vec[2 * t] = every[(t + seed) % len(every)]
    return vec


def limbs(curve, vecs, mont):
    """[batch, n, 4] uint64: the integers themselves, or -- `mont` -- the Montgomery words of the same integers mod r"""
    r = synth.FR_MODULUS[curve]
    return np.stack([synth.to_mont([k % r for k in v], r, 4) if mont else synth.ints_to_limbs(v, 4) for v in vecs])


def first_difference(p, got_k, got_v, want_k, want_v):
    bad = np.flatnonzero((got_k != want_k) | (got_v != want_v))
    if not len(bad):
        return ""
    q, rem = divmod(int(bad[0]), p.W * p.n)
    w, i = divmod(rem, p.n)
    return "%d of %d pairs differ; first: vector %d window %d base %d: got (key %#x, val %#x), want (key %#x, val %#x)" % (
        len(bad), len(want_k), q, w, i, got_k[bad[0]], got_v[bad[0]], want_k[bad[0]], want_v[bad[0]])


def check_fixed(gpu, curve, c, n, vecs, modes=(False, True), **kw):
    """fixed layout: arrays equal to the reference's, for the integers as given and as Montgomery words"""
    p = R.Pairs(curve, vecs, c, n, **kw)
    want_k, want_v = p.fixed()
    for mont in modes:
        got = gpu.msm_digits(curve, limbs(curve, vecs, mont), c, n, mont=mont, keys=np.full(len(want_k), KEY_SENTINEL, dtype=np.uint32),
                             vals=np.full(len(want_k), VAL_SENTINEL, dtype=np.uint32), **kw)
        assert (got["W"], got["B"], got["seg_keys"], got["invalid"]) == (p.W, p.B, p.seg_keys, p.invalid)
        diff = first_difference(p, got["keys"], got["vals"], want_k, want_v)
        assert not diff, "curve %d c %d n %d batch %d mont %d %r: %s" % (curve, c, n, len(vecs), mont, sorted(kw), diff)
    return p, want_k, want_v


def check_compact(gpu, curve, c, n, vecs, mont, **kw):
    """compact layout: the count, the pairs as a multiset, and the sentinels from the count on"""
    p = R.Pairs(curve, vecs, c, n, **kw)
    size, want = len(vecs) * p.W * n, p.compact()
    got = gpu.msm_digits(curve, limbs(curve, vecs, mont), c, n, mont=mont, compact=True, keys=np.full(size, KEY_SENTINEL, dtype=np.uint32),
                         vals=np.full(size, VAL_SENTINEL, dtype=np.uint32), **kw)
    tag = "curve %d c %d n %d batch %d mont %d %r" % (curve, c, n, len(vecs), mont, sorted(kw))
    cnt = got["count"]
    assert cnt == len(want), "%s: count %d, non-zero digits %d" % (tag, cnt, len(want))
    assert (got["keys"][cnt:] == KEY_SENTINEL).all() and (got["vals"][cnt:] == VAL_SENTINEL).all(), tag + ": a write past the pair count"
    have = R.sorted_pairs(got["keys"][:cnt], got["vals"][:cnt])
    bad = np.flatnonzero((have != want).any(axis=1))
    assert not len(bad), "%s: %d pairs differ as sorted multisets; first: got %s, want %s" % (tag, len(bad), have[bad[0]], want[bad[0]])
    return got


# ---------------------------------------------------------------------------------------------------------- digit kernel
@pytest.mark.parametrize("curve,c", [(curve, c) for curve in (0, 1) for c in CS[curve]])
def test_digits_fixed_layout(gpu, curve, c):
    for n in NS:
        if n == 1:  # one lane: every edge scalar in turn
            for k in R.edge_scalars(curve, c, unreduced=True):
                check_fixed(gpu, curve, c, 1, [[k]])
        for batch in (1, 3):
            check_fixed(gpu, curve, c, n, [scalar_vector(curve, c, n, 10 * n + 3 * batch + q) for q in range(batch)])


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("table_mode", [1, 2])
def test_digits_fixed_layout_with_tables(gpu, curve, table_mode):
    """a table per window: the windows share one bucket range and the value carries the window; full tables: one key per vector
    and the value addresses the multiple"""
    for c in ((5, 13, 17) if table_mode == 1 else (2, 8, 12)):
        for n, batch in ((65, 3), (257, 1), (257, 3)):
            check_fixed(gpu, curve, c, n, [scalar_vector(curve, c, n, 7 * n + c + q) for q in range(batch)], table_mode=table_mode)


@pytest.mark.parametrize("curve", [0, 1])
def test_digits_fixed_layout_with_a_shuffled_map_and_a_short_scalar_vector(gpu, curve):
    """stored base i takes scalar map[i]: a shuffled strict subset of 200 entries, with fewer scalars than max(map) + 1 -- the
    entries beyond the vector, the last lane of wave 0 among them, have no scalar and so no digit"""
    n_orig, n, c = 200, 128, 8
    rng = np.random.RandomState(5 + curve)
    mp = rng.permutation(n_orig)[:n].astype(np.uint32)
    for lane, rank in ((63, -1), (127, -2)):  # the last lanes of both waves hold the two largest indices
        at = int(np.argsort(mp)[rank])
        mp[[lane, at]] = mp[[at, lane]]
    n_scalars = int(mp[127])
    assert len(set(mp.tolist())) == n < n_orig and n_scalars < mp.max() + 1 and (mp >= n_scalars).sum() == 2 and mp[63] > mp[127]
    for batch in (1, 2):
        vecs = [scalar_vector(curve, c, n_scalars, 40 + q) for q in range(batch)]
        for table_mode in (0, 1):
            p, keys, _ = check_fixed(gpu, curve, c, n, vecs, table_mode=table_mode, map=mp, set_len=n_orig)
            assert (keys.reshape(batch, p.W, n)[:, :, [63, 127]] == p.invalid).all()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n_sets", [2, 3])
def test_digits_fixed_layout_with_concatenated_queries(gpu, curve, n_sets):
    """n_sets queries of 50 entries over ONE scalar vector of 47: the query boundaries (lanes 50, 100) fall inside waves 0 and 1,
    every (vector, query) has its own key range, entries 47-49 of each query have no scalar"""
    set_len, n_scalars, c = 50, 47, 8
    for batch in (1, 2):
        vecs = [scalar_vector(curve, c, n_scalars, 60 + q) for q in range(batch)]
        for table_mode in (0, 2):
            check_fixed(gpu, curve, c, n_sets * set_len, vecs, table_mode=table_mode, n_sets=n_sets, set_len=set_len)


@pytest.mark.parametrize("curve,c", [(0, 2), (0, 8), (0, 17), (1, 5), (1, 15), (1, 17)])
def test_digits_compact_layout(gpu, curve, c):
    for n in (1, 65, 257, 1025):  # 257, 1025: the last workgroup of 256 holds one lane
        for batch in (1, 3):
            check_compact(gpu, curve, c, n, [scalar_vector(curve, c, n, 20 * n + batch + q) for q in range(batch)], mont=(n + batch) % 2 == 1)


@pytest.mark.parametrize("curve", [0, 1])
def test_digits_compact_layout_special_cases(gpu, curve):
    r, c = synth.FR_MODULUS[curve], 8
    # nothing but zeros (r among them, unreduced): count 0, nothing written
    got = check_compact(gpu, curve, c, 300, [[0] * 299 + [r]], mont=False)
    assert got["count"] == 0
    # exactly one non-zero digit: 77 in window 3 of the next-to-last lane
    vec = [0] * 300
    vec[298] = 77 << (3 * c)
    got = check_compact(gpu, curve, c, 300, [vec, [0] * 300], mont=True)
    assert got["count"] == 1 and got["keys"][0] == 3 * 128 + 76 and got["vals"][0] == 298
    # a partial last workgroup with tables, a map and a short vector
    mp = np.random.RandomState(9).permutation(400)[:300].astype(np.uint32)
    for table_mode in (1, 2):
        check_compact(gpu, curve, c, 300, [scalar_vector(curve, c, 390, 70 + q) for q in range(2)], mont=False, table_mode=table_mode, map=mp,
                      set_len=400)
    # concatenated queries; on full tables with one vector the engine launches the kernel once per query (lanes from i_first
    # on) and relies on the stream coming out grouped by query, which is what spares that MSM its sort
    for table_mode, batch in ((0, 1), (0, 2), (2, 2), (2, 1)):
        got = check_compact(gpu, curve, c, 150, [scalar_vector(curve, c, 47, 80 + q) for q in range(batch)], mont=True, table_mode=table_mode,
                            n_sets=3, set_len=50)
    keys = got["keys"][:got["count"]]
    assert set(keys.tolist()) == {0, 1, 2} and (np.diff(keys.astype(np.int64)) >= 0).all(), "per-query launches: pairs not grouped by query"


# ------------------------------------------------------------------------------------------------------------------ sort
DISTRIBUTIONS = ("uniform", "all_equal", "top_bit", "descending", "distinct_digits", "one_digit", "digits_0_255")


def sort_keys(dist, n, end_bit, rng):
    """n keys below 2^end_bit"""
    top = (1 << end_bit) - 1
    i = np.arange(n, dtype=np.int64)
    group, lane = i // 64, i % 64
    if dist == "uniform":
        k = rng.randint(0, top + 1, size=n, dtype=np.int64)
    elif dist == "all_equal":  # the largest key there is
        k = np.full(n, top, dtype=np.int64)
    elif dist == "top_bit":  # two values that differ in the top sorted bit only
        k = (0x2B5C93A7 & (top >> 1)) | (rng.randint(0, 2, size=n, dtype=np.int64) << (end_bit - 1))
    elif dist == "descending":  # strictly, from the largest key down (wrapping where n exceeds the key space)
        k = (top - i) % (top + 1)
    elif dist == "distinct_digits":  # every 64-element group: 64 different digits in every pass, lanes shuffled
        k = ((((lane * 37 + group) % 64) * 4 + group % 4) & 255) * 0x01010101
    elif dist == "one_digit":  # every group one digit: all 64 lanes are peers of the ballot match
        k = ((group * 7) & 255) * 0x01010101
    else:  # every pass sees the digits 0 and 255 only
        k = sum((rng.randint(0, 2, size=n, dtype=np.int64) * 255) << (8 * p) for p in range(4))
    return (k & top).astype(np.uint32)


def check_sort(gpu, keys, vals, end_bit, tag, **kw):
    n = len(keys)
    ko, vo = np.full(n, KEY_SENTINEL, dtype=np.uint32), np.full(n, VAL_SENTINEL, dtype=np.uint32)
    want_k, want_v = R.sort_pairs(keys, vals, keys_out=ko, vals_out=vo, **kw)
    got_k, got_v = gpu.sort_pairs(keys, vals, end_bit, keys_out=ko, vals_out=vo, **kw)
    bad = np.flatnonzero((got_k != want_k) | (got_v != want_v))
    assert not len(bad), "%s: %d of %d outputs differ; first at %d: got (key %#x, val %#x), want (key %#x, val %#x)" % (
        tag, len(bad), n, bad[0], got_k[bad[0]], got_v[bad[0]], want_k[bad[0]], want_v[bad[0]])
    return got_k, got_v


@pytest.mark.parametrize("end_bit", [1, 8, 9, 16, 17, 24, 25, 32])
def test_sort_is_stable_at_every_pass_count(gpu, end_bit):
    """1-4 radix passes (odd: the first pass writes the output pair, even: the scratch pair), sizes within one of the 64-lane,
    1024-per-wave and 4096-per-tile boundaries; values = positions, so an unstable pass shows"""
    rng = np.random.RandomState(end_bit)
    for n in (1, 63, 64, 65, 1023, 1025, 4095, 4096, 4097, 8193):
        for dist in DISTRIBUTIONS:
            check_sort(gpu, sort_keys(dist, n, end_bit, rng), np.arange(n, dtype=np.uint32), end_bit, "n %d end_bit %d %s" % (n, end_bit, dist))


@pytest.mark.parametrize("n", [257 * 4096 + 3, 513 * 4096 - 1])
@pytest.mark.parametrize("end_bit", [8, 17, 32])
def test_sort_with_more_than_256_tiles(gpu, n, end_bit):
    """every lane of the row scan owns 2 (257 tiles: most lanes own none) or 3 (513 tiles) histogram entries"""
    rng = np.random.RandomState(end_bit + n % 97)
    for dist in ("uniform", "descending", "top_bit"):
        check_sort(gpu, sort_keys(dist, n, end_bit, rng), np.arange(n, dtype=np.uint32), end_bit, "n %d end_bit %d %s" % (n, end_bit, dist))


@pytest.mark.parametrize("end_bit", [16, 17])
def test_sort_device_count_leaves_the_rest_untouched(gpu, end_bit):
    """the pair count read on the device: nothing, one pair, all of them, a tile boundary and its neighbours, wave boundaries (64
    lanes, 1024 elements); both outputs keep the caller's values from the count on"""
    n = 3 * 4096 + 100
    rng = np.random.RandomState(end_bit)
    keys, vals = sort_keys("uniform", n, end_bit, rng), np.arange(n, dtype=np.uint32)
    for count in (0, 1, n, 4095, 4096, 4097, 8191, 8192, 8193, 64, 1024, 4096 + 1024, 4096 + 1024 + 64):
        got_k, got_v = check_sort(gpu, keys, vals, end_bit, "n %d end_bit %d count %d" % (n, end_bit, count), count=count)
        assert (got_k[count:] == KEY_SENTINEL).all() and (got_v[count:] == VAL_SENTINEL).all()


@pytest.mark.parametrize("batch,seg,per_vector", [(3, 128, 3000), (32, 1 << 13, 1500), (2, 1, 700)])
def test_sort_masked_mode_keeps_every_run_contiguous(gpu, batch, seg, per_vector):
    """what msm_launch asks of a batched pass in the fixed layout: keys q seg + bucket arrive vector by vector, mixed with the
    invalid key batch seg; a STABLE sort by the bucket bits leaves every (q, bucket) run contiguous and the invalid keys last"""
    rng = np.random.RandomState(batch)
    invalid = batch * seg
    q = np.repeat(np.arange(batch, dtype=np.int64), per_vector)
    keys = q * seg + rng.randint(0, seg, size=len(q), dtype=np.int64)
    keys[rng.randint(0, 10, size=len(q)) < 3] = invalid
    keys = keys.astype(np.uint32)
    end_bit = int(seg).bit_length()  # bits(seg) + 1: the bucket bits and one value for the invalid key
    got_k, got_v = check_sort(gpu, keys, np.arange(len(keys), dtype=np.uint32), end_bit, "masked batch %d seg %d" % (batch, seg),
                              lowmask=seg - 1, inv_from=invalid)
    n_inv = int((keys == invalid).sum())
    assert n_inv and (got_k[len(keys) - n_inv:] == invalid).all() and (got_k[:len(keys) - n_inv] != invalid).all()
    runs = 1 + int((np.diff(got_k.astype(np.int64)) != 0).sum())
    assert runs == len(np.unique(keys)), "a (vector, bucket) run is split: %d runs for %d keys" % (runs, len(np.unique(keys)))
    for k in np.unique(keys)[:50]:  # inside a run the input order survives
        assert (np.diff(got_v[got_k == k].astype(np.int64)) > 0).all()


# ----------------------------------------------------------------------------------------------------------- both stages
@pytest.mark.parametrize("curve", [0, 1])
def test_digits_then_sort_as_msm_launch_chains_them(gpu, curve):
    """a batch of 3 in the fixed layout, sorted with the parameters launch_reserve chooses: a table per window at c = 8 (128 keys
    per vector, a power of two: sorted by the bucket bits, 8 bits for 9) and plain bases at c = 5 (the full key)"""
    n, batch = 300, 3
    for c, table_mode, masked in ((8, 1, True), (5, 0, False)):
        vecs = [scalar_vector(curve, c, n, 90 + q) for q in range(batch)]
        p = R.Pairs(curve, vecs, c, n, table_mode)
        end_bit, lowmask, inv_from = R.launch_sort_params(p.seg_keys, p.invalid, batch, 1)
        assert (lowmask == p.seg_keys - 1 and inv_from == p.invalid and end_bit == 8) if masked else lowmask == 0xFFFFFFFF
        got = gpu.msm_digits(curve, limbs(curve, vecs, False), c, n, table_mode=table_mode)
        want_k, want_v = R.sort_pairs(*p.fixed(), lowmask=lowmask, inv_from=inv_from)
        got_k, got_v = gpu.sort_pairs(got["keys"], got["vals"], end_bit, lowmask=lowmask, inv_from=inv_from)
        bad = np.flatnonzero((got_k != want_k) | (got_v != want_v))
        assert not len(bad), "curve %d c %d: %d sorted pairs differ, first at %d" % (curve, c, len(bad), bad[0])
