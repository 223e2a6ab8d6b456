"""GPU parity of the radix sort (sort.hip, through `mg_sort_pairs`) at the sizes where radix_scatter's bookkeeping changes hands:
a lane's 16 keys and packed rank pairs, a wavefront's 1 024-element slice, half a tile, a tile (4 096) and its neighbours. Keys
and values are compared exactly against a NumPy stable sort; the values are the positions, so an unstable pass shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096
NS = [1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 3 * TILE + 17]
END_BITS = [8, 16, 17]
PATTERNS = ["all_equal", "two_digits", "round_robin", "uniform"]
KEY_SENTINEL, VAL_SENTINEL = 0xDEADBEEF, 0xABCD1234


def make_keys(pattern, n, end_bit, seed):
    i = np.arange(n, dtype=np.uint64)
    top = (1 << end_bit) - 1
    if pattern == "all_equal":
        k = np.full(n, 0x1A5A5 & top, dtype=np.uint64)
    elif pattern == "two_digits":  # two keys that differ in every digit of every pass, alternating
        k = np.where(i % 2 == 0, 0x1FE03 & top, 0x001FC & top)
    elif pattern == "round_robin":  # all 256 digits in turn in the low pass, in the opposite order in the second
        k = ((i % 256) | ((255 - (i // 3) % 256) << 8) | ((i % 2) << 16)) & top
    else:
        k = np.random.RandomState(seed).randint(0, top + 1, size=n).astype(np.uint64)
    return k.astype(np.uint32)


def reference(keys, vals, count=None, lowmask=0xFFFFFFFF, inv_from=0xFFFFFFFF):
    """NumPy stable sort of the first `count` pairs by the key the passes sort by; the rest keeps the sentinels"""
    n = len(keys)
    m = n if count is None else count
    by = keys[:m].astype(np.uint64)
    if lowmask != 0xFFFFFFFF:
        by = np.where(keys[:m] >= inv_from, np.uint64(lowmask + 1), by & np.uint64(lowmask))
    order = np.argsort(by, kind="stable")
    ko, vo = np.full(n, KEY_SENTINEL, dtype=np.uint32), np.full(n, VAL_SENTINEL, dtype=np.uint32)
    ko[:m], vo[:m] = keys[:m][order], vals[:m][order]
    return ko, vo


def check(gpu, keys, end_bit, tag, **kw):
    n = len(keys)
    vals = np.arange(n, dtype=np.uint32)
    want_k, want_v = reference(keys, vals, **kw)
    got_k, got_v = gpu.sort_pairs(keys, vals, end_bit, keys_out=np.full(n, KEY_SENTINEL, dtype=np.uint32),
                                  vals_out=np.full(n, VAL_SENTINEL, dtype=np.uint32), **kw)
    bad = np.flatnonzero((got_k != want_k) | (got_v != want_v))
    assert not len(bad), "%s: %d of %d outputs differ; first at %d: got (key %#x, val %#x), want (key %#x, val %#x)" % (
        tag, len(bad), n, bad[0], got_k[bad[0]], got_v[bad[0]], want_k[bad[0]], want_v[bad[0]])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("end_bit", END_BITS)
def test_sizes_around_slice_half_tile_and_tile(gpu, end_bit, pattern):
    """one, two and three passes (17 bits: the third pass sees two digits) at every size of NS"""
    for n in NS:
        check(gpu, make_keys(pattern, n, end_bit, seed=n + end_bit), end_bit, "%s n %d end_bit %d" % (pattern, n, end_bit))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("count", [1, 2047, 2049, 4097])
def test_device_count_inside_a_tile(gpu, count, pattern):
    """a 3-tile buffer of which only `count` pairs exist (read on the device): the count ends inside the first wavefront's slice,
    on either side of half a tile and one element into the second tile; both outputs keep the caller's values from the count on"""
    n = 3 * TILE
    for end_bit in END_BITS:
        check(gpu, make_keys(pattern, n, end_bit, seed=count + end_bit), end_bit, "%s count %d end_bit %d" % (pattern, count, end_bit),
              count=count)


def test_masked_mode_sorts_invalid_keys_behind_every_bucket(gpu):
    """keys q seg + bucket of a batch of 3, vector by vector, mixed with the invalid key 3 seg: sorted by the bucket bits alone
    (lowmask), the keys from inv_from up behind every bucket, stably"""
    seg, batch, per_vector = 128, 3, 2 * TILE // 3 + 7
    invalid = batch * seg
    rng = np.random.RandomState(5)
    keys = np.concatenate([q * seg + rng.randint(0, seg, size=per_vector) for q in range(batch)]).astype(np.uint32)
    keys[rng.rand(len(keys)) < 0.3] = invalid
    keys[0] = keys[-1] = invalid
    check(gpu, keys, int(seg).bit_length(), "masked", lowmask=seg - 1, inv_from=invalid)
    n_inv = int((keys == invalid).sum())
    got_k, _ = gpu.sort_pairs(keys, np.arange(len(keys), dtype=np.uint32), int(seg).bit_length(), lowmask=seg - 1, inv_from=invalid)
    assert (got_k[len(keys) - n_inv:] == invalid).all() and (got_k[:len(keys) - n_inv] != invalid).all()
