"""GPU parity of radix_scatter's ranking through per-wave LDS lane masks (sort.hip, through `mg_sort_pairs`): every wave-step ORs
lane bits into the masks of the digits it holds, ranks from them and clears them again. The key patterns fill one mask with all
64 lanes, 64 masks with one lane each, two masks with the alternate lanes, and the first and last entry of the table; the sizes
end inside a wave-step, at a wavefront's slice, at half a tile and at a tile. Keys AND values are compared exactly against a
NumPy stable sort on the sort key; the values are the positions, so a pass that is not stable shows in them.

The same file has to pass on the library built with -DMG_SCATTER_MASKS=0 (the eight-ballot ranking), selected through MANTA_LIB."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096
NS = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097, 3 * TILE + 17]
END_BITS = [8, 16, 17, 24]  # one, two, three (the third over one bit) and three full passes
PATTERNS = ["all_equal", "digit_is_lane", "two_by_lane", "first_and_last", "same_pass_byte"]
KEY_SENTINEL, VAL_SENTINEL = 0xDEADBEEF, 0xABCD1234


def make_keys(pattern, n, end_bit):
    """keys below 2^end_bit; the pattern is laid over every byte of the key, so that every pass meets it"""
    i = np.arange(n, dtype=np.uint64)
    lane = i % 64
    top = np.uint64((1 << end_bit) - 1)
    rep = np.uint64(0x010101)  # a byte in all three digits
    if pattern == "all_equal":  # one mask fills to 64 bits and is cleared 16 times per wavefront
        k = np.full(n, 0x5AA5A5, dtype=np.uint64)
    elif pattern == "digit_is_lane":  # all 64 digits of a wave-step distinct: 64 masks of one bit
        k = lane * rep
    elif pattern == "two_by_lane":  # even lanes one digit, odd lanes another: two masks of 32 interleaved bits
        k = np.where(lane % 2 == 0, np.uint64(0x17), np.uint64(0xE8)) * rep
    elif pattern == "first_and_last":  # table entries 0 and 255 only, in runs of three
        k = np.where((i // 3) % 2 == 0, np.uint64(0), np.uint64(0xFF)) * rep
    else:  # same_pass_byte: equal in the low byte, different in the second (and equal again in the third): the second pass must
        # keep the order the first pass left, the first and third must keep the input's
        k = np.uint64(0x3C) | (((i * np.uint64(7)) % np.uint64(256)) << np.uint64(8)) | np.uint64(0xA50000)
    return (k & top).astype(np.uint32)


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
def test_mask_patterns_at_every_size(gpu, end_bit, pattern):
    for n in NS:
        check(gpu, make_keys(pattern, n, end_bit), end_bit, "%s n %d end_bit %d" % (pattern, n, end_bit))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("count", [1, 37, 64 + 5, 1024 + 63, TILE + 2 * 64 + 1, 2 * TILE + 1024 + 33])
def test_device_count_ends_inside_a_wave_step(gpu, count, pattern):
    """a 3-tile buffer of which `count` pairs exist (read on the device), the count ending inside a 64-lane step of the first, a
    later and the last wave-step of a wavefront: the lanes past it hold keys of the SAME digits as the lanes before it (the
    patterns go on through the buffer), and must neither set mask bits nor be written out"""
    n = 3 * TILE
    for end_bit in END_BITS:
        check(gpu, make_keys(pattern, n, end_bit), end_bit, "%s count %d end_bit %d" % (pattern, count, end_bit), count=count)


@pytest.mark.parametrize("n", [65, 2047, TILE + 1, 3 * TILE + 17])
def test_masked_mode(gpu, n):
    """keys q seg + bucket of a batch of 3 with the invalid key 3 seg and keys above it mixed in, sorted by the bucket bits alone
    (lowmask = seg - 1) and everything from inv_from up behind every bucket, stably; seg = 256 puts the invalid keys into a
    second pass of their own"""
    for seg in (128, 256):
        batch, invalid = 3, 3 * seg
        rng = np.random.RandomState(n + seg)
        keys = (rng.randint(0, batch, size=n) * seg + rng.randint(0, seg, size=n)).astype(np.uint32)
        at = rng.rand(n)
        keys[at < 0.2] = invalid
        keys[(at >= 0.2) & (at < 0.3)] = invalid + 5  # above inv_from: the same sort key as the invalid key
        keys[0] = keys[-1] = invalid
        check(gpu, keys, int(seg).bit_length(), "masked n %d seg %d" % (n, seg), lowmask=seg - 1, inv_from=invalid)


def test_back_to_back_inputs_share_nothing(gpu):
    """two different inputs through the same call path, there and back: a mask or a count left over from one call (or from the
    tile before) would show in the next"""
    n, end_bit = 2 * TILE + 65, 16
    a, b = make_keys("all_equal", n, end_bit), make_keys("digit_is_lane", n, end_bit)
    for round_ in range(2):
        check(gpu, a, end_bit, "all_equal, round %d" % round_)
        check(gpu, b, end_bit, "digit_is_lane, round %d" % round_)
        check(gpu, a, end_bit, "all_equal with a count, round %d" % round_, count=TILE + 7)
