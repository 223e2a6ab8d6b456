"""Plain-integer reference of the MSM front end: the signed window digits of a scalar, the (bucket key, base index | sign)
pairs the digit stage makes of them in both layouts, and the order the pair sort must produce. Python integers and numpy
only; written from the contracts stated in msm_digits.h, engine.h (BaseSet, MsmPlan) and sort.hip, and checked against
the identities of tests/test_msm_frontend_ref.py, which need no GPU.

Scalars are Python integers of any size below 2^256 (they are reduced mod r first, as the kernel's input may be)."""
import numpy as np

from manta_rs_amd import synth

SIGN = 1 << 31


def windows(bits, c):
    return -(-bits // c)


def digits(k, r, bits, c):
    """The non-zero signed c-bit digits of the scalar k as [(window, magnitude, negative)], window-ascending:
    k is reduced mod r, the smaller of k and r - k is written as sum_w d_w 2^(c w) with |d_w| <= B = 2^(c-1) (a window value
    above B borrows 2^c from the next window), and every sign flips when r - k was taken: sum_w +-d_w 2^(c w) = k (mod r).
    No digit lies beyond window ceil(bits / c) - 1 (asserted)."""
    B, full = 1 << (c - 1), 1 << c
    k %= r
    folded = r - k < k
    if folded:
        k = r - k
    out, w = [], 0
    while k:
        d = k % full
        k //= full
        if d > B:
            d -= full
            k += 1
        if d:
            out.append((w, abs(d), (d < 0) != folded))
        w += 1
    assert w <= windows(bits, c), "a carry left the top window"
    return out


def digits_value(ds, c):
    """sum of the signed digits, the integer they stand for"""
    return sum((-m if neg else m) << (c * w) for w, m, neg in ds)


def layout(bits, c, table_mode, batch, n_sets):
    """dict(W, B, seg_keys, invalid): windows, buckets per window, bucket keys per (scalar vector, query) -- W B with plain
    bases (a bucket per window and magnitude), B with a table per window (the windows share their buckets), 1 with full
    tables (the one "bucket" is the result) -- and the key of a zero digit in the fixed layout, one past the last bucket"""
    W, B = windows(bits, c), 1 << (c - 1)
    seg = (W * B, B, 1)[table_mode]
    return dict(W=W, B=B, seg_keys=seg, invalid=batch * n_sets * seg)


class Pairs:
    """The pairs of a digit-stage call. scalars = [batch][n_scalars] integers; n stored bases; stored base i takes the scalar
    of original entry src = map[i] (i without a map), which belongs to query src // set_len and is scalar src % set_len of
    its vector when the set concatenates n_sets > 1 queries; an entry beyond the scalar vector has the scalar 0.
    Digit (m, sign) of window w:  key = (q n_sets + query) seg_keys + {w B + m - 1 | m - 1 | 0},
    value = {i | w n + i | (w n + i) B + m - 1} + sign 2^31  for plain bases | window tables | full tables."""

    def __init__(self, curve, scalars, c, n, table_mode=0, map=None, n_sets=1, set_len=None):
        r, bits = synth.FR_MODULUS[curve], synth.FR_BITS[curve]
        self.batch, self.n = len(scalars), n
        self.__dict__.update(layout(bits, c, table_mode, self.batch, n_sets))
        W, B, seg = self.W, self.B, self.seg_keys
        set_len = n if set_len is None else set_len
        cache = {}
        q_, w_, i_, key_, val_ = [], [], [], [], []
        for q, vec in enumerate(scalars):
            for i in range(n):
                src = i if map is None else int(map[i])
                query, j = (src // set_len, src % set_len) if n_sets > 1 else (0, src)
                k = vec[j] if j < len(vec) else 0
                if k not in cache:
                    cache[k] = digits(k, r, bits, c)
                key0 = (q * n_sets + query) * seg
                for w, m, neg in cache[k]:
                    q_.append(q), w_.append(w), i_.append(i)
                    key_.append(key0 + (w * B + m - 1, m - 1, 0)[table_mode])
                    val_.append((i, w * n + i, (w * n + i) * B + m - 1)[table_mode] + (SIGN if neg else 0))
        self.q, self.w, self.i = (np.array(a, dtype=np.int64) for a in (q_, w_, i_))
        self.key, self.val = np.array(key_, dtype=np.uint32), np.array(val_, dtype=np.uint32)

    def fixed(self):
        """(keys, vals) of the fixed layout: digit (q, w, i) at (q W + w) n + i, zero digits as (invalid, 0)"""
        size = self.batch * self.W * self.n
        keys, vals = np.full(size, self.invalid, dtype=np.uint32), np.zeros(size, dtype=np.uint32)
        at = (self.q * self.W + self.w) * self.n + self.i
        keys[at], vals[at] = self.key, self.val
        return keys, vals

    def compact(self):
        """the pairs of the non-zero digits as a sorted multiset: [count, 2] rows (key, val) in lexicographic order"""
        return sorted_pairs(self.key, self.val)


def sorted_pairs(keys, vals):
    kv = np.stack([np.asarray(keys, dtype=np.uint32), np.asarray(vals, dtype=np.uint32)], axis=1)
    return kv[np.lexsort((kv[:, 1], kv[:, 0]))]


def effective_key(keys, lowmask=0xFFFFFFFF, inv_from=0xFFFFFFFF):
    """what the sort orders by: keys from inv_from up count as lowmask + 1, the others as key & lowmask (plain integers: no wrap)"""
    k = np.asarray(keys).astype(np.int64)
    return np.where(k >= inv_from, lowmask + 1, k & lowmask)


def sort_pairs(keys, vals, lowmask=0xFFFFFFFF, inv_from=0xFFFFFFFF, count=None, keys_out=None, vals_out=None):
    """(keys, vals) after a stable sort of the first `count` pairs (all of them by default) by the effective key; the outputs
    from `count` on keep what keys_out / vals_out held"""
    keys, vals = np.asarray(keys, dtype=np.uint32), np.asarray(vals, dtype=np.uint32)
    m = len(keys) if count is None else count
    ko = np.zeros(len(keys), dtype=np.uint32) if keys_out is None else np.array(keys_out, dtype=np.uint32)
    vo = np.zeros(len(keys), dtype=np.uint32) if vals_out is None else np.array(vals_out, dtype=np.uint32)
    order = np.argsort(effective_key(keys[:m], lowmask, inv_from), kind="stable")
    ko[:m], vo[:m] = keys[:m][order], vals[:m][order]
    return ko, vo


def launch_sort_params(seg_keys, invalid, batch, n_sets):
    """(end_bit, lowmask, inv_from) msm_launch gives the sort in the FIXED layout (engine comments at launch_reserve): the bits
    of the invalid key; for several vectors over one query with seg_keys a power of two, the bucket bits alone plus one value
    for the invalid key -- when that saves an 8-bit pass"""
    end_bit = max(1, int(invalid).bit_length())
    if batch > 1 and n_sets == 1 and seg_keys & (seg_keys - 1) == 0:
        eb = int(seg_keys).bit_length()
        if -(-eb // 8) < -(-end_bit // 8):
            return eb, seg_keys - 1, invalid
    return end_bit, 0xFFFFFFFF, 0xFFFFFFFF


def edge_scalars(curve, c, unreduced=False):
    """the scalars at which a digit recoding goes wrong: window boundaries, the fold point (r +- 1) / 2, the top of the range,
    and -- unreduced -- values from r up to 2^256 - 1"""
    r, bits = synth.FR_MODULUS[curve], synth.FR_BITS[curve]
    B, W = 1 << (c - 1), windows(bits, c)
    e = [0, 1, 2, B - 1, B, B + 1, (1 << c) - 1, 1 << c, (B << c) | B]
    e += [(1 << (c * j)) - 1 for j in sorted({1, 2, 3, W // 2, W - 1})]  # every window below j all ones
    e += [(r - 1) // 2 - 1, (r - 1) // 2, (r + 1) // 2, (r + 1) // 2 + 1, r - 2, r - 1, r - B, (1 << (bits - 1)) - 1, (1 << (bits - 1)) + 1]
    e = [x % r for x in e]
    if unreduced:  # 5 r + 3 where 256 bits hold it (BN254: 2^256 = 5.29 r); BLS12-381 (2^256 = 2.2 r) takes 2 r + 3 in its place
        e += [r, r + 1, 2 * r - 1, 5 * r + 3 if 5 * r + 3 < 1 << 256 else 2 * r + 3, (1 << 256) - 1]
    return e
