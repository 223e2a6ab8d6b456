"""CPU tests of tests/msm_frontend_ref.py, the reference of tests/test_gpu_msm_frontend.py: identities that a digit recoding
and a pair layout must satisfy whoever wrote them, so that the reference cannot be wrong the way the kernel is."""
import numpy as np
import pytest

import msm_frontend_ref as R
from manta_rs_amd import synth

CS = {0: (2, 5, 8, 13, 16, 17), 1: (2, 5, 8, 13, 15, 16, 17)}  # the window widths of the GPU tests
CASES = [(curve, c) for curve in (0, 1) for c in CS[curve]]


@pytest.mark.parametrize("curve,c", CASES)
def test_digits_recompose_to_the_scalar_with_bounded_magnitudes(curve, c):
    r, bits = synth.FR_MODULUS[curve], synth.FR_BITS[curve]
    B, W = 1 << (c - 1), R.windows(bits, c)
    rng = synth.XorShift(100 * curve + c)
    ks = R.edge_scalars(curve, c, unreduced=True) + [rng.field(r) for _ in range(200)]
    ks += [int(x) for x in synth.limbs_to_ints(synth.msm_scalars(curve, 64, "W", seed=c))]
    for k in ks:
        ds = R.digits(k, r, bits, c)
        assert (R.digits_value(ds, c) - k) % r == 0, hex(k)
        assert all(1 <= m <= B for _, m, _ in ds), hex(k)  # no zero digit is listed, no magnitude exceeds B
        ws = [w for w, _, _ in ds]
        assert ws == sorted(set(ws)) and (not ws or ws[-1] <= W - 1), hex(k)  # one digit per window, none beyond W - 1
        # the folded scalar is below 2^(bits - 1): as an integer the digits are min(k, r - k) up to the common sign
        assert abs(R.digits_value(ds, c)) == min(k % r, r - k % r), hex(k)


def test_top_window_is_full_where_c_divides_the_scalar_bits():
    """BLS12-381, 255 = 15 x 17: W = 17 (c = 15) and W = 15 (c = 17) leave no spare bit above the folded scalar, so the largest
    one, (r - 1) / 2, must still end inside window W - 1"""
    r, bits = synth.FR_MODULUS[1], synth.FR_BITS[1]
    for c in (15, 17):
        assert bits % c == 0 and R.windows(bits, c) == bits // c
        for k in ((r - 1) // 2, (r + 1) // 2, (1 << (bits - 1)) - 1):
            assert R.digits(k, r, bits, c)[-1][0] <= bits // c - 1


@pytest.mark.parametrize("table_mode", [0, 1, 2])
def test_pairs_layouts_agree_and_zero_digits_yield_no_pair(table_mode):
    curve, c, n = 0, 5, 7
    r, bits = synth.FR_MODULUS[curve], synth.FR_BITS[curve]
    vec = [0, 1, r - 1, 0, 1 << c, (r + 1) // 2, 0]
    p = R.Pairs(curve, [vec, vec[::-1]], c, n, table_mode)
    nonzero = sum(len(R.digits(k, r, bits, c)) for k in vec)
    assert len(p.key) == 2 * nonzero and p.compact().shape == (2 * nonzero, 2)
    keys, vals = p.fixed()
    assert keys.shape == (2 * p.W * n,) and (keys == p.invalid).sum() == 2 * p.W * n - 2 * nonzero
    assert not vals[keys == p.invalid].any() and (keys <= p.invalid).all()
    live = keys != p.invalid
    assert (R.sorted_pairs(keys[live], vals[live]) == p.compact()).all()
    # the scalar 0 (lanes 0, 3, 6 of vector 0) leaves every window of its lane invalid
    for i in (0, 3, 6):
        assert (keys[:p.W * n].reshape(p.W, n)[:, i] == p.invalid).all()
    # every key names its vector: vector q's keys lie in [q seg_keys, (q + 1) seg_keys)
    assert (keys[:p.W * n][live[:p.W * n]] < p.seg_keys).all() and (keys[p.W * n:][live[p.W * n:]] >= p.seg_keys).all()
    # the pairs rebuild each scalar: sum over the pairs of a lane of +-(magnitude) 2^(c window) = k (mod r)
    B = p.B
    acc = [0] * n
    for key, val in zip(keys[:p.W * n][live[:p.W * n]].tolist(), vals[:p.W * n][live[:p.W * n]].tolist()):
        sign, idx = -1 if val >> 31 else 1, val & 0x7FFFFFFF
        if table_mode == 0:
            i, w, m = idx, key // B, key % B + 1
        elif table_mode == 1:
            i, w, m = idx % n, idx // n, key + 1
        else:
            i, w, m = (idx // B) % n, (idx // B) // n, idx % B + 1
        acc[i] += sign * m << (c * w)
    assert [a % r for a in acc] == [k % r for k in vec]


def test_pairs_follow_map_zip_and_queries():
    curve, c = 1, 8
    r, bits = synth.FR_MODULUS[curve], synth.FR_BITS[curve]
    vec = [3, 0, r - 5, 77, 1 << 200]                   # set_len 6, 5 scalars: entry 5 of every query has none
    mp = [11, 2, 5, 6, 0, 16]                           # stored base i <- original entry map[i]; queries 1, 0, 0, 1, 0, 2
    p = R.Pairs(curve, [vec], c, 6, 0, map=mp, n_sets=3, set_len=6)
    assert p.invalid == 3 * p.seg_keys
    for i, src in enumerate(mp):
        k = vec[src % 6] if src % 6 < len(vec) else 0
        mine = p.i == i
        assert mine.sum() == len(R.digits(k, r, bits, c))
        assert (p.key[mine] // p.seg_keys == src // 6).all() and ((p.val[mine] & 0x7FFFFFFF) == i).all()


def test_sort_reference_is_stable_and_masks():
    keys = np.array([5, 1, 9, 1, 5, 8, 1], dtype=np.uint32)
    vals = np.arange(7, dtype=np.uint32)
    k, v = R.sort_pairs(keys, vals)
    assert k.tolist() == [1, 1, 1, 5, 5, 8, 9] and v.tolist() == [1, 3, 6, 0, 4, 5, 2]
    # by the low two bits, keys from 8 up last: 5 -> 1, 1 -> 1, 9 -> last, 8 -> last
    k, v = R.sort_pairs(keys, vals, lowmask=3, inv_from=8)
    assert k.tolist() == [5, 1, 1, 5, 1, 9, 8] and v.tolist() == [0, 1, 3, 4, 6, 2, 5]
    # a count: the tail keeps the caller's values
    k, v = R.sort_pairs(keys, vals, count=3, keys_out=np.full(7, 99), vals_out=np.full(7, 98))
    assert k.tolist() == [1, 5, 9, 99, 99, 99, 99] and v.tolist() == [1, 0, 2, 98, 98, 98, 98]
    # the largest 32-bit key is the last one of a full-key sort
    k, _ = R.sort_pairs(np.array([0xFFFFFFFF, 0, 7], dtype=np.uint32), vals[:3])
    assert k.tolist() == [0, 7, 0xFFFFFFFF]


def test_launch_sort_params():
    full = 0xFFFFFFFF
    assert R.launch_sort_params(1 << 13, 32 << 13, 32, 1) == (14, (1 << 13) - 1, 32 << 13)  # 19 bits -> 14: a pass saved
    assert R.launch_sort_params(1 << 13, 3 << 13, 3, 1) == (15, full, full)                 # 15 bits -> 14: no pass saved
    assert R.launch_sort_params(128, 3 * 128, 3, 1) == (8, 127, 384)                        # 9 bits -> 8
    assert R.launch_sort_params(128, 128, 1, 1) == (8, full, full)                          # one vector: the key itself
    assert R.launch_sort_params(128, 6 * 128, 3, 2) == (10, full, full)                     # several queries
    assert R.launch_sort_params(3 * 16, 9 * 16, 3, 1) == (8, full, full)                    # not a power of two
