"""GPU parity of the MSM's fused front end (msm_digits.h digits_hist / digits_scatter over sort_scatter.h; chosen by
msm_dense_front_applies for a stand-alone dense MSM on window tables of at most 16 windows): every digit is a pair, a zero digit
points at the infinity record behind the last table, and the first radix pass runs over tiles of 256 scalars whose pairs are
computed, never stored.

End to end: G1 MSMs of both curves on tables of 17- and 16-bit windows (W = 15 and 16) at the tile edges n = 1, 63, 255, 256,
257, 4 097, equal to the CPU oracle and to the library with MANTA_DENSE_FRONT=0 (the diagnosis twin in a child process: knobs
are read once per process), over uniform scalars, all zeros, one scalar for every base, and the scalars at which the recoding
can go wrong: 0, 1, r - 1, the fold boundary (r -+ 1) / 2, values from r up, every window at B or B + 1 (a carry into the next
window), k and r - k on the same base. One case at c = 15 (W = 17) takes the digit kernel and the whole sort, as before.

Stage level, through `mg_msm_dense_front`: the sorted pairs against the plain-integer reference of tests/msm_frontend_ref.py
with the zero digits added as (0, infinity index) -- as a multiset, the order inside a run being unspecified."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import msm_frontend_ref as R
import oracle_lib as O
from manta_rs_amd import synth
from test_gpu_msm_frontend import KEY_SENTINEL, VAL_SENTINEL, limbs, scalar_vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CURVES = (0, 1)
TABLE_BITS = (17, 16)  # W = 15 and 16 on both curves
NS = (1, 63, 255, 256, 257, 4097)
N_MAX = max(NS)
TWIN, TWIN_AT = 10, 11  # bases 10 and 11 are the same point (n >= 63): k on one, r - k on the other


def special_scalars(curve):
    """integers at which the recoding can go wrong, for both table widths. Unreduced ones stay below 2^BITS: the oracle, like
    arkworks' multi_scalar_mul, walks the BITS bits of the scalar field (its BLS12-381 result for 2^255 + 5 is not that of the
    scalar mod r), while the library reduces mod r; up to 2^BITS - 1 both stand for the same group element."""
    r, bits = synth.FR_MODULUS[curve], synth.FR_BITS[curve]
    e = [0, 1, r - 1, (r - 1) // 2, (r + 1) // 2, r, r + 1, r + (1 << 64) + 3, (1 << bits) - 1]
    for c in TABLE_BITS:
        B, W = 1 << (c - 1), R.windows(bits, c)
        at_b = sum(B << (c * w) for w in range(W))                 # every window at B: the largest digit, no carry
        above = sum((B + 1) << (c * w) for w in range(W))          # every window at B + 1: every window carries, the top one too
        mixed = sum((B + (w & 1)) << (c * w) for w in range(W))
        for k in (at_b, above, mixed):
            e += [k, k % r, (r - k) % r, k >> c]                   # as given (folded or not as r decides), negated, top window clear
    assert any(k >= r for k in e)
    return [k for k in e if k < 1 << bits]


def scalar_sets(curve, n):
    """{name: n integers}"""
    r = synth.FR_MODULUS[curve]
    uniform = [int(x) for x in synth.limbs_to_ints(synth.msm_scalars(curve, n, "U", seed=4100 + 7 * curve + n))]
    sp = special_scalars(curve)
    if n == 1:  # one lane: every special scalar in turn
        return dict({"special%d" % t: [k] for t, k in enumerate(sp)}, uniform=uniform)
    edges = list(uniform)
    for t, k in enumerate(sp[:n - 12]):
        edges[12 + t] = k
    edges[TWIN], edges[TWIN_AT] = uniform[0], r - uniform[0]
    return {"uniform": uniform, "zeros": [0] * n, "repeated": [uniform[1]] * n, "edges": edges}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """per curve the points, every scalar vector and its oracle result, computed once; also as a file for the child"""
    d = {}
    for curve in CURVES:
        pts = H.random_points(curve, 1, N_MAX, seed=4000 + curve)
        pts[5] = 0  # a base at infinity
        pts[TWIN_AT] = pts[TWIN]
        d["pts%d" % curve] = pts
        for n in NS:
            for name, vec in scalar_sets(curve, n).items():
                sc = synth.ints_to_limbs(vec, 4)
                d["sc_%d_%d_%s" % (curve, n, name)] = sc
                d["want_%d_%d_%s" % (curve, n, name)] = O.msm(curve, 1, pts[:n], sc, algo=1)
    path = str(tmp_path_factory.mktemp("densefront") / "cases.npz")
    np.savez(path, **d)
    return d, path


_CHILD = r'''
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
from manta_rs_amd import api as gpu
gpu.init(0)
d = np.load({data!r})
out = {{}}
for curve in {curves!r}:
    for pre in {pres!r}:
        for n in {ns!r}:
            b = gpu.Bases(curve, 1, d["pts%d" % curve][:n], precompute_window_bits=pre)
            for key in d.files:
                if key.startswith("sc_%d_%d_" % (curve, n)):
                    out["got_%d_%s" % (pre, key[3:])] = gpu.VariableBaseMSM.multi_scalar_mul(b, d[key])
            b.close()
np.savez({out!r}, **out)
print("dense front off ok", os.path.basename(gpu.LIB_PATH))
'''


@pytest.fixture(scope="module")
def compacting_path(cases, tmp_path_factory):
    """every case through the library with MANTA_DENSE_FRONT=0: the compacting digit kernel and the whole sort"""
    _, path = cases
    out = str(tmp_path_factory.mktemp("densefront_off") / "got.npz")
    code = _CHILD.format(root=ROOT, data=path, curves=CURVES, pres=TABLE_BITS, ns=NS, out=out)
    p = subprocess.run([sys.executable, "-c", code], env=H.knob_env({"MANTA_DENSE_FRONT": "0"}), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "dense front off ok libmantagpu_diag.so" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    return np.load(out)


@pytest.mark.parametrize("pre", TABLE_BITS)
@pytest.mark.parametrize("curve", CURVES)
def test_dense_msm_equals_the_oracle_and_the_compacting_path(gpu, cases, compacting_path, curve, pre):
    d, _ = cases
    W = R.windows(synth.FR_BITS[curve], pre)
    assert W == 32 - pre and gpu.msm_dense_front_applies(1, 1, W, 1, False)
    for n in NS:
        b = gpu.Bases(curve, 1, d["pts%d" % curve][:n], precompute_window_bits=pre)
        assert b.device_bytes() % (W * n + 1) == 0, "no infinity record behind the last table"
        for key in d:
            if key.startswith("sc_%d_%d_" % (curve, n)):
                got = gpu.VariableBaseMSM.multi_scalar_mul(b, d[key])
                tag = "curve %d c %d n %d %s" % (curve, pre, n, key)
                assert (got == d["want" + key[2:]]).all(), tag + ": differs from the oracle"
                assert (got == compacting_path["got_%d_%s" % (pre, key[3:])]).all(), tag + ": differs from MANTA_DENSE_FRONT=0"
        b.close()


def test_seventeen_windows_take_the_digit_kernel_and_the_sort(gpu, cases):
    """c = 15 on BLS12-381: W = 17 items do not fit a lane of the first radix pass -- the launch is not dense, the fused entry point
    refuses the shape, and the result is the oracle's as before"""
    d, _ = cases
    curve, pre, n = 1, 15, 257
    assert R.windows(synth.FR_BITS[curve], pre) == 17 and not gpu.msm_dense_front_applies(1, 1, 17, 1, False)
    with pytest.raises(gpu.MantaGpuError):
        gpu.msm_dense_front(curve, d["sc_1_257_uniform"], pre, n)
    b = gpu.Bases(curve, 1, d["pts1"][:n], precompute_window_bits=pre)
    for name in ("uniform", "edges", "zeros"):
        assert (gpu.VariableBaseMSM.multi_scalar_mul(b, d["sc_1_257_" + name]) == d["want_1_257_" + name]).all(), name
    b.close()


# ------------------------------------------------------------------------------------------------------------ stage level
def check_stage(gpu, curve, c, n, vec, mont, **kw):
    """the sorted pairs of ALL digits: non-decreasing keys, every run contiguous, and as a multiset the reference's pairs plus
    (0, infinity index) for every zero digit"""
    p = R.Pairs(curve, [vec], c, n, table_mode=1, **kw)
    size = p.W * n
    got = gpu.msm_dense_front(curve, limbs(curve, [vec], mont)[0], c, n, mont=mont, keys=np.full(size, KEY_SENTINEL, dtype=np.uint32),
                              vals=np.full(size, VAL_SENTINEL, dtype=np.uint32), **kw)
    tag = "curve %d c %d n %d mont %d %r" % (curve, c, n, mont, sorted(kw))
    assert (got["W"], got["B"], got["seg_keys"], got["inf_index"]) == (p.W, p.B, p.seg_keys, p.W * n), tag
    keys, vals = got["keys"], got["vals"]
    assert (np.diff(keys.astype(np.int64)) >= 0).all(), tag + ": keys not sorted"
    assert 1 + int((np.diff(keys.astype(np.int64)) != 0).sum()) == len(np.unique(keys)), tag + ": a run of equal keys is split"
    zeros = size - len(p.key)
    want = R.sorted_pairs(np.concatenate([p.key, np.zeros(zeros, dtype=np.uint32)]),
                          np.concatenate([p.val, np.full(zeros, p.W * n, dtype=np.uint32)]))
    have = R.sorted_pairs(keys, vals)
    bad = np.flatnonzero((have != want).any(axis=1))
    assert not len(bad), "%s: %d pairs differ as sorted multisets; first: got %s, want %s" % (tag, len(bad), have[bad[0]], want[bad[0]])


@pytest.mark.parametrize("curve,c", [(curve, c) for curve in CURVES for c in TABLE_BITS])
def test_fused_front_end_pairs(gpu, curve, c):
    for n in NS:
        if n == 1:
            for k in R.edge_scalars(curve, c, unreduced=True):
                check_stage(gpu, curve, c, 1, [k], mont=False)
        for seed, mont in ((0, False), (1, True)):  # uniform / witness-like (many zero digits), edges mixed in
            check_stage(gpu, curve, c, n, scalar_vector(curve, c, n, 30 * n + seed), mont)
    check_stage(gpu, curve, c, 300, [0] * 300, mont=False)  # nothing but zero digits: one run of key 0


@pytest.mark.parametrize("curve", CURVES)
def test_fused_front_end_with_a_map_and_a_short_scalar_vector(gpu, curve):
    """stored base i takes scalar map[i], a shuffled strict subset of 400 entries; the entries beyond the vector have no scalar:
    all their digits are zero"""
    n_orig, n, c = 400, 300, 17
    mp = np.random.RandomState(21 + curve).permutation(n_orig)[:n].astype(np.uint32)
    check_stage(gpu, curve, c, n, scalar_vector(curve, c, 390, 5), mont=False, map=mp, set_len=n_orig)
    check_stage(gpu, curve, c, n, scalar_vector(curve, c, 290, 6), mont=True)
