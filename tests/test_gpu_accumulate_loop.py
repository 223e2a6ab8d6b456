"""GPU parity of the bucket-accumulate loop (msm_accumulate.h: accumulate_chunks / accumulate_single) against the CPU oracle,
bit-exact through the C ABI: chunk lengths shorter than a four-entry block of the pair stream, with heads and tails of every
length 0-3 and a last lane that ends inside a block, lanes that end on an `invalid` key, runs longer and shorter than a chunk,
and the exceptional additions at every position of a block and of a chunk."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
from manta_rs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

N = 4096
CHUNK_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9]


def exceptional_case(curve, n_groups=240, seed=7):
    """Scalars that are one small digit each (window >= 9 bits): bucket g holds the entries of group g in index order. The groups
    cycle through  P P Q (doubling at the start of a run),  P -P Q (cancellation to infinity, then a further addition; -P is the
    scalar r - g on the same base: the digit kernel recodes k > r / 2 as -(r - k), msm_digits.h) and  inf P inf Q,  each followed
    by 0-3 more points, so the group sizes cycle through 3-7 and the runs -- and with them the repeated entries -- start at every
    residue of the pair index modulo 4 (block positions 0 and 3 among them) and at every offset of a lane's chunk. Whether two
    equal summands meet as a doubling or inside a later merge depends on the order the sort leaves inside a bucket, which the
    test does not fix: the result is the same group element either way, and that is what is compared."""
    r = synth.FR_MODULUS[curve]
    pool = H.random_points(curve, 1, 3 * n_groups, seed=seed)
    pts, ks = [], []
    for g in range(1, n_groups + 1):
        p, q = pool[3 * g - 3], pool[3 * g - 2]
        kind = g % 3
        if kind == 0:
            grp = [(p, g), (p, g), (q, g)]
        elif kind == 1:
            grp = [(p, g), (p, r - g), (q, g)]
        else:
            grp = [(np.zeros_like(p), g), (p, g), (np.zeros_like(p), g), (q, g)]
        grp += [(pool[(3 * g + 5 * e) % len(pool)], g) for e in range(g % 4)]
        for pt, k in grp:
            pts.append(pt)
            ks.append(k)
    return np.stack(pts), synth.ints_to_limbs(ks, 4)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """inputs and oracle results shared by the chunk-length children and the in-process tests (computed once)"""
    d = {}
    for curve in (0, 1):
        pts = H.random_points(curve, 1, N, seed=300 + curve)
        pts[9] = 0
        d["pts%d" % curve] = pts
        for dist in ("U", "W"):
            sc = synth.msm_scalars(curve, N, dist, seed=310 + curve)
            d["sc%s%d" % (dist, curve)] = sc
            d["want%s%d" % (dist, curve)] = O.msm(curve, 1, pts, sc, algo=1)
        epts, esc = exceptional_case(curve)
        d["epts%d" % curve], d["esc%d" % curve] = epts, esc
        d["ewant%d" % curve] = O.msm(curve, 1, epts, esc, algo=1)
    path = str(tmp_path_factory.mktemp("accloop") / "cases.npz")
    np.savez(path, **d)
    return path, d


_CHILD = r'''
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
from manta_rs_amd import api as gpu
gpu.init(0)
d = np.load({data!r})
for curve in (0, 1):
    for pre in (0, 17):
        b = gpu.Bases(curve, 1, d["pts%d" % curve], precompute_window_bits=pre)
        got = gpu.VariableBaseMSM.multi_scalar_mul(b, d["scU%d" % curve])
        assert (got == d["wantU%d" % curve]).all(), ("uniform", curve, pre)
        for dist in ("U", "W"):  # the compacted stream: the pair count is only known on the device
            sc = gpu.DeviceBuffer.from_numpy(d["sc%s%d" % (dist, curve)])
            got = gpu.VariableBaseMSM.launch(b, sc, {n}, sparse=True).finish()
            assert (got == d["want%s%d" % (dist, curve)]).all(), ("sparse", dist, curve, pre)
        b.close()
    b = gpu.Bases(curve, 1, d["epts%d" % curve], precompute_window_bits=9)
    assert (gpu.VariableBaseMSM.multi_scalar_mul(b, d["esc%d" % curve]) == d["ewant%d" % curve]).all(), ("exceptional", curve)
    b.close()
print("accumulate loop ok", os.path.basename(gpu.LIB_PATH))
'''


@pytest.fixture(scope="module")
def chunk_children(cases):
    """one child per chunk length (MANTA_MSM_L is read once per process by the diagnosis twin), all eight started together"""
    path, _ = cases
    code = _CHILD.format(root=ROOT, data=path, n=N)
    procs = {L: subprocess.Popen([sys.executable, "-c", code], env=H.knob_env({"MANTA_MSM_L": str(L)}), stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True) for L in CHUNK_LENGTHS}
    out = {}
    for L, p in procs.items():
        so, se = p.communicate(timeout=600)
        out[L] = (p.returncode, so, se)
    return out


@pytest.mark.parametrize("L", CHUNK_LENGTHS)
def test_chunk_lengths(gpu, chunk_children, L):
    """BLS12-381 and BN254 G1, n = 4 096, plain bases and c = 17 tables, uniform and witness-like scalars (plain and compacted
    pair streams) and the exceptional additions, with MANTA_MSM_L entries per lane: chunks shorter than a block, heads and tails
    of every length 0-3 (L = 1, 2, 3, 5, 7, 9 put a chunk's start on every residue modulo 4), whole blocks (4, 8), a last lane
    that ends inside its chunk."""
    rc, so, se = chunk_children[L]
    assert rc == 0 and "accumulate loop ok libmantagpu_diag.so" in so, so[-2000:] + se[-2000:]


@pytest.mark.parametrize("curve", [0, 1])
def test_sparse_scalars(gpu, cases, curve):
    """witness-like scalars through the compacted stream at the plan's own chunk length (the `count` / `adapt` path: the pair
    count is no multiple of anything and most lanes of the round are empty)"""
    _, d = cases
    for pre in (0, 17):
        b = gpu.Bases(curve, 1, d["pts%d" % curve], precompute_window_bits=pre)
        got = gpu.VariableBaseMSM.launch(b, gpu.DeviceBuffer.from_numpy(d["scW%d" % curve]), N, sparse=True).finish()
        assert (got == d["wantW%d" % curve]).all(), pre


@pytest.mark.parametrize("curve", [0, 1])
def test_few_distinct_scalars(gpu, curve):
    """three distinct scalars: every run is far longer than a chunk, so nearly every lane leaves its loop with `first` still set
    and its second partial at infinity"""
    n = 2048
    pts = H.random_points(curve, 1, n, seed=41 + curve)
    three = synth.msm_scalars(curve, 3, "U", seed=42)
    sc = three[np.arange(n) % 3]
    want = O.msm(curve, 1, pts, sc, algo=1)
    for pre in (0, 13):
        assert (gpu.VariableBaseMSM.multi_scalar_mul(gpu.Bases(curve, 1, pts, precompute_window_bits=pre), sc) == want).all(), pre


@pytest.mark.parametrize("curve", [0, 1])
def test_all_distinct_digits(gpu, curve):
    """scalars 1 .. n below one 13-bit window: every entry of the stream is a run of its own (a boundary in every iteration)"""
    n = 2048
    pts = H.random_points(curve, 1, n, seed=51 + curve)
    sc = synth.ints_to_limbs(list(range(1, n + 1)), 4)
    want = O.msm(curve, 1, pts, sc, algo=1)
    assert (gpu.VariableBaseMSM.multi_scalar_mul(gpu.Bases(curve, 1, pts, precompute_window_bits=13), sc) == want).all()


@pytest.mark.parametrize("curve", [0, 1])
def test_exceptional_additions(gpu, cases, curve):
    """doubling, cancellation followed by a further addition and infinity bases (exceptional_case) at the plan's chunk length,
    plain bases and tables"""
    _, d = cases
    for pre in (0, 9):
        b = gpu.Bases(curve, 1, d["epts%d" % curve], precompute_window_bits=pre)
        assert (gpu.VariableBaseMSM.multi_scalar_mul(b, d["esc%d" % curve]) == d["ewant%d" % curve]).all(), pre


def test_bn254_g2(gpu):
    """over Fp2 the additions are calls and the loop is the straight one"""
    n = 1024
    pts = H.random_points(0, 2, n, seed=61)
    pts[3] = 0
    pts[40] = pts[41]
    sc = synth.msm_scalars(0, n, "U", seed=62)
    sc[40] = sc[41]
    assert (gpu.VariableBaseMSM.multi_scalar_mul(gpu.Bases(0, 2, pts), sc) == O.msm(0, 2, pts, sc, algo=1)).all()


@pytest.mark.parametrize("curve", [0, 1])
def test_single_key(gpu, curve):
    """full tables, one scalar vector: accumulate_single (every pair has key 0); repeated bases, infinity, P and -P"""
    n = 700
    r = synth.FR_MODULUS[curve]
    pts = H.random_points(curve, 1, n, seed=71 + curve)
    pts[3] = 0
    pts[40] = pts[41]
    ks = synth.limbs_to_ints(synth.msm_scalars(curve, n, "U", seed=72))
    ks[40], ks[41] = 5, r - 5
    ks[0] = ks[1] = 1
    pts[1] = pts[0]
    sc = synth.ints_to_limbs(ks, 4)
    want = O.msm(curve, 1, pts, sc, algo=1)
    b = gpu.Bases(curve, 1, pts, precompute_window_bits=-6)
    assert (gpu.VariableBaseMSM.multi_scalar_mul(b, sc) == want).all()
    assert (gpu.VariableBaseMSM.launch(b, gpu.DeviceBuffer.from_numpy(sc), n, sparse=True).finish() == want).all()
