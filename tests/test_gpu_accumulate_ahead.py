"""GPU parity of the rotated accumulate loop of BLS12-381 G1 (msm_accumulate.h accumulate_chunks) where its fetches run ahead
of the addition: the base record of entry j + 1 and the pair of entry j + 2 are requested while addition j is under way. Bit-exact
against the CPU oracle through the diagnosis library with 1, 2, 3 and 5 entries per lane: the pair fetch two entries ahead then
lands on a chunk's last entry, one before it and one past it in every lane. n = 4 096 at window 8 (128 buckets per window: runs
of several entries that cross lane boundaries)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
from manta_rs_amd import synth
from test_gpu_accumulate_loop import exceptional_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CURVE, N, WINDOW = 1, 4096, 8
SHORTER = [N - 2, N - 3]  # pair counts (a multiple of n) that leave the last lane of L = 3 and L = 5 one or two entries
CHUNK_LENGTHS = [1, 2, 3, 5]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """inputs and oracle results, computed once and shared by the four children"""
    pts = H.random_points(CURVE, 1, N, seed=900)
    pts[9] = 0
    d = {"pts": pts}
    for dist in ("U", "W"):
        sc = synth.msm_scalars(CURVE, N, dist, seed=910 + ord(dist))
        d["sc" + dist] = sc
        d["want" + dist] = O.msm(CURVE, 1, pts, sc, algo=1)
    for m in SHORTER:
        d["wantU%d" % m] = O.msm(CURVE, 1, pts[:m], d["scU"][:m], algo=1)
    # doubling, cancellation and infinity groups; 120 groups: every scalar is one signed window-8 digit (|digit| < 128)
    d["epts"], d["esc"] = exceptional_case(CURVE, n_groups=120)
    d["ewant"] = O.msm(CURVE, 1, d["epts"], d["esc"], algo=1)
    path = str(tmp_path_factory.mktemp("accahead") / "cases.npz")
    np.savez(path, **d)
    return path


_CHILD = r'''
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
from manta_rs_amd import api as gpu
gpu.init(0)
d = np.load({data!r})
def msm(pts, sc, **kw):
    b = gpu.Bases({curve}, 1, pts)
    got = gpu.VariableBaseMSM.launch(b, gpu.DeviceBuffer.from_numpy(sc), len(sc), window_bits={window}, **kw).finish()
    b.close()
    return got
assert (msm(d["pts"], d["scU"]) == d["wantU"]).all(), "uniform"
for m in {shorter!r}:
    assert (msm(d["pts"][:m], d["scU"][:m]) == d["wantU%d" % m]).all(), ("uniform", m)
for dist in ("U", "W"):  # the compacted stream: lanes end on an `invalid` key, the pair count is only known on the device
    assert (msm(d["pts"], d["sc" + dist], sparse=True) == d["want" + dist]).all(), ("sparse", dist)
assert (msm(d["epts"], d["esc"]) == d["ewant"]).all(), "exceptional"
assert (msm(d["epts"], d["esc"], sparse=True) == d["ewant"]).all(), "exceptional, sparse"
print("accumulate ahead ok", os.path.basename(gpu.LIB_PATH))
'''


@pytest.fixture(scope="module")
def chunk_children(cases):
    """one child per chunk length (MANTA_MSM_L is read once per process by the diagnosis twin), all four started together"""
    code = _CHILD.format(root=ROOT, data=cases, curve=CURVE, window=WINDOW, shorter=SHORTER)
    procs = {L: subprocess.Popen([sys.executable, "-c", code], env=H.knob_env({"MANTA_MSM_L": str(L)}), stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True) for L in CHUNK_LENGTHS}
    out = {}
    for L, p in procs.items():
        so, se = p.communicate(timeout=600)
        out[L] = (p.returncode, so, se)
    return out


@pytest.mark.parametrize("L", CHUNK_LENGTHS)
def test_entries_per_lane(gpu, chunk_children, L):
    """uniform scalars at n, n - 2 and n - 3 (pair counts that are no multiple of L = 3, 5: a last lane of one or two entries),
    uniform and witness-like scalars through the compacted stream (lanes that end on an `invalid` key at entries j + 1 and
    j + 2), and the doubling / cancellation / infinity groups of test_gpu_accumulate_loop.exceptional_case"""
    rc, so, se = chunk_children[L]
    assert rc == 0 and "accumulate ahead ok libmantagpu_diag.so" in so, so[-2000:] + se[-2000:]
