"""GPU parity of the MSM on inputs with few distinct points: doublings and cancellations in every tail addition.
Every other MSM test draws its bases with H.random_points, so bucket sums and partials are distinct random points and the
tail kernels behind the accumulate stage (merge_partials, tile_reduce, serial_reduce, reduce_level1, fold_windows, the host
fold, the workgroup fold of accumulate_single; XYZZ::add, CoopAdd with two exchange areas and -- BLS12-381 G2 -- with one) only
ever add general pairs or infinity. The inputs of tests/msm_degenerate_inputs.py dictate the bucket contents (ones, alternating,
tile-alternating, lane-mixed, zero total, a front pattern for serial_reduce), repeat one point through the merge levels and
through accumulate_single, and run uniform scalars over an eight-point base cycle; what the additions meet is counted by the
plain-integer model in tests/test_msm_tail_ref.py. Expected, bit-exact: [sum k_i m_i mod r] G by one scalar multiplication of
the oracle, zeros for a zero sum; that the oracle's own MSM (algo 0) gives the same on every one of these inputs needs no GPU
and is asserted in tests/test_msm_tail_ref.py.
Each case runs through multi_scalar_mul, launch().finish(), launch(sparse=True) and -- tables -- result_to_device + xyzz_sum.
With tables all of them see the dictated buckets; with plain bases launch() and launch(sparse=True) do (window_bits = c), while
multi_scalar_mul takes no window width and runs the same few points at the library's own. All this on the shipped library at
the defaults and in child processes (knobs are read once per process; the diagnosis twin) with every tail forced plain and forced
cooperative, with front levels (MANTA_RED_MIN=128, once inline), and the merge inputs with chunk lengths 1, 2, 3."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import msm_degenerate_inputs as D
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CASES = [(0, 1), (1, 1), (0, 2), (1, 2)]

_CHILD = r'''
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import msm_degenerate_inputs as D
from manta_rs_amd import api as gpu
gpu.init(0)
for line in D.run(gpu, {curve}, {group}, np.load({data!r})):
    print(line)
print("degenerate done", os.path.basename(gpu.LIB_PATH))
'''


def _all_ok(lines, names, tag):
    bad = [ln for ln in lines if not ln.endswith(" ok")]
    assert not bad, "%s: %s" % (tag, bad[:12])
    assert [ln.split()[0] for ln in lines] == [str(n) for n in names], tag


def _children(curve, group, kind, knob_sets, tmp_path):
    """one child per knob set, all alive at once (at most 8), each on the diagnosis twin; one line per case"""
    assert len(knob_sets) <= 8
    cases, data = D.inputs(curve, group, kind)
    path = str(tmp_path / "degenerate.npz")
    np.savez(path, **data)
    code = _CHILD.format(root=ROOT, curve=curve, group=group, data=path)
    procs = {}
    for name, knobs in knob_sets.items():
        out, err = open(str(tmp_path / (name + ".out")), "w+"), open(str(tmp_path / (name + ".err")), "w+")
        procs[name] = (subprocess.Popen([sys.executable, "-c", code], env=H.knob_env(knobs), stdout=out, stderr=err, text=True), out, err)
    results = {}
    for name, (p, out, err) in procs.items():
        try:
            rc = p.wait(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            rc = "timeout"
        out.seek(0), err.seek(0)
        results[name] = (rc, out.read(), err.read())
        out.close(), err.close()
    for name, (rc, text, errors) in results.items():
        lines = text.splitlines()
        assert rc == 0 and lines and lines[-1].startswith("degenerate done"), "%s: exit %s: %s" % (name, rc, text[-2000:] + errors[-2000:])
        assert lines[-1].split()[-1] == "libmantagpu_diag.so", name  # the shipped library has the defaults compiled in
        _all_ok(lines[:-1], data["names"], name)


@pytest.mark.parametrize("curve,group", CASES)
def test_degenerate_tails_at_the_defaults(gpu, curve, group):
    """the dictated-bucket vectors at c = 7 / 9 / 13 / 14 (tables and plain bases, one entry per bucket and copies of +-G) and the
    small-multiple inputs, in-process on the library that was loaded"""
    cases, data = D.inputs(curve, group, "tails")
    assert any(not data["want%d" % i].any() for i in range(len(cases)))  # zero totals: all-zero limbs
    _all_ok(D.run(gpu, curve, group, data), data["names"], "defaults")


@pytest.mark.parametrize("curve,group", CASES)
def test_degenerate_tails_forced_plain_cooperative_and_with_front_levels(gpu, tmp_path, curve, group):
    _children(curve, group, "tails", D.TAIL_KNOBS, tmp_path)


@pytest.mark.parametrize("curve,group", CASES)
def test_one_point_inputs_through_merge_and_accumulate_single(gpu, tmp_path, curve, group):
    """all bases G (or G, -G alternating): equal partials through the serial fold and the segmented scan of merge_partials for
    chunk lengths 1, 2, 3, plain and cooperative; one key on full tables: the workgroup fold of accumulate_single (G2 too)"""
    cases, data = D.inputs(curve, group, "merge")
    _all_ok(D.run(gpu, curve, group, data), data["names"], "defaults")
    _children(curve, group, "merge", D.MERGE_KNOBS, tmp_path)


_PROVE_CHILD = r'''
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import msm_degenerate_inputs as D
from manta_rs_amd import api as gpu
gpu.init(0)
c, pk = D.degenerate_key({curve})
ctx_proofs = D.prove_all(gpu, {curve}, c, pk)
for p in ctx_proofs:
    print("PROOF", p.hex())
'''


@pytest.mark.parametrize("curve", [0, 1])
def test_proofs_under_a_key_of_eight_distinct_points(gpu, curve):
    """A proving key whose every query cycles through G, G, -G, 2G, G, infinity, -G, G (G1 and G2): single proofs and a batch of
    three give the oracle's bytes (its MSM algo 0) -- at the default table budget (full tables: plain sums) and, in a child,
    with MANTA_FULL_TABLE_GB=0 (bucket tables). The one route to the batched-pass and full-table MSM configurations with
    exceptional pairs."""
    c, pk = D.degenerate_key(curve)
    rs = H.rand_fr_mont(curve, 6, seed=32)
    want = [O.groth16_prove(c, pk, rs[i], rs[3 + i], msm_algo=0) for i in range(3)] * 2
    got = D.prove_all(gpu, curve, c, pk)
    assert got == want, H.proof_diff(got, want)
    env = dict(os.environ, MANTA_FULL_TABLE_GB="0")
    out = subprocess.run([sys.executable, "-c", _PROVE_CHILD.format(root=ROOT, curve=curve)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = [bytes.fromhex(ln.split()[1]) for ln in out.stdout.splitlines() if ln.startswith("PROOF")]
    assert got == want, H.proof_diff(got, want, {"MANTA_FULL_TABLE_GB": "0"})
