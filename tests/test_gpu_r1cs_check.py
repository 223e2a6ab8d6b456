"""The R1CS satisfaction check on the GPU (mg_r1cs_check, mg_ctx_r1cs_check) against the plain-integer reference of
tests/r1cs_check_ref.py: the first unsatisfied row and the number of unsatisfied rows per assignment, through the stand-alone
form and the context form, on both curves. The shapes are the smallest at which the kernel can go wrong: 333 rows are one
whole workgroup of 256 lanes (four wavefronts of 64) and a partial one."""
import functools
import threading

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
import r1cs_check_ref as R
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu
CURVES = [0, 1]


@functools.lru_cache(maxsize=None)
def _key(curve, profile="sparse", shape=None):
    c = R.circuit(curve, profile) if shape is None else synth.make_circuit(curve, *shape, seed=7)
    return c, O.groth16_setup(c, H.toxic(curve, seed=19))


def context(gpu, curve, profile="sparse", shape=None):
    """a fresh context on the circuit, its matrices uploaded"""
    c, pk = _key(curve, profile, shape)
    ctx = gpu.ProvingContext(curve, pk)
    ctx.set_r1cs(gpu.R1CS.from_circuit(c))
    return c, pk, ctx


def both_forms(gpu, c, ctx, zs):
    """(first, counts) of the assignments through mg_r1cs_check, after checking that mg_ctx_r1cs_check says the same"""
    alone = gpu.r1cs_check(c.curve, c.A, c.B, c.C, c.m, c.V, zs)
    inside = ctx.check_assignments(zs)
    assert alone[0].tolist() == inside[0].tolist() and alone[1].tolist() == inside[1].tolist()
    return alone[0].tolist(), alone[1].tolist()


@pytest.mark.parametrize("profile", synth.PROFILES)
@pytest.mark.parametrize("curve", CURVES)
def test_single_rows(gpu, curve, profile):
    """one failing defining row at a time: first and last lane of a wavefront, first lane of the second wavefront, last lane of
    the first workgroup, first lane of the second one, last row of the partial workgroup"""
    c, _, ctx = context(gpu, curve, profile)
    assert both_forms(gpu, c, ctx, c.z) == ([-1], [0])
    for k in R.ROWS:
        z_int, z = R.corrupt_row(c, k)
        first, count = R.verdict(c, z_int)
        assert first == k                                     # (pinned on the CPU by test_r1cs_check_ref)
        assert both_forms(gpu, c, ctx, z) == ([first], [count]), k
    # the Python mirror of R1CS::is_satisfied / which_is_unsatisfied, on the compiler's own assignment
    good = gpu.R1CS.from_circuit(c)
    assert good.is_satisfied() and good.which_is_unsatisfied() is None
    bad = gpu.R1CS(curve, c.A, c.B, c.C, c.m, c.P, R.corrupt_row(c, 256)[1])
    assert not bad.is_satisfied() and bad.which_is_unsatisfied() == 256


@pytest.mark.parametrize("curve", CURVES)
def test_several_rows_in_different_wavefronts_and_workgroups(gpu, curve):
    """the minimum across several atomics and the summed count"""
    c, _, ctx = context(gpu, curve)
    z_int, z = R.corrupt(c, c.P + 300, c.P + 70, c.P + 5)
    bad = R.failing_rows(c, z_int)
    assert bad[0] == 5 and len({r // 64 for r in bad}) >= 3 and len({r // 256 for r in bad}) == 2
    assert both_forms(gpu, c, ctx, z) == ([5], [len(bad)])


@pytest.mark.parametrize("curve", CURVES)
def test_only_the_c_side_is_wrong(gpu, curve):
    c, _, ctx = context(gpu, curve)
    z_int, z = R.corrupt(c, R.c_only_variable(c))
    first, count = R.verdict(c, z_int)
    assert count >= 1
    assert both_forms(gpu, c, ctx, z) == ([first], [count])


@pytest.mark.parametrize("curve", CURVES)
def test_batch_of_five(gpu, curve):
    """verdicts [ok, row 64, ok, rows 0 and 332, row 255]: a stride or output-index mistake moves one of them"""
    c, _, ctx = context(gpu, curve)
    other = synth.reassign(c, 5)
    members = [(c.z_int, c.z), R.corrupt_row(c, 64), (other.z_int, other.z), R.corrupt(c, c.P, c.P + 332), R.corrupt_row(c, 255)]
    want = [R.verdict(c, z_int) for z_int, _ in members]
    assert [w[0] for w in want] == [-1, 64, -1, 0, 255] and R.failing_rows(c, members[3][0])[-1] == 332
    first, count = both_forms(gpu, c, ctx, R.stack([z for _, z in members]))
    assert list(zip(first, count)) == want
    for (_, z), w in zip(members, want):                       # the same assignments one by one
        f1, c1 = ctx.check_assignments(z)
        assert (int(f1[0]), int(c1[0])) == w


@pytest.mark.parametrize("shape", [(1, 3, 2), (63, 70, 3), (64, 70, 3), (65, 70, 3), (257, 300, 4)])
@pytest.mark.parametrize("curve", CURVES)
def test_edge_sizes(gpu, curve, shape):
    """one row; one short of, exactly and one past a wavefront; one past a workgroup"""
    c = synth.make_circuit(curve, *shape, seed=7)
    zs = [c.z]
    want = [(-1, 0)]
    for k in sorted({0, c.m - 1}):
        z_int, z = R.corrupt_row(c, k)
        zs.append(z)
        want.append(R.verdict(c, z_int))
        assert want[-1][0] == k
    first, count = gpu.r1cs_check(curve, c.A, c.B, c.C, c.m, c.V, R.stack(zs))
    assert list(zip(first.tolist(), count.tolist())) == want


@pytest.mark.parametrize("curve", CURVES)
def test_rows_without_entries(gpu, curve):
    """the sparse profile's boolean rows have an empty C (<C_i, z> = 0): a wrong boolean is caught there, a right one passes"""
    c, _, ctx = context(gpu, curve)
    k = R.empty_c_row(c)
    z_int, z = R.corrupt_row(c, k)
    first, count = R.verdict(c, z_int)
    assert first == k
    assert both_forms(gpu, c, ctx, z) == ([first], [count])


@pytest.mark.parametrize("curve", CURVES)
def test_chunk_boundary(gpu, curve):
    """65 537 assignments of three variables (6 MB): one more than two launches of at most 65 535 hold, with bad assignments
    exactly at the first index, at the last two of the first launch's range and at the first of the next"""
    c, _, ctx = context(gpu, curve, shape=(1, 3, 2))
    z_int, z_bad = R.corrupt_row(c, 0)
    good, bad = R.verdict(c), R.verdict(c, z_int)
    assert good == (-1, 0) and bad == (0, 1)
    k, at = 65537, (0, 65534, 65535, 65536)
    zs = np.ascontiguousarray(np.broadcast_to(c.z, (k,) + c.z.shape))
    zs[list(at)] = z_bad
    want_first, want_count = np.full(k, good[0], dtype=np.int64), np.full(k, good[1], dtype=np.int64)
    want_first[list(at)], want_count[list(at)] = bad
    for first, count in (gpu.r1cs_check(curve, c.A, c.B, c.C, c.m, c.V, zs), ctx.check_assignments(zs)):
        assert (first == want_first).all() and (count == want_count).all()


def test_state_error_before_set_r1cs(gpu):
    c, pk = _key(0)
    ctx = gpu.ProvingContext(0, pk)
    with pytest.raises(gpu.MantaGpuError) as e:
        ctx.check_assignments(c.z)
    assert e.value.status == 5


@pytest.mark.parametrize("curve", CURVES)
def test_agreement_with_the_prover(gpu, curve):
    """what the check says about a good and a bad assignment is what verifying their proofs says, and checking changes no
    proof byte: the proofs of a context that was never checked are the proofs of one checked before and after"""
    c, pk, plain = context(gpu, curve)
    _, _, ctx = context(gpu, curve)
    _, z_bad = R.corrupt_row(c, 64)
    zs = R.stack([c.z, z_bad])
    rs = H.rand_fr_mont(curve, 4, seed=23)
    want = gpu.Groth16.prove_batch(plain, zs, rs[:2], rs[2:])
    first, count = ctx.check_assignments(zs)
    assert first.tolist() == [-1, 64] and count[0] == 0 and count[1] >= 1
    got = gpu.Groth16.prove_batch(ctx, zs, rs[:2], rs[2:])
    assert ctx.check_assignments(zs)[0].tolist() == [-1, 64]
    single = gpu.Groth16.prove_with_randomness(ctx, c.z, rs[0], rs[2])
    assert got == want and single == want[0]
    assert O.groth16_verify(curve, pk, c.z[1:c.P], got[0]) == 1
    assert O.groth16_verify(curve, pk, c.z[1:c.P], got[1]) == 0


@pytest.mark.parametrize("curve", CURVES)
def test_beside_proofs_in_flight(gpu, curve):
    """two threads on one context, 20 rounds each: a batch of 8 proofs and a check; every result is its single-threaded value"""
    c, _, ctx = context(gpu, curve)
    re = synth.Reassigner(c)
    zs = R.stack([re.assign(s).z for s in range(1, 7)] + [R.corrupt_row(c, 255)[1], R.corrupt(c, c.P, c.P + 332)[1]])
    rs = H.rand_fr_mont(curve, 16, seed=29)
    want_proofs = gpu.Groth16.prove_batch(ctx, zs, rs[:8], rs[8:])
    want = [x.tolist() for x in ctx.check_assignments(zs)]
    assert want[0] == [-1] * 6 + [255, 0]
    wrong = []

    def rounds(what, step, expected):
        try:
            for i in range(20):
                if step() != expected:
                    wrong.append((what, i))
        except Exception as e:  # (an exception in a thread would otherwise pass unseen)
            wrong.append((what, repr(e)))

    ts = [threading.Thread(target=rounds, args=("proofs", lambda: gpu.Groth16.prove_batch(ctx, zs, rs[:8], rs[8:]), want_proofs)),
          threading.Thread(target=rounds, args=("check", lambda: [x.tolist() for x in ctx.check_assignments(zs)], want))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not wrong, wrong
