"""CPU tests of the plain-integer reference the GPU tests of the R1CS check compare against (tests/r1cs_check_ref.py): it agrees
with synth.check_satisfied, the generators' own assignments have no failing row, and the corruption the GPU tests lean on does
what they assume -- for both curves and all three witness profiles."""
import pytest

import r1cs_check_ref as R
from manta_rs_amd import synth

CASES = [(curve, profile) for curve in (0, 1) for profile in synth.PROFILES]


@pytest.mark.parametrize("curve,profile", CASES)
def test_generated_assignments_have_no_failing_row(curve, profile):
    c = R.circuit(curve, profile)
    assert synth.check_satisfied(c) and R.failing_rows(c) == [] and R.verdict(c) == (-1, 0)
    re = synth.Reassigner(c)
    for seed in (1, 2, 3):
        d = re.assign(seed)
        assert synth.check_satisfied(d) and R.failing_rows(d) == []
    for shape in ((1, 3, 2), (63, 70, 3), (64, 70, 3), (65, 70, 3), (257, 300, 4)):
        e = synth.make_circuit(curve, *shape, seed=7, profile=profile)
        assert synth.check_satisfied(e) and R.failing_rows(e) == [], shape


@pytest.mark.parametrize("curve,profile", CASES)
def test_agrees_with_check_satisfied_on_corrupted_assignments(curve, profile):
    import dataclasses
    c = R.circuit(curve, profile)
    for v in (1, c.P, c.P + 17, c.V - 1):
        z, zm = R.corrupt(c, v)
        assert synth.check_satisfied(dataclasses.replace(c, z_int=z, z=zm)) == (R.failing_rows(c, z) == []), v


@pytest.mark.parametrize("curve", [0, 1])
def test_the_other_corruptions_the_gpu_tests_use(curve):
    """what tests/test_gpu_r1cs_check.py assumes about its inputs, without a GPU"""
    c = R.circuit(curve)
    bad = R.failing_rows(c, R.corrupt(c, c.P + 300, c.P + 70, c.P + 5)[0])
    assert bad[0] == 5 and len({r // 64 for r in bad}) >= 3 and len({r // 256 for r in bad}) == 2
    two = R.failing_rows(c, R.corrupt(c, c.P, c.P + 332)[0])
    assert two[0] == 0 and two[-1] == 332
    v = R.c_only_variable(c)                      # a . b stays right, c goes wrong
    A, B, C = R._rows(c)
    rows = R.failing_rows(c, R.corrupt(c, v)[0])
    assert rows and all(any(j == v for j, _ in C[i]) and all(j != v for j, _ in A[i] + B[i]) for i in rows)
    k = R.empty_c_row(c)                          # a row whose C has no entry
    assert c.C.row_ptr[k] == c.C.row_ptr[k + 1] and R.failing_rows(c, R.corrupt_row(c, k)[0])[0] == k
    for shape in ((1, 3, 2), (63, 70, 3), (64, 70, 3), (65, 70, 3), (257, 300, 4)):
        e = synth.make_circuit(curve, *shape, seed=7)
        for k in (0, e.m - 1):
            assert R.failing_rows(e, R.corrupt_row(e, k)[0])[0] == k, (shape, k)


@pytest.mark.parametrize("curve,profile", CASES)
def test_corrupting_the_variable_of_row_k_makes_row_k_the_first_failing_row(curve, profile):
    c = R.circuit(curve, profile)
    for k in R.ROWS:
        z, _ = R.corrupt_row(c, k)
        bad = R.failing_rows(c, z)
        assert bad and bad[0] == k and 1 <= len(bad) <= 10, (k, bad)
