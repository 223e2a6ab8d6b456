"""CPU tests (no GPU) of what mg_r1cs_check and mg_ctx_r1cs_check refuse: every malformed call comes back with
MG_ERROR_INVALID_ARGUMENT before any device work -- on a machine without a GPU a call that reached the device would answer
with a HIP status instead -- and leaves both output arrays as the caller filled them. Empty work (k = 0, no constraint row)
succeeds without a device."""
import copy
import ctypes

import numpy as np
import pytest

import r1cs_check_ref as R
from manta_rs_amd import api

INVALID = 1
FILL = 0xA5A5A5A5A5A5A5A5
K = 3


def _call(curve, mats, m, n_vars, k, z, first, count):
    keep = [api._csr(M) if M is not None else (None, None) for M in mats]
    ptr = [ctypes.byref(x[1]) if x[1] is not None else None for x in keep]
    return api.LIB.mg_r1cs_check(curve, ptr[0], ptr[1], ptr[2], ctypes.c_uint64(m), ctypes.c_uint64(n_vars), ctypes.c_uint64(k),
                                 api._p(z), api._p(first), api._p(count))


@pytest.mark.parametrize("curve", [0, 1])
def test_r1cs_check_refuses_malformed_calls_and_leaves_outputs_alone(curve):
    c = R.circuit(curve)
    zs = R.stack([c.z] * K)
    first, count = np.full(K, FILL, dtype=np.uint64), np.full(K, FILL, dtype=np.uint64)

    def refused(mats=None, m=c.m, n_vars=c.V, k=K, z=zs, f=first, cnt=count, cv=curve):
        rc = _call(cv, mats or (c.A, c.B, c.C), m, n_vars, k, z, f, cnt)
        assert (first == FILL).all() and (count == FILL).all(), "a refused call wrote to an output"
        return rc == INVALID

    # the control: the well-formed call is not refused (it succeeds on a GPU and answers with a HIP status without one) --
    # without it a validator that refused everything would pass every assertion below
    f2, c2 = np.zeros(K, dtype=np.uint64), np.zeros(K, dtype=np.uint64)
    assert _call(curve, (c.A, c.B, c.C), c.m, c.V, K, zs, f2, c2) != INVALID
    assert _call(curve, (c.A, c.B, c.C), c.m, c.V, K, zs, f2, None) != INVALID   # the counts are optional

    def with_matrix(which, edit):
        mats = [copy.deepcopy(x) for x in (c.A, c.B, c.C)]
        edit(mats[which])
        return mats

    def bad_col(M_):
        M_.col[len(M_.col) // 2] = c.V            # a column >= n_vars

    def dip(M_):
        M_.row_ptr[3] = M_.row_ptr[4] + 1         # row_ptr not monotone

    def short(M_):
        M_.row_ptr[c.m] += 1                      # row_ptr[m] != nnz

    def first_entry(M_):
        M_.row_ptr[0] = 1                         # row_ptr[0] != 0

    for which in range(3):
        for edit in (bad_col, dip, short, first_entry):
            assert refused(mats=with_matrix(which, edit)), (which, edit.__name__)
        mats = [c.A, c.B, c.C]
        mats[which] = None
        assert refused(mats=mats), which          # a NULL matrix
    assert refused(n_vars=0)
    assert refused(n_vars=int(max(M_.col.max() for M_ in (c.A, c.B, c.C))))   # the highest column in use is out of range now
    assert refused(z=None) and refused(f=None)
    for cv in (2, 7, -1):
        assert refused(cv=cv)                     # an unknown curve
    # the Python wrapper raises the same status
    with pytest.raises(api.MantaGpuError) as e:
        api.r1cs_check(curve, *with_matrix(1, bad_col), c.m, c.V, zs)
    assert e.value.status == INVALID


def test_ctx_r1cs_check_refuses_a_null_context():
    zs = np.zeros((K, 4, 4), dtype=np.uint64)
    first, count = np.full(K, FILL, dtype=np.uint64), np.full(K, FILL, dtype=np.uint64)
    assert api.LIB.mg_ctx_r1cs_check(None, ctypes.c_uint64(K), api._p(zs), api._p(first), api._p(count)) == INVALID
    assert api.LIB.mg_ctx_r1cs_check(None, ctypes.c_uint64(0), None, None, None) == INVALID
    assert (first == FILL).all() and (count == FILL).all()


@pytest.mark.parametrize("curve", [0, 1])
def test_empty_work_succeeds_without_a_device(curve):
    c = R.circuit(curve)
    # k = 0: nothing to check, the pointers may be NULL
    assert _call(curve, (c.A, c.B, c.C), c.m, c.V, 0, None, None, None) == 0
    first, count = api.r1cs_check(curve, c.A, c.B, c.C, c.m, c.V, np.zeros((0, c.V, 4), dtype=np.uint64))
    assert first.shape == (0,) and count.shape == (0,)
    # no constraint row: every assignment satisfies the system
    empty = type(c.A)(np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint64))
    first, count = api.r1cs_check(curve, empty, empty, empty, 0, c.V, R.stack([c.z] * K))
    assert first.tolist() == [-1] * K and count.tolist() == [0] * K
    f = np.full(K, FILL, dtype=np.uint64)
    assert _call(curve, (empty, empty, empty), 0, c.V, K, R.stack([c.z] * K), f, None) == 0
    assert (f == np.uint64(api.R1CS_SATISFIED)).all()
