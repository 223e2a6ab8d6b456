"""The host-array entry points on a machine WITHOUT a device: every one of them takes arrays in the caller's memory, asks for its
stream and its device block (staging.h DevCall), finds neither, and has to say so -- a status (MG_ERROR_HIP or
MG_ERROR_OUT_OF_MEMORY; the scope asks for the stream first, so it is the latter), the caller's output arrays as they were, and a
process that goes on to the next call. Smallest legal inputs: four elements, eight pairs, one tree of two leaves, a circuit of two
constraints. Skipped where a device answers: there the GPU suite runs the same calls for their results."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from manta_rs_amd import api

MG_ERROR_HIP, MG_ERROR_OUT_OF_MEMORY = 2, 3
SENTINEL = 0xA5A5A5A5


def _devices():
    try:
        return api.device_count()
    except api.MantaGpuError:
        return 0


pytestmark = pytest.mark.skipif(_devices() >= 1, reason="a device answers: the GPU suite covers these calls")

sz, u32 = ctypes.c_size_t, ctypes.c_uint32


def refused(call, *args, **kw):
    """the call raises MantaGpuError with one of the two statuses of a missing device"""
    with pytest.raises(api.MantaGpuError) as e:
        call(*args, **kw)
    assert e.value.status in (MG_ERROR_HIP, MG_ERROR_OUT_OF_MEMORY), e.value
    return e.value.status


def elements(n, limbs=4, dtype=np.uint64):
    return (np.arange(n * limbs, dtype=dtype) + 1).reshape(n, limbs)


def circuit():
    """two constraints over three variables, one of them public: x0 * x1 = x2 twice"""
    def mat(col):
        return SimpleNamespace(row_ptr=np.array([0, 1, 2], dtype=np.uint32), col=np.array([col, col], dtype=np.uint32),
                               val=np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), (2, 1)))
    return SimpleNamespace(A=mat(0), B=mat(1), C=mat(2), m=2, P=1, V=3)


def hasher():
    full, partial = 2, 1
    return api.PoseidonHasher(api.BN254, 3, full, partial, bytes(32 * api.poseidon_param_count(3, full, partial)))


def test_field_and_pairing_operations_report_the_missing_device():
    refused(api.field_op, "bn254_fr", "mul", elements(4), elements(4))
    refused(api.field_op, "bls381_fq", "sqr", elements(4, 6))
    refused(api.fpr_raw_op, "bn254_fq", "mul_add", *[elements(4, 9, np.uint32)] * 4)
    refused(api.pairing_op, api.BN254, "fq_half", elements(4, 8, np.uint32))
    refused(api.pairing_op, api.BN254, "fq2_mul", elements(4, 16, np.uint32), elements(4, 16, np.uint32))
    refused(api.Radix2EvaluationDomain(api.BN254, 4).fft, elements(4))


def test_the_msm_front_end_calls_leave_the_callers_arrays_alone():
    sc = elements(4)
    layout, cnt = (u32 * 4)(), u32(7)

    def untouched(rc, *arrays):
        assert rc in (MG_ERROR_HIP, MG_ERROR_OUT_OF_MEMORY), rc
        for a in arrays:
            assert (a == SENTINEL).all()

    # eight pairs
    keys, vals = np.arange(8, dtype=np.uint32)[::-1].copy(), np.arange(8, dtype=np.uint32)
    ko, vo = np.full(8, SENTINEL, dtype=np.uint32), np.full(8, SENTINEL, dtype=np.uint32)
    untouched(api.LIB.mg_sort_pairs(api._p(keys), api._p(vals), sz(8), 3, None, u32(0xFFFFFFFF), u32(0xFFFFFFFF), api._p(ko), api._p(vo)), ko, vo)
    # four scalars over four bases: c = 16 is 16 windows, the fixed layout and the compacted one
    k, v = np.full(16 * 4, SENTINEL, dtype=np.uint32), np.full(16 * 4, SENTINEL, dtype=np.uint32)
    for compact in (0, 1):
        untouched(api.LIB.mg_msm_digits(api.BN254, api._p(sc), sz(1), sz(4), 0, 16, 0, sz(4), None, sz(1), sz(4), compact, api._p(k), api._p(v),
                                        ctypes.byref(cnt) if compact else None, layout), k, v)
    assert cnt.value == 7
    untouched(api.LIB.mg_msm_dense_front(api.BN254, api._p(sc), sz(4), 0, 16, sz(4), None, sz(4), api._p(k), api._p(v), layout), k, v)
    # and through the binding
    refused(api.sort_pairs, keys, vals, 3)
    refused(api.msm_digits, api.BN254, sc, 16, 4)
    refused(api.msm_dense_front, api.BN254, sc, 16, 4)


def test_group_operations_and_codecs_report_the_missing_device():
    refused(api.ec_elementwise, api.BN254, 1, api.EC_ADD_MIXED, elements(4, 8), elements(4, 8))
    refused(api.ec_elementwise, api.BLS12_381, 2, api.EC_DOUBLE, elements(4, 24))
    refused(api.group_ntt, api.BN254, 1, elements(4, 8))
    refused(api.edwards_check, elements(4, 8))
    refused(api.points_decode, api.BN254, 1, bytes(4 * 32))


def test_poseidon_and_merkle_calls_report_the_missing_device():
    h = hasher()
    refused(h.permute, elements(4 * 3).reshape(4, 3, 4))
    refused(h.hash, elements(4 * 2).reshape(4, 2, 4))
    refused(api.merkle_tree, h, 2, elements(2), [0])
    refused(api.merkle_forest_roots, h, 2, elements(2), [0, 2])
    h.close()


def test_circuit_calls_report_the_missing_device():
    c = circuit()
    z = elements(3)
    refused(api.r1cs_check, api.BN254, c.A, c.B, c.C, c.m, c.V, np.stack([z] * 4))
    refused(api.qap_columns, api.BN254, 1, [elements(2, 8)], [c.A], c.V)
    r1cs = api.R1CS(api.BN254, c.A, c.B, c.C, c.m, c.P, z)
    refused(api.groth16_setup, r1cs, c.V, elements(5), elements(1, 8), elements(1, 16))
    D = 4  # the domain of m + P = 3 rows
    refused(api.mpc_initialize, api.BN254, elements(2 * D - 1, 8), elements(D, 16), elements(D, 8), elements(D, 8), elements(1, 16), r1cs,
            c.V, D - 1, elements(1, 8), elements(1, 16))
