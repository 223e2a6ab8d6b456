"""CPU tests (no GPU) of what mg_qap_columns and mg_mpc_initialize refuse: every malformed call comes back with
MG_ERROR_INVALID_ARGUMENT (or MG_ERROR_DOMAIN_TOO_LARGE) before any device work -- on a machine without a GPU a call that
reached the device would answer with a HIP status instead -- and leaves the output arrays as the caller filled them."""
import ctypes

import numpy as np
import pytest

from manta_rs_amd import api, synth

INVALID, DOMAIN = 1, 4
FILL = 0xA5A5A5A5A5A5A5A5
M, NCOLS = 6, 5


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except api.MantaGpuError as e:
        return e.status if hasattr(e, "status") else e.args[0]
    return 0


def _matrix(curve, m=M, n_cols=NCOLS, per_row=2):
    r = synth.FR_MODULUS[curve]
    row_ptr = np.arange(0, per_row * (m + 1), per_row, dtype=np.uint32)
    col = (np.arange(per_row * m, dtype=np.uint32) * 3) % n_cols
    val = synth.to_mont([(7 * k + 1) % r for k in range(per_row * m)], r, 4)
    return synth.CSR(row_ptr, col.astype(np.uint32), val)


def _raw_qap_columns(curve, group, n_terms, bases_ptrs, mat_ptrs, m, n_cols, out):
    return api.LIB.mg_qap_columns(curve, group, ctypes.c_size_t(n_terms), bases_ptrs, mat_ptrs, ctypes.c_uint64(m),
                                  ctypes.c_uint64(n_cols), ctypes.c_uint32(0), api._p(out))


@pytest.mark.parametrize("curve,group", [(0, 1), (0, 2), (1, 1), (1, 2)])
def test_qap_columns_refuses_malformed_calls_and_leaves_out_alone(curve, group):
    w = api.affine_limbs(curve, group)
    basis = np.ones((M, w), dtype=np.uint64)
    out = np.full((NCOLS, w), FILL, dtype=np.uint64)
    good = _matrix(curve)

    def call(mat, n_cols=NCOLS, grp=group, bases=None, n_terms=1, mats=None):
        keep, csr = api._csr(mat)
        bp = (ctypes.c_void_p * 1)(basis.ctypes.data if bases is None else bases)
        mp = (ctypes.POINTER(api._Csr) * 1)(ctypes.pointer(csr) if mats is None else mats)
        rc = _raw_qap_columns(curve, grp, n_terms, bp, mp, M, n_cols, out)
        assert (out == FILL).all(), "a refused call wrote to the output"
        return rc

    # the control: the well-formed call is not refused (it succeeds on a GPU and answers with a HIP status without one)
    keep, csr = api._csr(good)
    scratch = np.zeros((NCOLS, w), dtype=np.uint64)
    assert _raw_qap_columns(curve, group, 1, (ctypes.c_void_p * 1)(basis.ctypes.data),
                            (ctypes.POINTER(api._Csr) * 1)(ctypes.pointer(csr)), M, NCOLS, scratch) != INVALID
    bad_col = _matrix(curve)
    bad_col.col[3] = NCOLS
    assert call(bad_col) == INVALID                      # a column >= n_cols
    dip = _matrix(curve)
    dip.row_ptr[2] = dip.row_ptr[1] - 1
    assert call(dip) == INVALID                          # row_ptr not monotone
    short = _matrix(curve)
    short.row_ptr[M] -= 1
    assert call(short) == INVALID                        # row_ptr[m] != nnz
    first = _matrix(curve)
    first.row_ptr[0] = 1
    assert call(first) == INVALID                        # row_ptr[0] != 0
    assert call(good, n_terms=0) == INVALID
    assert call(good, bases=0) == INVALID                # a NULL basis
    assert call(good, mats=ctypes.POINTER(api._Csr)()) == INVALID   # a NULL matrix
    assert call(good, n_cols=0) == INVALID
    for grp in (0, 3, -1):
        assert call(good, grp=grp) == INVALID
    assert _raw_qap_columns(curve, group, 1, None, None, M, NCOLS, out) == INVALID
    assert (out == FILL).all()
    # the Python wrapper raises the same status
    assert _status(api.qap_columns, curve, group, [basis], [bad_col], NCOLS) == INVALID


def test_qap_columns_without_entries_is_all_infinity_and_needs_no_device():
    """nnz = 0 in every term: the sums are the point at infinity, known before any device work."""
    for curve, group in ((0, 1), (1, 2)):
        w = api.affine_limbs(curve, group)
        empty = synth.CSR(np.zeros(M + 1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint64))
        out = api.qap_columns(curve, group, [np.ones((M, w), dtype=np.uint64)] * 2, [empty, empty], NCOLS)
        assert out.shape == (NCOLS, w) and not out.any()


def _initialize_call(curve, c, n_g1, n_g2, h_len, mats=None, n_vars=None, n_inputs=None):
    """mg_mpc_initialize on accumulator arrays of ones (never read by a refused call); returns (status, outputs untouched)"""
    w1, w2 = api.affine_limbs(curve, 1), api.affine_limbs(curve, 2)
    V, P = c.V if n_vars is None else n_vars, c.P if n_inputs is None else n_inputs
    vecs = [np.ones((max(n_g1, 1), w1), dtype=np.uint64), np.ones((max(n_g2, 1), w2), dtype=np.uint64),
            np.ones((max(n_g2, 1), w1), dtype=np.uint64), np.ones((max(n_g2, 1), w1), dtype=np.uint64), np.ones((1, w2), dtype=np.uint64)]
    view = api._KzgView(n_g1, n_g2, *[api._p(v) for v in vecs])
    sizes = {"alpha_g1": (1, w1), "beta_g1": (1, w1), "delta_g1": (1, w1), "beta_g2": (1, w2), "gamma_g2": (1, w2),
             "delta_g2": (1, w2), "gamma_abc_g1": (c.P, w1), "a_query": (c.V, w1), "b_g1_query": (c.V, w1),
             "b_g2_query": (c.V, w2), "h_query": (c.D, w1), "l_query": (c.V - c.P, w1)}
    outs = {k: np.full(s, FILL, dtype=np.uint64) for k, s in sizes.items()}
    out = api._PkOut(*[api._p(outs[k]) for k, _ in api._PkOut._fields_])
    keep = [api._csr(M_) for M_ in (mats or (c.A, c.B, c.C))]
    g1, g2 = np.ones(w1, dtype=np.uint64), np.ones(w2, dtype=np.uint64)
    rc = api.LIB.mg_mpc_initialize(curve, ctypes.byref(view), ctypes.byref(keep[0][1]), ctypes.byref(keep[1][1]),
                                   ctypes.byref(keep[2][1]), ctypes.c_uint64(c.m), ctypes.c_uint64(V), ctypes.c_uint64(P),
                                   ctypes.c_uint64(h_len), api._p(g1), api._p(g2), ctypes.byref(out))
    return rc, all((v == FILL).all() for v in outs.values())


@pytest.mark.parametrize("curve", [0, 1])
def test_mpc_initialize_refuses_malformed_calls_and_leaves_out_alone(curve):
    import copy
    c = synth.make_circuit(curve, 27, 20, 4, seed=81)   # D = 32
    D = c.D

    def refused(status=INVALID, **kw):
        args = dict(n_g1=2 * D, n_g2=D, h_len=D - 1)
        args.update(kw)
        rc, untouched = _initialize_call(curve, c, **args)
        assert untouched, "a refused call wrote to the key"
        return rc == status

    # the control: well-formed calls pass every check and reach the device -- success on a GPU, a HIP status without one, never
    # a refusal (without it a validator that refused everything would pass all of the assertions below)
    for kw in (dict(n_g1=2 * D, n_g2=D, h_len=D - 1), dict(n_g1=2 * D - 1, n_g2=D, h_len=D - 1), dict(n_g1=2 * D, n_g2=D, h_len=D)):
        rc, _ = _initialize_call(curve, c, **kw)
        assert rc not in (INVALID, DOMAIN), kw
    for h_len in (0, D - 2, D + 1, 2 * D):
        assert refused(h_len=h_len)                       # h_len other than D - 1 or D
    assert refused(n_g1=2 * D - 2)                        # tau^(2D-2) G is needed for h_len = D - 1 ...
    assert refused(n_g1=2 * D - 1, h_len=D)               # ... and tau^(2D-1) G for h_len = D
    assert refused(n_g2=D - 1)                            # fewer than D powers in G2 / of alpha and beta
    assert refused(n_g1=0, n_g2=0)

    def with_matrix(which, edit):
        mats = [copy.deepcopy(x) for x in (c.A, c.B, c.C)]
        edit(mats[which])
        return mats

    def bad_col(M_):
        M_.col[len(M_.col) // 2] = c.V

    def dip(M_):
        M_.row_ptr[3] = M_.row_ptr[4] + 1

    def short(M_):
        M_.row_ptr[c.m] += 1

    for which in range(3):
        for edit in (bad_col, dip, short):
            assert refused(mats=with_matrix(which, edit)), (which, edit.__name__)
    assert refused(n_inputs=0) and refused(n_inputs=c.V) and refused(n_vars=1, n_inputs=1)
    # NULL arguments
    w1 = api.affine_limbs(curve, 1)
    keep, csr = api._csr(c.A)
    out = api._PkOut()
    rc = api.LIB.mg_mpc_initialize(curve, None, ctypes.byref(csr), ctypes.byref(csr), ctypes.byref(csr), ctypes.c_uint64(c.m),
                                   ctypes.c_uint64(c.V), ctypes.c_uint64(c.P), ctypes.c_uint64(D - 1),
                                   api._p(np.ones(w1, dtype=np.uint64)), api._p(np.ones(w1, dtype=np.uint64)), ctypes.byref(out))
    assert rc == INVALID
    assert api.LIB.mg_mpc_initialize(7, None, None, None, None, ctypes.c_uint64(1), ctypes.c_uint64(2), ctypes.c_uint64(1),
                                     ctypes.c_uint64(1), None, None, None) == INVALID


def test_mpc_initialize_domain_beyond_the_two_adicity_is_too_many_constraints():
    """BN254's scalar field has two-adicity 28: m + P > 2^28 is the reference's `TooManyConstraints`, decided from the
    sizes alone before the matrices are read (so small placeholders stand in for them here)."""
    curve = 0
    c = synth.make_circuit(curve, 27, 20, 4, seed=81)
    c.m = (1 << 28) + 1
    rc, untouched = _initialize_call(curve, c, n_g1=8, n_g2=4, h_len=3)
    assert rc == DOMAIN and untouched
