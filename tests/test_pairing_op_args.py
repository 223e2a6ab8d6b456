"""CPU test (no GPU) of what mg_pairing_op refuses: every malformed call comes back with MG_ERROR_INVALID_ARGUMENT before any
device work -- on a machine without a GPU a call that reached the device would answer with a HIP status instead -- and leaves
the output array as the caller filled it."""
import numpy as np
import pytest

from manta_rs_amd import api

INVALID = 1
FILL = 0xA5A5A5A5


@pytest.mark.parametrize("curve", [0, 1])
def test_pairing_op_refuses_malformed_calls_and_leaves_the_output_alone(curve):
    N = 2 * api.FQ_LIMBS[curve]
    n = 3
    a = np.ones((n, 12 * N), dtype=np.uint32)
    ten = np.ones((n, 10, N), dtype=np.uint32)
    out = np.full((n, 12 * N), FILL, dtype=np.uint32)
    ops = api.PAIRING_OPS

    def call(op, a_=a, b_=None, cf=None, n_=n, out_=out, cv=curve):
        return api.LIB.mg_pairing_op(cv, op, api._p(a_), api._p(b_), api._p(cf), api._sz(n_), api._p(out_))

    def refused(*args, **kw):
        rc = call(*args, **kw)
        assert (out == FILL).all(), "a refused call wrote to the output"
        return rc == INVALID

    good = np.array([[255, -255] + [0] * 8] * n, dtype=np.int16)
    # the controls: well-formed calls are not refused (they succeed on a GPU and answer with a HIP status without one)
    scratch = np.zeros_like(out)
    assert call(ops["sqr12"], out_=scratch) != INVALID
    assert call(ops["mul12"], b_=a, out_=scratch) != INVALID
    assert call(ops["fq_lincomb"], a_=ten, cf=good, out_=scratch) != INVALID

    assert sorted(ops.values()) == list(range(16))
    for op in (-1, 16, 99):
        assert refused(op, b_=a, cf=good), op                       # an unknown op
    for name in ("mul12", "ell", "fq2_mul"):
        assert refused(ops[name]), name                             # the second operand is missing
    for name in ops:
        assert refused(ops[name], a_=None, b_=a, cf=good), name     # no first operand
        assert refused(ops[name], b_=a, cf=good, out_=None), name   # no output
        assert refused(ops[name], b_=a, cf=good, n_=0), name        # n = 0
        assert refused(ops[name], b_=a, cf=good, n_=65537), name    # more than a call takes
    for cv in (2, 7, -1):
        assert refused(ops["sqr12"], cv=cv)                         # an unknown curve
    assert refused(ops["fq_lincomb"], a_=ten)                       # no coefficients
    for row in ([255, 1] + [0] * 8, [-255, -1] + [0] * 8, [128, 128] + [0] * 8, [-26] * 10, [256] + [0] * 9, [0] * 9 + [-256],
                [300, -300] + [0] * 8):
        cf = good.copy()
        cf[n - 1] = row                                             # the last row alone is out of range
        assert refused(ops["fq_lincomb"], a_=ten, cf=cf), row
    # the Python wrapper raises the same status
    with pytest.raises(api.MantaGpuError) as e:
        api.pairing_op(curve, "fq_lincomb", ten, coeffs=np.array([[128, 128] + [0] * 8] * n, dtype=np.int16))
    assert e.value.status == INVALID
