"""CPU tests of the batched Schnorr authorization signatures (mg_blake2s256, mg_schnorr_challenges, mg_signatures_verify,
mg_signatures_sign): the library's Blake2s -- the source the challenge kernel compiles -- against RFC 7693 and hashlib; the
Python restatement the GPU tests check against (tests/schnorr_ref.py) for its reduction mod l and its own consistency; and
every argument check of the C ABI, which answers MG_ERROR_INVALID_ARGUMENT before any device work, so these run without a GPU."""
import ctypes
import hashlib
import os
import random
import re

import numpy as np
import pytest

import edwards_ref as E
import schnorr_ref as S
import utxo_ref as U
from manta_rs_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = 1  # MG_ERROR_INVALID_ARGUMENT
R, L = S.R, S.L
FILES = [U.read(n) for n in U.FILES]


def mont_points(points):
    return synth.to_mont([c for p in points for c in p], R, 4).reshape(-1, 8)


def test_blake2s_rfc7693_vector():
    from manta_rs_amd import api
    want = "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"  # RFC 7693 appendix B
    assert hashlib.blake2s(b"abc").hexdigest() == want
    assert api.blake2s(b"abc").hex() == want


def test_blake2s_equals_hashlib_at_every_length():
    """0..200 covers the empty stream, the tails of 1 to 3 bytes, 63 / 64 / 65 and 127 / 128 / 129 (the final-block rule: an
    exact multiple of 64 finalises its last full block); 1 KiB +- 1 the same behind many blocks"""
    from manta_rs_amd import api
    data = random.Random(11).randbytes(1025)
    for n in list(range(201)) + [1023, 1024, 1025]:
        assert api.blake2s(data[:n]) == hashlib.blake2s(data[:n]).digest(), n
    assert api.LIB.mg_blake2s256(None, ctypes.c_size_t(0), ctypes.create_string_buffer(32)) == 0
    assert api.LIB.mg_blake2s256(None, ctypes.c_size_t(1), ctypes.create_string_buffer(32)) == INVALID
    assert api.LIB.mg_blake2s256(b"abc", ctypes.c_size_t(3), None) == INVALID


def test_reduction_mod_l_reaches_every_quotient():
    assert S.MAX_QUOTIENT == 42 and 42 * L < 1 << 256 < 43 * L and 32 * L < 1 << 256
    rng = random.Random(13)
    edge = [0, 1, (1 << 256) - 1] + [k * L + d for k in range(1, 43) for d in (-1, 0, 1)]
    seen = set()
    for v in edge:
        got, q = S.rem_mod_l(v)
        assert got == v % L and q == v // L
    for _ in range(20000):  # digests are uniform 256-bit strings: the quotient 42 has probability 0.7 %
        v = int.from_bytes(hashlib.blake2s(rng.randbytes(8)).digest(), "little")
        got, q = S.rem_mod_l(v)
        assert got == v % L and q == v // L
        seen.add(q)
    assert seen == set(range(43))


def test_model_signatures_are_consistent():
    g = E.generator()
    rng = random.Random(17)
    assert E.on_curve((0, R - 1)) and not E.in_subgroup((0, R - 1))
    for msg in (b"", b"a", rng.randbytes(100)):
        sk, k = rng.randrange(1, L), rng.randrange(1, L)
        s, rp, pk = S.sign(g, sk, k, msg)
        assert rp == E.mul(g, k) and pk == E.mul(g, sk) and s < L
        assert S.verify(g, pk, msg, s, rp) == S.OK
        assert S.verify(g, pk, msg + b"x", s, rp) == S.MISMATCH
        assert S.verify(g, pk, msg, (s + 1) % L, rp) == S.MISMATCH
        assert S.verify(g, E.mul(g, sk + 1), msg, s, rp) == S.MISMATCH
        assert S.verify(g, pk, msg, s + L, rp) == S.BAD_ENCODING
        assert S.verify(g, (0, 0), msg, s, rp) == S.BAD_ENCODING and S.verify(g, pk, msg, s, (pk[0] + R, pk[1])) == S.BAD_ENCODING
        s0, rp0, pk0 = S.sign(g, 0, k, msg)  # sk = 0: s = k, so s G == R
        assert pk0 == E.IDENTITY and s0 == k and S.verify(g, pk0, msg, s0, rp0) == S.DEGENERATE
        s1, rp1, pk1 = S.sign(g, sk, 0, msg)  # k = 0: R is the identity, which is a point like any other
        assert rp1 == E.IDENTITY and S.verify(g, pk1, msg, s1, rp1) == S.OK


def test_argument_checks_need_no_gpu():
    from manta_rs_amd import api
    m = api.UtxoModel(*FILES)
    lib, p, sz = api.LIB, api._p, api._sz
    n, stride = 3, 8
    pts = np.repeat(mont_points([E.generator()]), n, axis=0)
    sc = api.edwards_scalars([5, 6, 7])
    msg = np.zeros((n, stride), dtype=np.uint8)
    lens = np.array([0, 3, 8], dtype=np.uint32)
    out4, out8, out8b = (np.zeros((n, w), dtype=np.uint64) for w in (4, 8, 8))
    st = np.zeros(n, dtype=np.uint8)
    n_ok = ctypes.c_size_t(7)

    def challenges(h=m._h, pk=p(pts), rp=p(pts), ms=p(msg), stride=stride, ln=p(lens), n=n, out=p(out4)):
        return lib.mg_schnorr_challenges(h, pk, rp, ms, sz(stride), ln, sz(n), out)

    def verify(h=m._h, pk=p(pts), rp=p(pts), s=p(sc), ms=p(msg), stride=stride, ln=p(lens), n=n, status=p(st)):
        return lib.mg_signatures_verify(h, pk, rp, s, ms, sz(stride), ln, sz(n), status, ctypes.byref(n_ok))

    def sign(h=m._h, sk=p(sc), k=p(sc), ms=p(msg), stride=stride, ln=p(lens), n=n, s=p(out4), rp=p(out8), pk=p(out8b)):
        return lib.mg_signatures_sign(h, sk, k, ms, sz(stride), ln, sz(n), s, rp, pk)

    # a NULL required array, a NULL model
    for call, names in ((challenges, ("h", "pk", "rp", "ms", "out")), (verify, ("h", "pk", "rp", "s", "ms")),
                        (sign, ("h", "sk", "k", "ms", "s", "rp"))):
        for name in names:
            assert call(**{name: None}) == INVALID, (call.__name__, name)
        # the stride: a multiple of 4, at most MG_SIGNATURE_MAX_MESSAGE
        for bad in (1, 2, 3, 6, stride + 1, api.SIGNATURE_MAX_MESSAGE + 4, 1 << 40):
            assert call(stride=bad) == INVALID, (call.__name__, bad)
        # a length beyond the stride, in any lane
        for i in range(n):
            over = lens.copy()
            over[i] = stride + 1
            assert call(ln=p(over)) == INVALID, (call.__name__, i)
        # n = 0 succeeds without a device and touches nothing
        assert call(n=0) == 0
    assert lib.mg_schnorr_challenges(m._h, None, None, None, sz(0), None, sz(0), None) == 0
    assert lib.mg_signatures_verify(m._h, None, None, None, None, sz(0), None, sz(0), None, None) == 0
    assert lib.mg_signatures_sign(m._h, None, None, None, sz(0), None, sz(0), None, None, None) == 0
    # signing: a key or a nonce of l or more is the caller's own mistake
    for bad in (L, L + 1, (1 << 256) - 1):
        for i in range(n):
            vals = [5, 6, 7]
            vals[i] = bad
            assert sign(sk=p(api.edwards_scalars(vals))) == INVALID and sign(k=p(api.edwards_scalars(vals))) == INVALID
    # the wrapper refuses the same through the exception
    for call in (lambda: m.schnorr_challenges(pts, pts, np.zeros((n, 6), dtype=np.uint8)),
                 lambda: m.verify_signatures(pts, pts, sc, msg, lengths=[9, 0, 0]),
                 lambda: m.sign(api.edwards_scalars([L, 1, 1]), sc, msg)):
        with pytest.raises(api.MantaGpuError) as e:
            call()
        assert e.value.status == INVALID
    h = m.schnorr_challenges(pts[:0], pts[:0], msg[:0])
    stt, ok = m.verify_signatures(pts[:0], pts[:0], sc[:0], msg[:0])
    s, rp, pk = m.sign(sc[:0], sc[:0], msg[:0])
    assert h.shape == (0, 4) and stt.shape == (0,) and ok == 0 and s.shape == (0, 4) and rp.shape == (0, 8) and pk.shape == (0, 8)
    m.close()


def test_no_gpu_is_an_error_not_a_fallback():
    from manta_rs_amd import api
    try:
        n = api.device_count()
    except api.MantaGpuError:
        n = 0
    if n:
        return  # the GPU suite covers the compute paths
    m = api.UtxoModel(*FILES)
    g = mont_points([E.generator()])
    one = api.edwards_scalars([1])
    for msg in (np.zeros((1, 4), dtype=np.uint8), np.zeros((1, 0), dtype=np.uint8)):
        for call in (lambda: m.schnorr_challenges(g, g, msg), lambda: m.verify_signatures(g, g, one, msg), lambda: m.sign(one, one, msg),
                     lambda: m.sign(one, one, msg, pks=False)):
            with pytest.raises(api.MantaGpuError) as e:
                call()
            assert e.value.status in (2, 3)  # MG_ERROR_HIP / MG_ERROR_OUT_OF_MEMORY: the device's refusal, never a result


def test_constants_match_the_header():
    from manta_rs_amd import api
    hdr = open(os.path.join(HERE, "..", "include", "mantagpu.h")).read()
    for name, val, ref in (("MG_SIG_OK", api.SIG_OK, S.OK), ("MG_SIG_BAD_ENCODING", api.SIG_BAD_ENCODING, S.BAD_ENCODING),
                           ("MG_SIG_DEGENERATE", api.SIG_DEGENERATE, S.DEGENERATE), ("MG_SIG_MISMATCH", api.SIG_MISMATCH, S.MISMATCH)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val == ref
    shift = int(re.search(r"#define MG_SIGNATURE_MAX_MESSAGE \(1u << (\d+)\)", hdr).group(1))
    assert 1 << shift == api.SIGNATURE_MAX_MESSAGE
