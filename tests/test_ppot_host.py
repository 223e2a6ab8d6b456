"""CPU tests of the Perpetual Powers of Tau reader: the Python restatement the GPU tests check against (tests/ppot_ref.py) for
its own consistency and a known answer, `ppot.position` against the reference's closed forms and the restated layout, the
library's Blake2b-512 against hashlib, and the argument checks of the C ABI that answer before any device work."""
import hashlib
import random

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
import ppot_ref as P
from manta_rs_amd import synth

INVALID = 1  # MG_ERROR_INVALID_ARGUMENT
FORMS = [(1, True), (1, False), (2, True), (2, False)]


@pytest.mark.parametrize("group,compressed", FORMS)
def test_reference_round_trip(group, compressed):
    """decode(encode(p)) == p with status 0 for 100 random points and infinity"""
    pts = H.random_points(0, group, 100, seed=610 + group)
    pts[37] = 0
    for p in pts:
        rec = P.encode(group, p, compressed)
        assert len(rec) == P.point_bytes(group, compressed)
        st, back = P.decode(group, rec, compressed)
        assert st == P.OK and (back == p).all()


def test_generator_known_answer():
    """G1's generator (1, 2): uncompressed 31 zero bytes, 01, 31 zero bytes, 02; compressed 31 zero bytes, 01 with bit 7
    clear, because 2 < q - 2"""
    g = O.generator(0, 1)
    assert synth.from_mont(g.reshape(2, 4), P.Q) == [1, 2]
    assert P.encode(1, g, False) == bytes(31) + b"\x01" + bytes(31) + b"\x02"
    assert P.encode(1, g, True) == bytes(31) + b"\x01"
    neg = g.copy()
    neg[4:] = synth.to_mont([P.Q - 2], P.Q, 4)[0]
    assert P.encode(1, neg, True) == b"\x80" + bytes(30) + b"\x01"
    assert P.encode(1, np.zeros(8, dtype=np.uint64), True) == b"\x40" + bytes(31)
    assert P.encode(2, np.zeros(16, dtype=np.uint64), False) == b"\x40" + bytes(127)


def test_position_closed_forms_and_restated_layout():
    from manta_rs_amd import ppot
    assert ppot.position("TauG1", 0, False) == 64 and ppot.position("TauG1", 0, True) == 64
    assert ppot.position("TauG2", 0, False) == 64 + 64 * (2 ** 29 - 1)
    assert ppot.position("BetaG2", 0, True) == 64 + 32 * (2 ** 29 - 1) + 64 * 2 ** 28 + 2 * 32 * 2 ** 28
    rng = random.Random(28)
    for _ in range(50):
        element = rng.choice(list(ppot.ELEMENTS))
        powers = rng.choice([1 << 28, 32, 1])
        count = 2 * powers - 1 if element == "TauG1" else 1 if element == "BetaG2" else powers
        index, compressed = rng.randrange(count), rng.random() < 0.5
        assert ppot.position(element, index, compressed, powers) == P.position(element, index, compressed, powers)
    for element, index in (("TauG1", 2 ** 29 - 1), ("TauG2", 2 ** 28), ("BetaG2", 1), ("GammaG2", 0), ("AlphaG1", -1)):
        with pytest.raises(ValueError):
            ppot.position(element, index, True)
    assert ppot.proof_position(32) == 64 + (63 + 64) * 32 + 33 * 64
    assert ppot.proof_position(32) == P.position("BetaG2", 0, True, 32) + 64


def test_blake2b512_equals_hashlib():
    """0 and 1; 127 / 128 / 129 and 255 / 256 (a message that ends on a block boundary finalises its last full block); one
    million and three bytes behind many blocks -- from bytes, and read in place from a read-only memoryview"""
    from manta_rs_amd import api
    data = random.Random(12).randbytes(1_000_003)
    for n in (0, 1, 127, 128, 129, 255, 256, 1_000_003):
        want = hashlib.blake2b(data[:n], digest_size=64).digest()
        assert api.blake2b512(data[:n]) == want, n
        assert api.blake2b512(memoryview(data)[:n]) == want, n
    assert api.blake2b512(b"abc").hex() == (  # RFC 7693 appendix A
        "ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d17d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923")


def test_arguments_answered_before_device_work():
    """Bn254 only, group 1 or 2, no null buffer with n > 0"""
    import ctypes
    from manta_rs_amd import api
    buf = (ctypes.c_uint8 * 128)()
    out = (ctypes.c_uint64 * 16)()
    n1 = ctypes.c_size_t(1)
    dec, enc = api.LIB.mg_ppot_points_decode, api.LIB.mg_ppot_points_encode
    assert dec(api.BLS12_381, 1, buf, n1, 1, 1, out, None, None) == INVALID
    assert dec(api.BN254, 3, buf, n1, 1, 1, out, None, None) == INVALID
    assert dec(api.BN254, 1, None, n1, 1, 1, out, None, None) == INVALID
    assert dec(api.BN254, 1, buf, n1, 1, 1, None, None, None) == INVALID
    assert enc(api.BLS12_381, 2, out, n1, 0, buf) == INVALID
    assert enc(api.BN254, 0, out, n1, 0, buf) == INVALID
    assert enc(api.BN254, 2, None, n1, 0, buf) == INVALID
    assert enc(api.BN254, 2, out, n1, 0, None) == INVALID
    assert api.LIB.mg_blake2b512(None, n1, buf) == INVALID and api.LIB.mg_blake2b512(buf, n1, None) == INVALID
    assert api.ppot_point_bytes(1, True) == 32 and api.ppot_point_bytes(1, False) == 64
    assert api.ppot_point_bytes(2, True) == 64 and api.ppot_point_bytes(2, False) == 128
    with pytest.raises(ValueError):
        api.ppot_points_decode(1, bytes(33), True)
