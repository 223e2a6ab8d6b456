"""CPU tests of the embedded curve and the Poseidon note encryption (mg_edwards_*, mg_note_cipher_*, mg_notes_*): the Python
restatement the GPU tests check against (tests/edwards_ref.py) reproduces what the reference's parameter files pin down; the
committed files carry the reference's checkfile digests; mg_note_cipher_create decodes on the host; and every argument check
of the C ABI answers MG_ERROR_INVALID_ARGUMENT before any device work, so these run without a GPU."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest

import edwards_ref as E
import poseidon_ref as P
from manta_rs_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = json.load(open(os.path.join(P.PARAM_DIR, "edwards_checkfile.json")))
INVALID = 1  # MG_ERROR_INVALID_ARGUMENT
R, L = E.R, E.L


def read(name):
    return open(os.path.join(P.PARAM_DIR, name), "rb").read()


def mont_points(points):
    """[(x, y)] -> [n, 8] affine Montgomery limbs"""
    return synth.to_mont([c for p in points for c in p], R, 4).reshape(-1, 8)


def test_curve_constants():
    assert E.D == 9706598848417545097372247223557719406784115219466060233080913168975159366771
    assert pow(E.D, (R - 1) // 2, R) == R - 1  # d is a non-square: the addition law is complete
    assert E.on_curve(E.IDENTITY) and E.on_curve((0, R - 1)) and E.on_curve((1, 0)) and E.on_curve((R - 1, 0))
    assert E.add((0, R - 1), (0, R - 1)) == E.IDENTITY  # order 2
    assert E.mul((1, 0), 4) == E.IDENTITY and E.mul((1, 0), 2) == (0, R - 1)  # order 4


def test_generator_file_pins_curve_encoding_and_root_rule():
    """group-generator.dat decodes (x little-endian, bit 255 = y is the larger root) to a point on the curve of order l; the
    other root gives a point outside the subgroup; encoding it again gives the file"""
    data = read("group-generator.dat")
    assert len(data) == 32
    g, st = E.decode(data)
    assert st == E.OK and E.on_curve(g) and E.mul(g, L) == E.IDENTITY and g != E.IDENTITY
    assert E.encode(g) == data
    flipped = bytearray(data)
    flipped[31] ^= 0x80
    q, st = E.decode(bytes(flipped), checked=False)
    assert st == E.OK and q == (g[0], R - g[1]) and E.on_curve(q) and not E.in_subgroup(q)
    assert E.decode(bytes(flipped))[1] == E.NOT_IN_SUBGROUP


def test_cipher_file_layout():
    data = read("incoming-base-encryption-scheme.dat")
    assert len(data) == E.CIPHER_BYTES == 8712
    assert int.from_bytes(data[8576:8584], "little") == 4
    c = E.Cipher(data)
    assert c.perm.mds == [pow(i + 4 + j, -1, R) for i in range(4) for j in range(4)]
    assert len(c.perm.keys) == 63 * 4 and len(c.initial) == 4


@pytest.mark.parametrize("name", sorted(CHECK))
def test_parameter_fixture_digests(name):
    from manta_rs_amd import api
    data = read(name)
    assert len(data) == CHECK[name]["bytes"]
    assert api.blake3(data).hex() == CHECK[name]["blake3"]


def test_codec_model_round_trips_and_rejects():
    g = E.generator()
    rng = random.Random(5)
    for _ in range(8):
        p = E.mul(g, rng.randrange(1, L))
        for q in (p, E.neg(p)):
            assert E.decode(E.encode(q)) == (q, E.OK)
    assert E.encode(E.IDENTITY) == bytes(32) and E.decode(bytes(32)) == (E.IDENTITY, E.OK)
    assert E.decode(E.encode((0, R - 1))) == (E.IDENTITY, E.OK)  # x = 0 is the identity whatever the flag
    assert E.decode(R.to_bytes(32, "little"))[1] == E.BAD_ENCODING
    assert E.decode((1 << 254).to_bytes(32, "little"))[1] == E.BAD_ENCODING
    assert E.decode(E.encode((1, 0)))[1] == E.NOT_IN_SUBGROUP and E.decode(E.encode((1, 0)), checked=False) == ((1, 0), E.OK)
    x = next(x for x in range(2, 100) if E.y_from_x(x, False) is None)
    assert E.decode(x.to_bytes(32, "little"))[1] == E.NOT_ON_CURVE


def test_model_encrypt_decrypt_round_trip_and_tamper():
    c, g = E.Cipher.load(), E.generator()
    rng = random.Random(7)
    sk, rnd = rng.randrange(1, L), rng.randrange(1, L)
    pk = E.mul(g, sk)
    pt = [rng.randrange(R), rng.randrange(R), rng.randrange(1 << 128)]
    epk, ct, tag = E.note_encrypt(c, g, pk, rnd, pt)
    assert epk == E.mul(g, rnd) and E.mul(epk, sk) == E.mul(pk, rnd)
    assert E.note_decrypt(c, sk, epk, ct, tag) == (pt, True)
    for j in range(3):
        bad = list(ct)
        bad[j] = (bad[j] + 1) % R
        assert E.note_decrypt(c, sk, epk, bad, tag) == (None, False)
    assert E.note_decrypt(c, sk, epk, ct, (tag + 1) % R) == (None, False)
    assert E.note_decrypt(c, (sk + 1) % L, epk, ct, tag) == (None, False)
    big = [pt[0], pt[1], 1 << 128]
    epk, ct, tag = E.note_encrypt(c, g, pk, rnd, big)
    assert E.note_decrypt(c, sk, epk, ct, tag) == (None, False)  # the tag matches, the value does not fit u128


def _cipher_create(curve, data, gen):
    from manta_rs_amd import api
    h = ctypes.c_void_p()
    g = np.ascontiguousarray(gen, dtype=np.uint64)
    rc = api.LIB.mg_note_cipher_create(curve, data, api._sz(len(data)), api._p(g), ctypes.byref(h))
    return rc, h


def test_note_cipher_create_accepts_the_production_file_and_rejects_malformed_ones():
    from manta_rs_amd import api
    data = read("incoming-base-encryption-scheme.dat")
    g = mont_points([E.generator()])[0]
    rc, h = _cipher_create(0, data, g)
    assert rc == 0 and h.value
    api.LIB.mg_note_cipher_destroy(h)
    for bad in (data[:-32], data[:-1], data + bytes(32)):  # truncated, one byte short, too long
        rc, h = _cipher_create(0, bad, g)
        assert rc == INVALID and not h.value
    for pos in (0, 100, 63 * 4 + 15):  # an element equal to p: a round key, another, the last MDS entry
        bad = bytearray(data)
        bad[32 * pos:32 * pos + 32] = R.to_bytes(32, "little")
        rc, h = _cipher_create(0, bytes(bad), g)
        assert rc == INVALID and not h.value, pos
    bad = bytearray(data)
    bad[-32:] = R.to_bytes(32, "little")  # the last word of the initial state
    assert _cipher_create(0, bytes(bad), g)[0] == INVALID
    bad = bytearray(data)
    bad[-32:] = (R - 1).to_bytes(32, "little")  # p - 1 is canonical
    rc, h = _cipher_create(0, bytes(bad), g)
    assert rc == 0
    api.LIB.mg_note_cipher_destroy(h)
    bad = bytearray(data)
    bad[8576] = 3  # the length of the initial state
    assert _cipher_create(0, bytes(bad), g)[0] == INVALID
    assert _cipher_create(1, data, g)[0] == INVALID  # BLS12-381 has no embedded curve here
    off = mont_points([(E.generator()[0], 5)])[0]
    assert _cipher_create(0, data, off)[0] == INVALID  # a generator that is not on the curve
    with pytest.raises(api.MantaGpuError):
        api.NoteCipher(data[:-1], g)


def test_argument_checks_need_no_gpu():
    from manta_rs_amd import api
    g = mont_points([E.generator()])
    pts = np.repeat(g, 3, axis=0)
    ok_sc = api.edwards_scalars([1, 2, L - 1])
    status = []

    def invalid(call):
        with pytest.raises(api.MantaGpuError) as e:
            call()
        status.append(e.value.status)
        assert e.value.status == INVALID

    for mode, p, s in ((0, pts, api.edwards_scalars([L])), (0, pts, api.edwards_scalars([1 << 255])),
                       (1, g, api.edwards_scalars([1, L, 2])), (2, pts, api.edwards_scalars([1, 2, L + 5]))):
        invalid(lambda: api.edwards_mul(mode, p, s))  # a scalar >= l
    invalid(lambda: api.edwards_mul(0, pts, ok_sc))  # shared scalar: exactly one
    invalid(lambda: api.edwards_mul(1, pts, ok_sc))  # fixed base: exactly one
    invalid(lambda: api.edwards_mul(2, pts[:2], ok_sc))  # pairwise: as many as points
    invalid(lambda: api.edwards_mul(3, pts, ok_sc))  # no such mode
    for curve in (1, 2):  # only BN254 has this embedded curve
        invalid(lambda: api.edwards_mul(2, pts, ok_sc, curve=curve))
        invalid(lambda: api.edwards_add(pts, pts, curve=curve))
        invalid(lambda: api.edwards_check(pts, curve=curve))
        invalid(lambda: api.edwards_encode(pts, curve=curve))
        invalid(lambda: api.edwards_decode(bytes(64), curve=curve))
    assert api.LIB.mg_edwards_mul(0, 2, None, api._sz(3), api._p(ok_sc), api._sz(3), api._p(pts)) == INVALID  # NULL
    assert api.LIB.mg_edwards_add(0, api._p(pts), None, api._sz(3), api._p(pts)) == INVALID
    assert api.LIB.mg_edwards_decode(0, None, api._sz(1), 1, api._p(pts), None, None) == INVALID
    c = api.NoteCipher(read("incoming-base-encryption-scheme.dat"), g)
    pt = np.zeros((3, 3, 4), dtype=np.uint64)
    tags = np.zeros((3, 4), dtype=np.uint64)
    invalid(lambda: c.encrypt(pts, api.edwards_scalars([1, L, 2]), pt))
    invalid(lambda: c.decrypt(api.edwards_scalars([L])[0], pts, pt, tags))
    assert api.LIB.mg_notes_decrypt(None, api._p(ok_sc), api._p(pts), api._p(pt), api._p(tags), api._sz(3), api._p(pt),
                                    api._p(np.zeros(3, dtype=np.uint8)), None) == INVALID
    # n = 0 succeeds without a device
    assert api.edwards_mul(2, np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)).shape == (0, 8)
    assert api.edwards_decode(b"")[0].shape == (0, 8) and api.edwards_encode(np.zeros((0, 8), dtype=np.uint64)) == b""
    assert c.decrypt(ok_sc[0], pts[:0], pt[:0], tags[:0])[0].shape == (0, 3, 4)


def test_no_gpu_is_an_error_not_a_fallback():
    from manta_rs_amd import api
    try:
        n = api.device_count()
    except api.MantaGpuError:
        n = 0
    if n:
        return  # the GPU suite covers the compute paths
    g = mont_points([E.generator()])
    one = api.edwards_scalars([1])
    c = api.NoteCipher(read("incoming-base-encryption-scheme.dat"), g)
    pt, tags = np.zeros((1, 3, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
    for call in (lambda: api.edwards_mul(0, g, one), lambda: api.edwards_mul(1, g, one), lambda: api.edwards_mul(2, g, one),
                 lambda: api.edwards_add(g, g), lambda: api.edwards_check(g), lambda: api.edwards_encode(g),
                 lambda: api.edwards_decode(bytes(32)), lambda: c.encrypt(g, one, pt), lambda: c.decrypt(one[0], g, pt, tags)):
        with pytest.raises(api.MantaGpuError) as e:
            call()
        assert e.value.status in (2, 3)  # MG_ERROR_HIP / MG_ERROR_OUT_OF_MEMORY: the device's refusal, never a result


def test_constants_match_the_header():
    from manta_rs_amd import api
    hdr = open(os.path.join(HERE, "..", "include", "mantagpu.h")).read()
    m = re.search(r"#define MG_EDWARDS_CHUNK \(1u << (\d+)\)", hdr)
    assert m and api.EDWARDS_CHUNK == 1 << int(m.group(1))
    for name, val in (("MG_EDWARDS_MUL_SHARED_SCALAR", api.EDWARDS_MUL_SHARED_SCALAR), ("MG_EDWARDS_MUL_FIXED_BASE", api.EDWARDS_MUL_FIXED_BASE),
                      ("MG_EDWARDS_MUL_PAIRWISE", api.EDWARDS_MUL_PAIRWISE), ("MG_NOTE_OK", api.NOTE_OK),
                      ("MG_NOTE_BAD_TAG", api.NOTE_BAD_TAG), ("MG_NOTE_BAD_VALUE", api.NOTE_BAD_VALUE)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val
    assert api.EDWARDS_ORDER == L
