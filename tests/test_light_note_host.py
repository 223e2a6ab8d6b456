"""CPU tests of the AES-GCM notes (mg_aes256_gcm, mg_blake2s, mg_light_notes_*, mg_outgoing_notes_*, mg_address_partitions,
mg_merkle_shard_indices): the library's AES-256-GCM and variable-length Blake2s -- the sources the note kernels compile --
against OpenSSL's vectors (tests/golden/aes_gcm_vectors.json), hashlib and the Python restatement of tests/light_note_ref.py;
that restatement against the same vectors; and every argument check of the six batched calls, which answer
MG_ERROR_INVALID_ARGUMENT before any device work, so these run without a GPU."""
import ctypes
import hashlib
import json
import os
import random
import re

import numpy as np
import pytest

import edwards_ref as E
import light_note_ref as N
import utxo_ref as U
from manta_rs_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = 1  # MG_ERROR_INVALID_ARGUMENT
R, L = N.R, N.L
FILES = [U.read(n) for n in U.FILES]
VECTORS = [{k: bytes.fromhex(v) for k, v in vec.items()}
           for vec in json.load(open(os.path.join(HERE, "golden", "aes_gcm_vectors.json")))["vectors"]]
LENGTHS = [0, 1, 15, 16, 17, 48, 80, 96]


def mont_points(points):
    return synth.to_mont([c for p in points for c in p], R, 4).reshape(-1, 8)


def test_fixture_covers_the_lengths_and_the_fixed_nonce():
    assert len(VECTORS) == 40 and sorted({len(v["plaintext"]) for v in VECTORS}) == LENGTHS
    assert sum(v["nonce"] == N.NONCE for v in VECTORS) == 24 and len({v["nonce"] for v in VECTORS}) == 17
    assert all(len(v["sealed"]) == len(v["plaintext"]) + 16 and len(v["key"]) == 32 for v in VECTORS)


def test_model_equals_the_fixture():
    assert N.SBOX[:4] == [0x63, 0x7c, 0x77, 0x7b] and sorted(N.SBOX) == list(range(256))  # FIPS 197 figure 7, first row
    for v in VECTORS:
        assert N.gcm_encrypt(v["key"], v["nonce"], v["plaintext"]) == v["sealed"]
        assert N.gcm_decrypt(v["key"], v["nonce"], v["sealed"]) == v["plaintext"]
    # NIST's GCM test cases 13 and 14
    assert N.gcm_encrypt(bytes(32), bytes(12), b"").hex() == "530f8afbc74536b9a963b4f1c4cb738b"
    assert N.gcm_encrypt(bytes(32), bytes(12), bytes(16)).hex() == "cea7403d4d606b6e074ec5d3baf39d18d0d1c8a799996bf0265b98b5d48ab919"


def test_aes256_gcm_equals_the_fixture_and_the_model():
    from manta_rs_amd import api
    for v in VECTORS:
        assert api.aes256_gcm_encrypt(v["key"], v["nonce"], v["plaintext"]) == v["sealed"], len(v["plaintext"])
        assert api.aes256_gcm_decrypt(v["key"], v["nonce"], v["sealed"]) == (v["plaintext"], True)
    rng = random.Random(31)
    for n in list(range(0, 40)) + [47, 48, 49, 79, 80, 81, 255, 256, 257]:  # every tail length; both sides of the two template sizes
        key, nonce, pt = rng.randbytes(32), rng.randbytes(12), rng.randbytes(n)
        sealed = api.aes256_gcm_encrypt(key, nonce, pt)
        assert sealed == N.gcm_encrypt(key, nonce, pt), n
        assert api.aes256_gcm_decrypt(key, nonce, sealed) == (pt, True), n


@pytest.mark.parametrize("n", [1, 17, 48, 80, 96])
def test_aes256_gcm_refuses_one_flipped_bit(n):
    """in the ciphertext body, in the tag and in the key: ok = 0 and the output is zeros"""
    from manta_rs_amd import api
    rng = random.Random(37 + n)
    key, pt = rng.randbytes(32), rng.randbytes(n)
    sealed = api.aes256_gcm_encrypt(key, N.NONCE, pt)
    for byte in (0, n // 2, n - 1, n, n + 7, n + 15):  # n - 1: the last of the body; n: the first of the tag
        for bit in (0, 7):
            bad = bytearray(sealed)
            bad[byte] ^= 1 << bit
            assert api.aes256_gcm_decrypt(key, N.NONCE, bytes(bad)) == (bytes(n), False), (byte, bit)
            assert N.gcm_decrypt(key, N.NONCE, bytes(bad)) is None
    for byte in (0, 16, 31):
        bad = bytearray(key)
        bad[byte] ^= 0x10
        assert api.aes256_gcm_decrypt(bytes(bad), N.NONCE, sealed) == (bytes(n), False)
    other = bytearray(N.NONCE)
    other[11] ^= 1
    assert api.aes256_gcm_decrypt(key, bytes(other), sealed) == (bytes(n), False)


def test_aes256_gcm_argument_checks():
    from manta_rs_amd import api
    lib, sz = api.LIB, api._sz
    key, nonce, buf, ok = bytes(32), bytes(12), ctypes.create_string_buffer(64), ctypes.c_int(5)
    assert lib.mg_aes256_gcm(None, nonce, b"abc", sz(3), 0, buf, None) == INVALID
    assert lib.mg_aes256_gcm(key, None, b"abc", sz(3), 0, buf, None) == INVALID
    assert lib.mg_aes256_gcm(key, nonce, None, sz(3), 0, buf, None) == INVALID
    assert lib.mg_aes256_gcm(key, nonce, b"abc", sz(3), 0, None, None) == INVALID
    assert lib.mg_aes256_gcm(key, nonce, bytes(15), sz(15), 1, buf, ctypes.byref(ok)) == INVALID  # shorter than a tag
    assert lib.mg_aes256_gcm(key, nonce, bytes(16), sz(16), 1, buf, None) == INVALID  # decrypting needs `ok`
    assert lib.mg_aes256_gcm(key, nonce, None, sz(0), 0, buf, None) == 0  # the empty message
    assert buf.raw[:16] == N.gcm_encrypt(key, nonce, b"")
    assert lib.mg_aes256_gcm(key, nonce, buf.raw[:16], sz(16), 1, None, ctypes.byref(ok)) == 0 and ok.value == 1


def test_blake2s_equals_hashlib_at_every_digest_length():
    """the 39-byte prefixes of the partition and shard functions make streams of 71 and 103 bytes: three bytes past a word"""
    from manta_rs_amd import api
    data = random.Random(41).randbytes(128)
    for k in range(1, 33):
        for n in (0, 1, 63, 64, 65, 71, 103, 128):
            assert api.blake2s(data[:n], digest_size=k) == hashlib.blake2s(data[:n], digest_size=k).digest(), (k, n)
    for n in (0, 1, 64, 103):
        assert api.blake2s(data[:n], digest_size=32) == api.blake2s(data[:n])  # = mg_blake2s256
    assert api.blake2s(b"abc", digest_size=1) == b"\x0d" and api.blake2s(b"abc")[:1] == b"\x50"  # another hash, not a prefix
    lib, sz, out = api.LIB, api._sz, ctypes.create_string_buffer(32)
    for bad in (0, 33, 1 << 40):
        assert lib.mg_blake2s(b"abc", sz(3), sz(bad), out) == INVALID
    assert lib.mg_blake2s(None, sz(1), sz(1), out) == INVALID and lib.mg_blake2s(b"abc", sz(3), sz(1), None) == INVALID
    assert lib.mg_blake2s(None, sz(0), sz(1), out) == 0 and out.raw[:1] == hashlib.blake2s(b"", digest_size=1).digest()


def test_model_notes_are_consistent():
    g = E.generator()
    rng = random.Random(43)
    vk, r = rng.randrange(1, L), rng.randrange(1, L)
    rk = E.mul(g, vk)
    pt = [rng.randrange(R), rng.randrange(R), rng.randrange(N.U128)]
    epk, note, st = N.light_encrypt(g, rk, r, pt)
    assert st == N.OK and len(note) == 96 and epk == E.mul(g, r)
    assert N.light_open(vk, epk, note) == (pt, N.OK)
    assert N.light_open((vk + 1) % L, epk, note) == (None, N.BAD_TAG)
    assert N.light_encrypt(g, rk, r, pt[:2] + [N.U128]) == (None, None, N.BAD_VALUE)
    forged = N.gcm_encrypt(N.note_key(E.mul(rk, r)), N.NONCE, N.light_bytes([pt[0], R, pt[2]]))  # id = r behind a valid tag
    assert N.light_open(vk, epk, forged) == (None, N.BAD_VALUE)
    epk, note, st = N.outgoing_encrypt(g, rk, r, pt[1:])
    assert st == N.OK and len(note) == 64 and N.outgoing_open(vk, epk, note) == (pt[1:], N.OK)
    assert len(N.PARTITION_PREFIX) == len(N.SHARD_PREFIX) == 39
    assert N.address_partition(rk) == hashlib.blake2s(N.PARTITION_PREFIX + rk[0].to_bytes(32, "little")
                                                      + rk[1].to_bytes(32, "little"), digest_size=1).digest()[0]


def test_argument_checks_need_no_gpu():
    from manta_rs_amd import api
    m = api.UtxoModel(*FILES)
    lib, p, sz = api.LIB, api._p, api._sz
    n = 3
    g = mont_points([E.generator()])[0]
    pts = np.repeat(g[None], n, axis=0)
    sc, vk = api.edwards_scalars([5, 6, 7]), api.edwards_scalars([9])[0]
    pt3, pt2, leaves = (np.zeros((n, w), dtype=np.uint64) for w in (12, 8, 4))
    ct96, ct64 = np.zeros((n, 96), dtype=np.uint8), np.zeros((n, 64), dtype=np.uint8)
    part, st, ok, out1 = (np.zeros(n, dtype=np.uint8) for _ in range(4))
    epk = np.zeros((n, 8), dtype=np.uint64)
    tried = ctypes.c_size_t(7)

    def partitions(h=m._h, rk=p(pts), n=n, out=p(out1)):
        return lib.mg_address_partitions(h, rk, sz(n), out)

    def shards(curve=api.BN254, lv=p(leaves), n=n, out=p(out1)):
        return lib.mg_merkle_shard_indices(curve, lv, sz(n), out)

    def light_enc(h=m._h, rk=p(pts), r=p(sc), pt=p(pt3), n=n, epk=p(epk), ct=p(ct96), status=p(st)):
        return lib.mg_light_notes_encrypt(h, rk, r, pt, sz(n), epk, ct, status)

    def light_open(h=m._h, vk=p(vk), ep=p(pts), ct=p(ct96), parts=p(part), n=n, pt=p(pt3), ok=p(ok), status=p(st)):
        return lib.mg_light_notes_open(h, vk, ep, ct, parts, sz(n), pt, ok, status, ctypes.byref(tried))

    def out_enc(h=m._h, rk=p(g), r=p(sc), a=p(pt2), n=n, epk=p(epk), ct=p(ct64), status=p(st)):
        return lib.mg_outgoing_notes_encrypt(h, rk, r, a, sz(n), epk, ct, status)

    def out_open(h=m._h, vk=p(vk), ep=p(pts), ct=p(ct64), n=n, a=p(pt2), ok=p(ok), status=p(st)):
        return lib.mg_outgoing_notes_open(h, vk, ep, ct, sz(n), a, ok, status)

    # a NULL model or required array (light_enc's epk, the opens' status and light_open's partitions may be NULL: those reach
    # the device and are for the GPU suite)
    for call, names in ((partitions, ("h", "rk", "out")), (shards, ("lv", "out")), (light_enc, ("h", "rk", "r", "pt", "ct", "status")),
                        (light_open, ("h", "vk", "ep", "ct", "pt", "ok")), (out_enc, ("h", "rk", "r", "a", "epk", "ct", "status")),
                        (out_open, ("h", "vk", "ep", "ct", "a", "ok"))):
        for name in names:
            assert call(**{name: None}) == INVALID, (call.__name__, name)
        assert call(n=0) == 0, call.__name__  # n = 0 succeeds without a device
        for wraps in ((1 << 64) // 96, (1 << 64) - 1):  # n x 96 bytes would wrap a size_t
            assert call(n=wraps) == INVALID, (call.__name__, wraps)
    assert tried.value == 0  # light_open(n=0) reported no lane tried
    assert lib.mg_address_partitions(m._h, None, sz(0), None) == 0 and lib.mg_merkle_shard_indices(api.BN254, None, sz(0), None) == 0
    assert lib.mg_light_notes_encrypt(m._h, None, None, None, sz(0), None, None, None) == 0
    assert lib.mg_light_notes_open(m._h, p(vk), None, None, None, sz(0), None, None, None, None) == 0
    assert lib.mg_outgoing_notes_encrypt(m._h, p(g), None, None, sz(0), None, None, None) == 0
    assert lib.mg_outgoing_notes_open(m._h, p(vk), None, None, sz(0), None, None, None) == 0
    # the other curve
    assert shards(curve=api.BLS12_381) == INVALID and shards(curve=api.BLS12_381, n=0) == INVALID
    # a randomness or a viewing key of l or more
    for bad in (L, L + 1, (1 << 256) - 1):
        for i in range(n):
            vals = [5, 6, 7]
            vals[i] = bad
            assert light_enc(r=p(api.edwards_scalars(vals))) == INVALID and out_enc(r=p(api.edwards_scalars(vals))) == INVALID
        big = api.edwards_scalars([bad])[0]
        assert light_open(vk=p(big)) == INVALID and out_open(vk=p(big)) == INVALID
        assert light_open(vk=p(big), n=0) == INVALID
    # the outgoing receiving key: off the curve, or a coordinate that is not reduced
    off = g.copy()
    off[4] ^= np.uint64(1)
    assert out_enc(rk=p(off)) == INVALID and out_enc(rk=p(off), n=0) == INVALID
    assert out_enc(rk=p(np.full(8, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))) == INVALID
    # the wrappers refuse the same through the exception, and pass n = 0 through
    for call in (lambda: m.light_encrypt(pts, api.edwards_scalars([L, 1, 1]), pt3), lambda: m.light_open(api.edwards_scalars([L])[0], pts, ct96),
                 lambda: m.outgoing_encrypt(off, sc, pt2), lambda: m.outgoing_open(api.edwards_scalars([L])[0], pts, ct64),
                 lambda: api.merkle_shard_indices(leaves, curve=api.BLS12_381)):
        with pytest.raises(api.MantaGpuError) as e:
            call()
        assert e.value.status == INVALID
    for call in (lambda: m.light_encrypt(pts, sc[:2], pt3), lambda: m.light_open(vk, pts, ct96[:2]),
                 lambda: m.light_open(vk, pts, ct96, partitions=part[:2]), lambda: m.outgoing_encrypt(pts, sc, pt2),
                 lambda: m.outgoing_open(vk, pts[:2], ct64)):
        with pytest.raises(ValueError):
            call()
    e0, c0, s0 = m.light_encrypt(pts[:0], sc[:0], pt3[:0])
    p0, k0, t0, tr0 = m.light_open(vk, pts[:0], ct96[:0], partitions=part[:0])
    assert e0.shape == (0, 8) and c0.shape == (0, 96) and s0.shape == (0,) and p0.shape == (0, 3, 4) and k0.shape == (0,) and tr0 == 0
    assert m.address_partitions(pts[:0]).shape == (0,) and api.merkle_shard_indices(leaves[:0]).shape == (0,)
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
    for call in (lambda: m.address_partitions(g), lambda: api.merkle_shard_indices(np.zeros((1, 4), dtype=np.uint64)),
                 lambda: m.light_encrypt(g, one, np.zeros((1, 12), dtype=np.uint64)),
                 lambda: m.light_open(one[0], g, np.zeros((1, 96), dtype=np.uint8)),
                 lambda: m.outgoing_encrypt(g[0], one, np.zeros((1, 8), dtype=np.uint64)),
                 lambda: m.outgoing_open(one[0], g, np.zeros((1, 64), dtype=np.uint8))):
        with pytest.raises(api.MantaGpuError) as e:
            call()
        assert e.value.status in (2, 3)  # MG_ERROR_HIP / MG_ERROR_OUT_OF_MEMORY: the device's refusal, never a result


def test_constants_match_the_header():
    from manta_rs_amd import api
    hdr = open(os.path.join(HERE, "..", "include", "mantagpu.h")).read()
    for name, val, ref in (("MG_NOTE_OK", api.NOTE_OK, N.OK), ("MG_NOTE_BAD_TAG", api.NOTE_BAD_TAG, N.BAD_TAG),
                           ("MG_NOTE_BAD_VALUE", api.NOTE_BAD_VALUE, N.BAD_VALUE),
                           ("MG_NOTE_OTHER_PARTITION", api.NOTE_OTHER_PARTITION, N.OTHER_PARTITION),
                           ("MG_LIGHT_NOTE_BYTES", api.LIGHT_NOTE_BYTES, N.LIGHT_SEALED),
                           ("MG_OUTGOING_NOTE_BYTES", api.OUTGOING_NOTE_BYTES, N.OUTGOING_SEALED)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val == ref
