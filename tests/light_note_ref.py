"""A pure-Python restatement of manta-pay's AES-GCM notes, its address partition and its Merkle shard function, for the tests of
mg_aes256_gcm / mg_blake2s / mg_light_notes_* / mg_outgoing_notes_* / mg_address_partitions / mg_merkle_shard_indices
(tests/test_light_note_host.py, tests/test_gpu_light_note.py). Bytes and Python integers; the key agreement is the affine curve of
tests/edwards_ref.py, the hashes are hashlib's. Nothing here follows the library's aes_gcm.h: the S-box comes from a logarithm
table of GF(2^8) and the affine map bit by bit, the cipher works on a 4 x 4 byte matrix, and GHASH is SP 800-38D's algorithm 1 on
128-bit integers.

  key        utxo.rs:907-949, 1658-1700: Blake2s-256 of the agreed point's 32-byte encoding
  cipher     manta-pay/src/crypto/encryption/aes.rs: AES-256-GCM, nonce b"random nonce", no associated data, ciphertext | tag
  light      utxo.rs:760-1031: randomness (32 bytes LE) | asset id (32) | asset value (u128, 16)
  outgoing   utxo.rs:1511-1777: asset id (32) | asset value (16)
  partition  utxo.rs:1810-1831: Blake2s, ONE-byte digest, of "manta-v1.0.0/address-partition-function" | x | y
  shard      utxo.rs:1319-1337: the same of "manta-v1.0.0/merkle-tree-shard-function" | leaf"""
import hashlib

import edwards_ref as E

R, L = E.R, E.L
NONCE = b"random nonce"
OK, BAD_TAG, BAD_VALUE, OTHER_PARTITION = 0, 1, 2, 3
U128 = 1 << 128
LIGHT_PLAIN, LIGHT_SEALED, OUTGOING_PLAIN, OUTGOING_SEALED = 80, 96, 48, 64
PARTITION_PREFIX = b"manta-v1.0.0/address-partition-function"
SHARD_PREFIX = b"manta-v1.0.0/merkle-tree-shard-function"


# ---- AES-256 (FIPS 197) -------------------------------------------------------------------------------------------------------
def _x2(b):
    return ((b << 1) ^ 0x11b) & 0xff if b & 0x80 else b << 1


def _sbox():
    exp, log = [0] * 255, [0] * 256  # powers and logarithms to the generator 3 = x + 1 of GF(2^8)*
    v = 1
    for i in range(255):
        exp[i], log[v] = v, i
        v ^= _x2(v)
    assert v == 1
    box = []
    for a in range(256):
        inv = 0 if a == 0 else exp[(255 - log[a]) % 255]
        bits = [(inv >> i) & 1 for i in range(8)]
        out = 0
        for i in range(8):  # b'_i = b_i + b_(i+4) + b_(i+5) + b_(i+6) + b_(i+7) + c_i, c = 0x63
            out |= (bits[i] ^ bits[(i + 4) % 8] ^ bits[(i + 5) % 8] ^ bits[(i + 6) % 8] ^ bits[(i + 7) % 8] ^ ((0x63 >> i) & 1)) << i
        box.append(out)
    return box


SBOX = _sbox()


def key_schedule(key):
    """32 key bytes -> 15 round keys of 16 bytes"""
    assert len(key) == 32
    w = [list(key[4 * i:4 * i + 4]) for i in range(8)]
    rc = 1
    for i in range(8, 60):
        t = list(w[i - 1])
        if i % 8 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rc
            rc = _x2(rc)
        elif i % 8 == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - 8], t)])
    return [bytes(sum(w[4 * r:4 * r + 4], [])) for r in range(15)]


def encrypt_block(round_keys, block):
    s = [b ^ k for b, k in zip(block, round_keys[0])]  # s[4 c + r]: column c, row r
    for rnd in range(1, 15):
        s = [SBOX[b] for b in s]
        s = [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]  # ShiftRows
        if rnd < 14:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                for r in range(4):
                    m.append(_x2(a[r]) ^ _x2(a[(r + 1) % 4]) ^ a[(r + 1) % 4] ^ a[(r + 2) % 4] ^ a[(r + 3) % 4])
            s = m
        s = [b ^ k for b, k in zip(s, round_keys[rnd])]
    return bytes(s)


# ---- GCM (SP 800-38D) -----------------------------------------------------------------------------------------------------------
def gf128_mul(x, y):
    """algorithm 1: blocks as integers whose most significant bit is bit 0 of the block"""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ (0xe1 << 120) if v & 1 else v >> 1
    return z


def ghash(h, data):
    y = 0
    for off in range(0, len(data), 16):
        y = gf128_mul(y ^ int.from_bytes(data[off:off + 16].ljust(16, b"\0"), "big"), h)
    return y


def _gcm(key, nonce, data):
    """-> (data xor keystream, a function ciphertext -> tag)"""
    assert len(nonce) == 12
    rk = key_schedule(key)
    h = int.from_bytes(encrypt_block(rk, bytes(16)), "big")
    stream = b"".join(encrypt_block(rk, nonce + (2 + i).to_bytes(4, "big")) for i in range((len(data) + 15) // 16))
    out = bytes(a ^ b for a, b in zip(data, stream))

    def tag(ct):
        y = gf128_mul(ghash(h, ct) ^ (8 * len(ct)), h)  # the length block: 64 zero bits of associated data, then 8 len
        return (y ^ int.from_bytes(encrypt_block(rk, nonce + b"\0\0\0\1"), "big")).to_bytes(16, "big")
    return out, tag


def gcm_encrypt(key, nonce, plaintext):
    ct, tag = _gcm(key, nonce, plaintext)
    return ct + tag(ct)


def gcm_decrypt(key, nonce, sealed):
    """-> the plaintext, or None where the tag does not verify"""
    ct, given = sealed[:-16], sealed[-16:]
    pt, tag = _gcm(key, nonce, ct)
    return pt if tag(ct) == given else None


# ---- the notes ----------------------------------------------------------------------------------------------------------------
def note_key(agreed):
    return hashlib.blake2s(E.encode(agreed)).digest()


def light_bytes(plaintext):
    rnd, aid, val = plaintext
    return rnd.to_bytes(32, "little") + aid.to_bytes(32, "little") + val.to_bytes(16, "little")


def outgoing_bytes(asset):
    return asset[0].to_bytes(32, "little") + asset[1].to_bytes(16, "little")


def _seal(agreed, fields, to_bytes):
    if fields[-1] >= U128:
        return None, BAD_VALUE
    return gcm_encrypt(note_key(agreed), NONCE, to_bytes(fields)), OK


def light_seal(agreed, plaintext):
    """agreed = the point both sides arrive at -> (note of 96 bytes or None, status)"""
    return _seal(agreed, plaintext, light_bytes)


def outgoing_seal(agreed, asset):
    return _seal(agreed, asset, outgoing_bytes)


def light_encrypt(g, recv_key, randomness, plaintext):
    """-> (epk, note of 96 bytes, status); (None, None, BAD_VALUE) for a value of 2^128 or more"""
    note, st = light_seal(E.mul(recv_key, randomness), plaintext)
    return (E.mul(g, randomness) if st == OK else None), note, st


def outgoing_encrypt(g, recv_key, randomness, asset):
    note, st = outgoing_seal(E.mul(recv_key, randomness), asset)
    return (E.mul(g, randomness) if st == OK else None), note, st


def _unseal(agreed, sealed, whole):
    """whole = the 32-byte fields in front of the 16-byte value -> (fields or None, status)"""
    pt = gcm_decrypt(note_key(agreed), NONCE, sealed)
    if pt is None:
        return None, BAD_TAG
    fields = [int.from_bytes(pt[32 * i:32 * i + 32], "little") for i in range(whole)]
    if any(f >= R for f in fields):
        return None, BAD_VALUE
    return fields + [int.from_bytes(pt[32 * whole:], "little")], OK


def light_unseal(agreed, note):
    assert len(note) == LIGHT_SEALED
    return _unseal(agreed, note, 2)


def outgoing_unseal(agreed, note):
    assert len(note) == OUTGOING_SEALED
    return _unseal(agreed, note, 1)


def light_open(viewing_key, epk, note):
    return light_unseal(E.mul(epk, viewing_key), note)


def outgoing_open(viewing_key, epk, note):
    return outgoing_unseal(E.mul(epk, viewing_key), note)


def address_partition(point):
    x, y = point
    return hashlib.blake2s(PARTITION_PREFIX + x.to_bytes(32, "little") + y.to_bytes(32, "little"), digest_size=1).digest()[0]


def merkle_shard(leaf):
    return hashlib.blake2s(SHARD_PREFIX + leaf.to_bytes(32, "little"), digest_size=1).digest()[0]
