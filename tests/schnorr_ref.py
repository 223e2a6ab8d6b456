"""A pure-Python restatement of manta-pay's Schnorr authorization signature, for the tests of mg_schnorr_challenges /
mg_signatures_verify / mg_signatures_sign (tests/test_schnorr_host.py, tests/test_gpu_schnorr.py). `hashlib.blake2s` for the hash
and the affine curve of tests/edwards_ref.py, so nothing here shares a formula with the device's extended coordinates or a line
with the library's Blake2s.

  scheme     manta-crypto/src/signature/mod.rs `schnorr`: R = k G, s = k + sk h, verify s G == R + h pk
  challenge  manta-pay/src/config/utxo.rs `SchnorrHashFunction`: Blake2s-256(tag | enc(pk) | enc(R) | message) read
             little-endian and reduced mod l (`from_le_bytes_mod_order`); enc = `affine_point_as_bytes`, the ark-ec encoding
  ledger     manta-accounting/src/transfer/utxo/protocol.rs `auth::VerifySignature::verify`: s G == R is refused first"""
import hashlib

import edwards_ref as E

R, L = E.R, E.L
TAG = b"manta-pay/1.0.0/Schnorr-hash"
OK, BAD_ENCODING, DEGENERATE, MISMATCH = 0, 1, 2, 3
MAX_QUOTIENT = ((1 << 256) - 1) // L  # of a 256-bit digest by l


def rem_mod_l(v):
    """v < 2^256 -> (v mod l, the quotient), by the six conditional subtractions of 32 l .. l the kernel runs"""
    assert 0 <= v < 1 << 256 and 32 * L < 1 << 256 <= 64 * L
    q = 0
    for s in (5, 4, 3, 2, 1, 0):
        if v >= L << s:
            v -= L << s
            q += 1 << s
    return v, q


def digest_int(pk, nonce_point, message):
    return int.from_bytes(hashlib.blake2s(TAG + E.encode(pk) + E.encode(nonce_point) + bytes(message)).digest(), "little")


def challenge(pk, nonce_point, message):
    return rem_mod_l(digest_int(pk, nonce_point, message))[0]


def sign(g, sk, k, message):
    """-> (s, R, pk)"""
    nonce_point, pk = E.mul(g, k), E.mul(g, sk)
    return (k + sk * challenge(pk, nonce_point, message)) % L, nonce_point, pk


def verify(g, pk, message, s, nonce_point):
    """the status of mantagpu.h MG_SIG_*: encoding first (s below l, coordinates below p, both points on the curve), then the
    ledger's refusal of s G == R, then the equation"""
    if s >= L or any(c >= R for c in pk + nonce_point) or not E.on_curve(pk) or not E.on_curve(nonce_point):
        return BAD_ENCODING
    sg = E.mul(g, s)
    if sg == nonce_point:
        return DEGENERATE
    return OK if sg == E.add(nonce_point, E.mul(pk, challenge(pk, nonce_point, message))) else MISMATCH
