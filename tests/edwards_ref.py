"""A pure-Python restatement of manta-pay's embedded curve and of its Poseidon note encryption, for the tests of
mg_edwards_* / mg_note_cipher_* / mg_notes_* (tests/test_edwards_host.py, tests/test_gpu_edwards.py). Plain integers, canonical
(not Montgomery); affine formulas with one inversion per operation, so nothing here shares a formula with the device's
extended coordinates.

  curve     ed_on_bn254 (manta-pay/src/config/mod.rs: Group = EdwardsProjective): a x^2 + y^2 = 1 + d x^2 y^2 over BN254 Fr,
            a = 1, d = 168696 / 168700, cofactor 8, prime subgroup order L
  codec     ark-ec 0.3 twisted Edwards: x little-endian, bit 255 set iff y > -y as integers; x = 0 is the identity
  cipher    FixedDuplexer<1, Poseidon3> (manta-pay/src/crypto/poseidon/encryption.rs, manta-crypto/src/permutation/duplex.rs,
            sponge.rs:83-90 absorb = write then permute): state <- initial state; the setup blocks are the key (x, y, 0) and
            -- padded_chunks_with (manta-util/src/vec.rs:76-93) always emits its remainder chunk -- one all-zero block for the
            empty header, each added to words 1..3 and followed by a permutation; the plaintext block is added to words 1..3,
            which are the ciphertext, one more permutation, tag = word 1"""
import os

import poseidon_ref as P

R = P.R_BN254  # the base field of the embedded curve
A = 1
D = 168696 * pow(168700, -1, R) % R
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
COFACTOR = 8
IDENTITY = (0, 1)
CIPHER_WIDTH, CIPHER_FULL, CIPHER_PARTIAL = 4, 8, 55
CIPHER_BYTES = 32 * ((CIPHER_FULL + CIPHER_PARTIAL) * 4 + 16) + 8 + 4 * 32


def on_curve(p):
    x, y = p
    return (A * x * x + y * y - 1 - D * x * x * y * y) % R == 0


def add(p, q):
    (x1, y1), (x2, y2) = p, q
    k = D * x1 * x2 * y1 * y2 % R
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, R) % R, (y1 * y2 - A * x1 * x2) * pow(1 - k, -1, R) % R)


def neg(p):
    return (-p[0] % R, p[1])


def mul(p, k):
    acc = IDENTITY
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, p)
    return acc


def in_subgroup(p):
    return mul(p, L) == IDENTITY


def sqrt(a):
    """a square root mod R (Tonelli-Shanks, R - 1 = 2^28 odd), or None"""
    a %= R
    if a == 0:
        return 0
    if pow(a, (R - 1) // 2, R) != 1:
        return None
    s, t = 28, (R - 1) >> 28
    z = pow(5, t, R)
    x, b, m = pow(a, (t + 1) // 2, R), pow(a, t, R), s
    while b != 1:
        i, c = 0, b
        while c != 1:
            c, i = c * c % R, i + 1
        g = pow(z, 1 << (m - i - 1), R)
        x, b, z, m = x * g % R, b * g * g % R, g * g % R, i
    return x


def y_from_x(x, greatest):
    """ark-ec 0.3 get_point_from_x: y^2 = (a x^2 - 1) / (d x^2 - 1), the larger root iff `greatest`"""
    x2 = x * x % R
    y = sqrt((A * x2 - 1) * pow(D * x2 - 1, -1, R))
    if y is None:
        return None
    ny = -y % R
    return y if (y < ny) != greatest else ny


OK, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = 0, 1, 2, 3


def decode(b, checked=True):
    """32 bytes -> (point or None, status)"""
    v = int.from_bytes(b, "little")
    greatest, x = bool(v >> 255), v & ((1 << 255) - 1)
    if x >= R:
        return None, BAD_ENCODING
    if x == 0:
        return IDENTITY, OK
    y = y_from_x(x, greatest)
    if y is None:
        return None, NOT_ON_CURVE
    if checked and not in_subgroup((x, y)):
        return None, NOT_IN_SUBGROUP
    return (x, y), OK


def encode(p):
    if p == IDENTITY:
        return bytes(32)
    x, y = p
    return (x | (int(y > -y % R) << 255)).to_bytes(32, "little")


def check(p):
    if p[0] >= R or p[1] >= R:
        return BAD_ENCODING
    if not on_curve(p):
        return NOT_ON_CURVE
    return OK if in_subgroup(p) else NOT_IN_SUBGROUP


def generator():
    data = open(os.path.join(P.PARAM_DIR, "group-generator.dat"), "rb").read()
    p, st = decode(data)
    assert st == OK
    return p


class Cipher:
    """`IncomingBaseEncryptionScheme` decoded from incoming-base-encryption-scheme.dat: the width-4 permutation (keys | MDS, no
    domain tag), then `FixedEncryption::initial_state` as a u64 length (4) and four elements"""

    def __init__(self, data):
        assert len(data) == CIPHER_BYTES
        nperm = CIPHER_BYTES - 8 - 4 * 32
        self.perm = P.Params.decode(R, data[:nperm] + bytes(32), CIPHER_WIDTH, CIPHER_FULL, CIPHER_PARTIAL)
        assert int.from_bytes(data[nperm:nperm + 8], "little") == 4
        self.initial = [int.from_bytes(data[nperm + 8 + 32 * i:nperm + 40 + 32 * i], "little") for i in range(4)]
        assert all(x < R for x in self.perm.keys + self.perm.mds + self.initial)

    @classmethod
    def load(cls):
        return cls(open(os.path.join(P.PARAM_DIR, "incoming-base-encryption-scheme.dat"), "rb").read())

    def _setup(self, key):
        st = list(self.initial)
        for block in ((key[0], key[1], 0), (0, 0, 0)):  # the key, then the empty header's zero block
            st = self.perm.permute([st[0]] + [(s + b) % R for s, b in zip(st[1:], block)])
        return st

    def encrypt(self, key, plaintext):
        """key = the agreed point (x, y); plaintext = 3 elements -> (ciphertext [3], tag)"""
        st = self._setup(key)
        ct = [(s + m) % R for s, m in zip(st[1:], plaintext)]
        return ct, self.perm.permute([st[0]] + ct)[1]

    def decrypt(self, key, ciphertext, tag):
        """-> (plaintext [3] or None, ok): ok iff the tag matches and the value word is below 2^128 (`try_into_u128`)"""
        st = self._setup(key)
        pt = [(c - s) % R for c, s in zip(ciphertext, st[1:])]
        ok = self.perm.permute([st[0]] + list(ciphertext))[1] == tag and pt[2] < (1 << 128)
        return (pt if ok else None), ok


def note_encrypt(cipher, g, recv_key, randomness, plaintext):
    """`Hybrid` encryption: epk = G * randomness, key = recv_key * randomness -> (epk, ciphertext, tag)"""
    ct, tag = cipher.encrypt(mul(recv_key, randomness), plaintext)
    return mul(g, randomness), ct, tag


def note_decrypt(cipher, viewing_key, epk, ciphertext, tag):
    return cipher.decrypt(mul(epk, viewing_key), ciphertext, tag)
