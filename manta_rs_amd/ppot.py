"""Perpetual Powers of Tau (PPoT) challenge / response files -> `ceremony.Accumulator`, every point decoded and checked on the
GPU (`mg_ppot_points_decode`) -- host mirror of manta-trusted-setup/src/groth16/ppot/serialization.rs:

    position                    :441-511   `calculate_mmap_position`: where an element of the accumulator sits in a file
    read_subaccumulator         :688-702   the first powers of every vector of a (much larger) ceremony file, checked
    write_accumulator                      the same layout written out (tests; producing a challenge file)
    read_kzg_proof              :678-684   the nine points of a response file's contribution proof, non-zero (util.rs:176-237)
    response_hash               ppot/kzg.rs:85-118   `Configuration::response`: Blake2b-512 of accumulator | challenge | the three ratio proofs (arkworks form)
    file_hash                              Blake2b-512 of a whole file: the 64-byte header of the file that answers it

A file is a 64-byte hash, then TauG1 (2P - 1 points), TauG2 (P), AlphaG1 (P), BetaG1 (P), BetaG2 (1) in the record format of
`PpotSerializer` (include/mantagpu.h); P is the CEREMONY's number of powers (2^28 for the Bn254 files),
whatever sub-accumulator is read from it. A response file is compressed and carries the proof after BetaG2.

Not built: the hash to G2 behind the proofs of knowledge (`ppot/hashing.rs`, a `rand 0.4`-compatible ChaCha sampler) -- the
ratio pairs it yields are the caller's to supply (`ceremony.Accumulator.verify_transform`); the ceremony's coordinator; and
fetching the files.
"""
from __future__ import annotations

import numpy as np

from . import api, ceremony

HASH_SIZE = 64
CEREMONY_POWERS = 1 << 28  # REQUIRED_POWER = 28 (:451)
# the reference's ElementType, in file order -> (field of ceremony.Accumulator, group)
ELEMENTS = {"TauG1": ("tau_powers_g1", 1), "TauG2": ("tau_powers_g2", 2), "AlphaG1": ("alpha_tau_powers_g1", 1),
            "BetaG1": ("beta_tau_powers_g1", 1), "BetaG2": ("beta_g2", 2)}
# the proof's points in file order (kzg.rs:314-327): three G1 ratio pairs, then the three matching points in G2
PROOF_G1 = ("tau_ratio", "alpha_ratio", "beta_ratio")
PROOF_G2 = ("tau_matching_point", "alpha_matching_point", "beta_matching_point")
VARIANTS = {api.POINT_NOT_ON_CURVE: "NotOnCurve", api.POINT_NOT_IN_SUBGROUP: "NotInSubgroup"}


class PpotDecodeError(ValueError):
    """a record of a PPoT file was rejected: field of the accumulator (or name of the proof's element), index in it, and the
    reference's `PointDeserializeError` variant: ExpectedUncompressed, PointAtInfinity, NotOnCurve or NotInSubgroup"""

    def __init__(self, field, index, variant):
        super().__init__(f"{field}[{index}]: {variant}")
        self.field, self.index, self.variant = field, index, variant


def _counts(element, ceremony_powers):
    return 2 * ceremony_powers - 1 if element == "TauG1" else 1 if element == "BetaG2" else ceremony_powers


def position(element, index, compressed, ceremony_powers=CEREMONY_POWERS) -> int:
    """:441-511 `calculate_mmap_position`: the byte offset of point `index` of `element` (a key of ELEMENTS) in a file of a
    ceremony with `ceremony_powers` powers in G2."""
    if element not in ELEMENTS:
        raise ValueError(f"element {element!r} is none of {tuple(ELEMENTS)}")
    if not 0 <= index < _counts(element, ceremony_powers):
        raise ValueError(f"{element} has no point {index} in a ceremony of {ceremony_powers} powers")
    pos = HASH_SIZE
    for e, (_, g) in ELEMENTS.items():
        if e == element:
            return pos + index * api.ppot_point_bytes(g, compressed)
        pos += _counts(e, ceremony_powers) * api.ppot_point_bytes(g, compressed)


def _copy_out(buf, groups):
    """groups = lists of byte ranges (start, stop) of buf -> one bytes object per list, its ranges joined. The ranges are
    sliced from a memoryview of buf (an object that is no buffer itself is sliced as it is), so nothing but them is read or
    copied, and every view is released before this returns: one kept alive, by the traceback of a later exception say, would
    make the caller's `mmap.close()` fail with BufferError and mask that exception."""
    try:
        views = [memoryview(buf)]
    except TypeError:
        views = [buf]
    try:
        out = []
        for ranges in groups:
            first = len(views)
            views.extend(views[0][a:b] for a, b in ranges)
            out.append(b"".join(views[first:]))
        return out
    finally:
        for v in reversed(views):
            if isinstance(v, memoryview):
                v.release()


def _first_error(field, st, records, first, nb, compressed):
    """the field's first encoding error, else its first curve or subgroup error (the reference parses a whole field before
    it checks it); the two encoding errors are told apart by bit 7 of the record's first byte. st: the field's statuses;
    its records start at record `first` of `records`. Exact for uncompressed files. In a compressed file the reference meets
    a root that does not exist (`NotOnCurve`) while it parses, in record order together with `PointAtInfinity`, and defers
    only the subgroup test (:592-616): there an earlier NotOnCurve would come before a later PointAtInfinity of the same
    field, where this rule names the PointAtInfinity."""
    bad = np.flatnonzero(st == api.POINT_BAD_ENCODING)
    if bad.size:
        i = int(bad[0])
        bit7 = records[(first + i) * nb] & 0x80
        raise PpotDecodeError(field, i, "ExpectedUncompressed" if bit7 and not compressed else "PointAtInfinity")
    bad = np.flatnonzero(st)
    if bad.size:
        raise PpotDecodeError(field, int(bad[0]), VARIANTS[int(st[bad[0]])])


def read_subaccumulator(buf, g2_powers, compressed, ceremony_powers=CEREMONY_POWERS) -> ceremony.Accumulator:
    """:688-702 `read_subaccumulator`: the first 2 g2_powers - 1 TauG1 points, the first g2_powers of TauG2, AlphaG1 and BetaG1,
    and BetaG2, every point checked (curve and subgroup) on the GPU -- all G1 spans in one batch, all G2 spans in another.
    buf: the file as any buffer (an `mmap` of a 100 GB challenge is the usual one), or an object with len() and slices that
    are buffers; only the five spans are ever touched, and nothing else of it is copied. A rejected point raises
    PpotDecodeError: fields in reading order; within a field the first encoding error, else the first curve or subgroup
    error. A buffer shorter than the ceremony's layout is a ValueError."""
    if not 1 <= g2_powers <= ceremony_powers:
        raise ValueError(f"{g2_powers} powers cannot be read from a ceremony of {ceremony_powers}")
    end = position("BetaG2", 0, compressed, ceremony_powers) + api.ppot_point_bytes(2, compressed)
    if len(buf) < end:
        raise ValueError(f"a file of a ceremony of {ceremony_powers} powers has at least {end} bytes, not {len(buf)}")
    counts = {e: _counts(e, g2_powers) for e in ELEMENTS}
    groups = {g: [e for e, (_, gg) in ELEMENTS.items() if gg == g] for g in (1, 2)}

    def span(e):
        start = position(e, 0, compressed, ceremony_powers)
        return start, start + counts[e] * api.ppot_point_bytes(ELEMENTS[e][1], compressed)

    joined = dict(zip((1, 2), _copy_out(buf, [[span(e) for e in groups[g]] for g in (1, 2)])))
    decoded = {}
    for g in (1, 2):
        pts, st = api.ppot_points_decode(g, joined[g], compressed, checked=True)
        o = 0
        for e in groups[g]:
            decoded[e] = (pts[o:o + counts[e]], st[o:o + counts[e]], o)
            o += counts[e]
    for e, (field, g) in ELEMENTS.items():
        _, st, o = decoded[e]
        _first_error(field, st, joined[g], o, api.ppot_point_bytes(g, compressed), compressed)
    return ceremony.Accumulator(api.BN254, *(decoded[e][0] for e in ELEMENTS))


def write_accumulator(acc, header64, compressed) -> bytes:
    """a PPoT file of a ceremony of exactly `acc`'s size: header64 | every vector in file order, encoded on the GPU"""
    header64 = bytes(header64)
    n2 = acc.tau_powers_g2.shape[0]
    if len(header64) != HASH_SIZE:
        raise ValueError(f"the header is a {HASH_SIZE}-byte hash, not {len(header64)} bytes")
    if acc.curve != api.BN254 or acc.tau_powers_g1.shape[0] != 2 * n2 - 1 or acc.alpha_tau_powers_g1.shape[0] != n2 \
            or acc.beta_tau_powers_g1.shape[0] != n2:
        raise ValueError("a PPoT file holds a Bn254 accumulator of 2P - 1 / P / P / P / 1 points")
    return header64 + b"".join(api.ppot_points_encode(g, getattr(acc, f), compressed) for f, g in ELEMENTS.values())


def proof_position(ceremony_powers=CEREMONY_POWERS) -> int:
    """:679-681: the proof follows the compressed accumulator of a response file"""
    g1_powers, g2_powers = 2 * ceremony_powers - 1, ceremony_powers
    return 64 + (g1_powers + 2 * g2_powers) * 32 + (g2_powers + 1) * 64


def read_kzg_proof(buf, ceremony_powers=CEREMONY_POWERS) -> dict:
    """:678-684 `read_kzg_proof`: the contribution proof of a response file -- six G1 and three G2 uncompressed records: the
    ratio pairs of tau, alpha, beta, then their matching points -- decoded checked on the GPU. Returns {"tau_ratio": [2, 8],
    "alpha_ratio", "beta_ratio", "tau_matching_point": [16], "alpha_matching_point", "beta_matching_point"} (affine Montgomery
    limbs). Every element is `NonZero` (util.rs:176-237): infinity is a ValueError naming it, like a file too short; a rejected
    record raises PpotDecodeError."""
    pos = proof_position(ceremony_powers)
    n1, n2 = 6 * api.ppot_point_bytes(1, False), 3 * api.ppot_point_bytes(2, False)
    if len(buf) < pos + n1 + n2:
        raise ValueError(f"a response of a ceremony of {ceremony_powers} powers has at least {pos + n1 + n2} bytes, not {len(buf)}")
    g1_records, g2_records = _copy_out(buf, [[(pos, pos + n1)], [(pos + n1, pos + n1 + n2)]])
    g1, st1 = api.ppot_points_decode(1, g1_records, False, checked=True)
    g2, st2 = api.ppot_points_decode(2, g2_records, False, checked=True)
    out = {}
    for k, name in enumerate(PROOF_G1):
        _first_error(name, st1[2 * k:2 * k + 2], g1_records, 2 * k, 64, False)
        out[name] = g1[2 * k:2 * k + 2]
    for k, name in enumerate(PROOF_G2):
        _first_error(name, st2[k:k + 1], g2_records, k, 128, False)
        out[name] = g2[k]
    for name, pts in out.items():
        if not np.atleast_2d(pts).any(axis=1).all():
            raise ValueError(f"{name}: the point at infinity in a contribution proof")
    return out


def response_hash(acc, challenge64, proof) -> bytes:
    """ppot/kzg.rs:85-118 `Configuration::response`: Blake2b-512 over every accumulator point in arkworks uncompressed form in
    field order (`acc.encode(compressed=False)`, on the GPU), the 64-byte challenge, and then `proof.tau.serialize`,
    `proof.alpha.serialize`, `proof.beta.serialize`. Those are NOT `Proof::serialize` (kzg.rs:288-296, PPoT records, ratios
    before matching points): each is a `RatioProof`, whose serializer is derived (manta-crypto/src/arkworks/ratio.rs:50-63), so
    it is arkworks' own -- ratio.0, ratio.1, matching_point in arkworks COMPRESSED form, proof by proof: tau (G1, G1, G2),
    alpha (G1, G1, G2), beta (G1, G1, G2). proof: as `read_kzg_proof` returns it."""
    challenge64 = bytes(challenge64)
    if len(challenge64) != HASH_SIZE:
        raise ValueError(f"the challenge is a {HASH_SIZE}-byte hash, not {len(challenge64)} bytes")
    parts = [acc.encode(compressed=False), challenge64]
    for ratio, matching in zip(PROOF_G1, PROOF_G2):
        parts.append(api.points_encode(api.BN254, 1, np.asarray(proof[ratio], dtype=np.uint64).reshape(2, -1), True))
        parts.append(api.points_encode(api.BN254, 2, np.asarray(proof[matching], dtype=np.uint64).reshape(1, -1), True))
    return api.blake2b512(b"".join(parts))


def file_hash(buf) -> bytes:
    """Blake2b-512 of a whole file, read in place: a response's header must equal this hash of the challenge it answers"""
    return api.blake2b512(buf)
