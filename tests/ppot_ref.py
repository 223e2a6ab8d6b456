"""Plain-Python restatement of the Perpetual Powers of Tau point format (`PpotSerializer`,
manta-trusted-setup/src/groth16/ppot/serialization.rs:52-379) and file layout (`calculate_mmap_position`, :441-511): what
tests/test_gpu_ppot_codec.py and test_gpu_ppot_file.py check the GPU codec against.

encode lays the bytes out from the integers of the Montgomery limbs. decode does NOT parse points itself: it translates a
PPoT record into the arkworks encoding of the same point (each element reduced mod q here, re-emitted little-endian with the
arkworks flag byte -- the "greatest" bit carries over unchanged) and asks the CPU oracle (`oracle_lib.deserialize`, `on_curve`,
`g_mul` by r), so the yardstick rests on the oracle and not on the code under test."""
import numpy as np

import oracle_lib as O
from manta_rs_amd import synth

CURVE = 0  # Bn254: the ceremony's curve
Q = synth.FQ_MODULUS[CURVE]
R = synth.FR_MODULUS[CURVE]
FB = 32
OK, BAD, OFF, SUB = 0, 1, 2, 3


def point_bytes(group, compressed):
    return FB * group * (1 if compressed else 2)


def coords(group, p):
    """affine Montgomery limbs -> (x, y), each a list of `group` integers, c0 first"""
    v = synth.from_mont(np.asarray(p, dtype=np.uint64).reshape(2 * group, 4), Q)
    return v[:group], v[group:]


def is_greatest(y):
    """y > -y in the arkworks order: c1 decides, c0 where c1 = 0 (c1 = -c1 only then)"""
    for c in reversed(y):
        if c:
            return c > Q - c
    return False


def encode(group, p, compressed):
    """:244-379: big-endian elements, Fq2 c1 first, x then y; flags in bits 7 / 6 of byte 0"""
    p = np.asarray(p, dtype=np.uint64).reshape(-1)
    out = bytearray(point_bytes(group, compressed))
    if not p.any():
        out[0] = 0x40
        return bytes(out)
    x, y = coords(group, p)
    elems = list(reversed(x)) + ([] if compressed else list(reversed(y)))
    out[:] = b"".join(int(e).to_bytes(FB, "big") for e in elems)
    if compressed and is_greatest(y):
        out[0] |= 0x80
    return bytes(out)


def encode_many(group, pts, compressed):
    return b"".join(encode(group, p, compressed) for p in pts)


def decode(group, rec, compressed, checked=True):
    """:52-242 and `curve_point_checks`: (status, affine Montgomery limbs -- zeros for infinity and for a rejected point)"""
    rec = bytes(rec)
    assert len(rec) == point_bytes(group, compressed)
    zero = np.zeros(8 * group, dtype=np.uint64)
    b0 = rec[0]
    if not compressed and b0 & 0x80:
        return BAD, zero  # ExpectedUncompressed
    if b0 & 0x40:
        rest = bytes([b0 & 0x3F]) + rec[1:]
        return (OK, zero) if not any(rest) else (BAD, zero)  # PointAtInfinity
    elems = [int.from_bytes(rec[i:i + FB], "big") for i in range(0, len(rec), FB)]
    elems[0] &= (1 << 254) - 1
    elems = [e % Q for e in elems]  # from_be_bytes_mod_order
    x = list(reversed(elems[:group]))  # c0 first, as arkworks writes it
    ark = bytearray(b"".join(e.to_bytes(FB, "little") for e in x))
    if compressed:
        if b0 & 0x80:
            ark[-1] |= 0x80
        ok, p = O.deserialize(CURVE, group, bytes(ark), True)  # get_point_from_x(x, greatest)
        if not ok:
            return OFF, zero
    else:
        y = list(reversed(elems[group:]))
        ark += b"".join(e.to_bytes(FB, "little") for e in y)
        ok, p = O.deserialize(CURVE, group, bytes(ark), False)
        assert ok
        # the point (0, 0) is not infinity here (the infinity flag is clear) and 0 != 0 + b; in the oracle's arrays zeros
        # ARE infinity, so it cannot be asked about this one
        if checked and (not p.any() or not O.on_curve(CURVE, group, p)):
            return OFF, zero
    if checked and O.g_mul(CURVE, group, p, synth.ints_to_limbs([R], 4)[0]).any():
        return SUB, zero
    return OK, p


# ---- the file layout, restated from the constants of :446-455 -----------------------------------------------------------
G1_UNCOMPRESSED_BYTE_SIZE, G2_UNCOMPRESSED_BYTE_SIZE = 64, 128
G1_COMPRESSED_BYTE_SIZE, G2_COMPRESSED_BYTE_SIZE = 32, 64
HASH_SIZE = 64


def position(element, index, compressed, tau_powers_length=1 << 28):
    g1, g2 = (G1_COMPRESSED_BYTE_SIZE, G2_COMPRESSED_BYTE_SIZE) if compressed else \
        (G1_UNCOMPRESSED_BYTE_SIZE, G2_UNCOMPRESSED_BYTE_SIZE)
    tau_powers_g1_length = (tau_powers_length << 1) - 1
    if element == "TauG1":
        assert index < tau_powers_g1_length
        return HASH_SIZE + g1 * index
    if element == "TauG2":
        assert index < tau_powers_length
        return HASH_SIZE + g1 * tau_powers_g1_length + g2 * index
    if element == "AlphaG1":
        assert index < tau_powers_length
        return HASH_SIZE + g1 * tau_powers_g1_length + g2 * tau_powers_length + g1 * index
    if element == "BetaG1":
        assert index < tau_powers_length
        return HASH_SIZE + g1 * tau_powers_g1_length + g2 * tau_powers_length + g1 * tau_powers_length + g1 * index
    assert element == "BetaG2" and index == 0
    return HASH_SIZE + g1 * tau_powers_g1_length + g2 * tau_powers_length + 2 * g1 * tau_powers_length
