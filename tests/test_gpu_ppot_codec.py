"""GPU codec of the Perpetual Powers of Tau point records (mg_ppot_points_decode / mg_ppot_points_encode, Bn254 G1 / G2,
compressed and uncompressed): big-endian elements, Fq2 c1 first, flags in byte 0, coordinates reduced mod q. Yardstick:
tests/ppot_ref.py, whose decoder rests on the CPU oracle's deserialize / on_curve / g_mul."""
import ctypes
import functools

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
import ppot_ref as P
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu
GROUPS = [1, 2]
CHUNK = 1 << 16  # points on the device per launch (mantagpu.h)
OK, BAD, OFF, SUB = 0, 1, 2, 3
Q = P.Q


@functools.lru_cache(maxsize=None)
def _base(group):
    """1000 random points with an infinity inside, and their reference records in both forms: computed once, never changed"""
    pts = H.random_points(0, group, 1000, seed=700 + group)
    pts[333] = 0
    pts.setflags(write=False)
    return pts, {c: [P.encode(group, p, c) for p in pts] for c in (True, False)}


def _decode_raw(gpu, group, data, compressed, checked):
    nb = P.point_bytes(group, compressed)
    n = len(data) // nb
    out = np.zeros((n, 8 * group), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    n_bad = ctypes.c_size_t(12345)
    rc = gpu.LIB.mg_ppot_points_decode(0, group, bytes(data), ctypes.c_size_t(n), int(compressed), int(checked),
                                       out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.byref(n_bad))
    assert rc == 0
    return out, st, n_bad.value


@pytest.mark.parametrize("group", GROUPS)
def test_round_trip_every_size(gpu, group):
    """encode == ppot_ref byte for byte; decode (checked) gives the limbs back with every status 0 -- for n = 0, 1, 63, 64,
    65, 1000 and one n above the staging chunk, both forms, an infinity inside the batch"""
    base, recs = _base(group)
    for compressed in (True, False):
        want = b"".join(recs[compressed])
        nb = gpu.ppot_point_bytes(group, compressed)
        assert nb == P.point_bytes(group, compressed)
        for n in (0, 1, 63, 64, 65, 1000):
            enc = gpu.ppot_points_encode(group, base[:n], compressed)
            assert enc == want[:n * nb], (n, compressed)
            pts, st = gpu.ppot_points_decode(group, enc, compressed)
            assert pts.shape == (n, 8 * group) and st.shape == (n,)
            assert (st == OK).all(), (n, compressed, np.flatnonzero(st)[:5])
            assert (pts == base[:n]).all(), (n, compressed)
        big = CHUNK + 37
        reps = -(-big // 1000)
        pts_big = np.tile(base, (reps, 1))[:big]
        enc = gpu.ppot_points_encode(group, pts_big, compressed)
        assert enc == (want * reps)[:big * nb]
        pts, st = gpu.ppot_points_decode(group, memoryview(enc), compressed)
        assert (st == OK).all() and (pts == pts_big).all()


def _bump_last_element(rec):
    """the record with its last element (y, or y.c0) replaced by that + 1 mod q"""
    b = bytearray(rec)
    b[-32:] = ((int.from_bytes(b[-32:], "big") + 1) % Q).to_bytes(32, "big")
    return bytes(b)


def _no_root_x(group, rng):
    """a compressed record whose x^3 + b has no square root"""
    while True:
        rec = b"".join((rng.field(Q) & ((1 << 254) - 1) if i == 0 else rng.field(Q)).to_bytes(32, "big") for i in range(group))
        if P.decode(group, rec, True)[0] == OFF:
            return rec


def _off_subgroup_g2(rng):
    """a G2 point on the curve outside the subgroup (found as the arkworks codec test finds it: the oracle's deserialize of a
    random x checks neither)"""
    rk = synth.ints_to_limbs([P.R], 4)[0]
    while True:
        enc = b"".join(rng.field(Q).to_bytes(32, "little") for _ in range(2))
        ok, p = O.deserialize(0, 2, enc, True)
        if ok and O.on_curve(0, 2, p) and O.g_mul(0, 2, p, rk).any():
            return p


@pytest.mark.parametrize("group", GROUPS)
def test_rejections_mixed_into_good_batches(gpu, group):
    """each rejected record sits between good points with its exact status; the good points still decode, n_bad is exact;
    the statuses are those of DESIGN section 17's table AND those ppot_ref gives"""
    base, recs = _base(group)
    rng = synth.XorShift(910 + group)
    zero = np.zeros(8 * group, dtype=np.uint64)
    for compressed in (True, False):
        enc = recs[compressed]
        nb = len(enc[0])
        cases = []  # (record, status, expected limbs)
        inf = bytearray(nb)
        inf[0] = 0x40
        cases.append((bytes(inf), OK, zero))
        for at in (nb - 1, 1):  # an infinity flag with one non-zero byte
            dirty = bytearray(inf)
            dirty[at] = 1
            cases.append((bytes(dirty), BAD, zero))
        both = bytearray(inf)
        both[0] = 0xC0
        cases.append((bytes(both), OK if compressed else BAD, zero))
        st0, p0 = P.decode(group, bytes(nb), compressed)  # all zero: not infinity
        if not compressed:
            assert st0 == OFF  # the point (0, 0)
            bit7 = bytearray(enc[5])
            bit7[0] |= 0x80
            cases.append((bytes(bit7), BAD, zero))
            cases.append((_bump_last_element(enc[6]), OFF, zero))
        else:
            cases.append((_no_root_x(group, rng), OFF, zero))
        cases.append((bytes(nb), st0, p0))
        if group == 2:  # G1 has cofactor 1: every point of its curve is in the subgroup
            cases.append((P.encode(2, _off_subgroup_g2(rng), compressed), SUB, zero))
        for rec, s, p in cases:
            got = P.decode(group, rec, compressed)
            assert got[0] == s and (got[1] == p).all(), (compressed, rec.hex())
        data, want_st, want_pts = [], [], []
        gi = 0
        for ci, (rec, s, p) in enumerate(cases):
            for _ in range(7 + ci):
                data.append(enc[gi])
                want_st.append(OK)
                want_pts.append(base[gi])
                gi += 1
            data.append(rec)
            want_st.append(s)
            want_pts.append(p)
        pts, st, n_bad = _decode_raw(gpu, group, b"".join(data), compressed, True)
        assert list(st) == want_st, (compressed, [(i, int(a), b) for i, (a, b) in enumerate(zip(st, want_st)) if a != b])
        assert n_bad == sum(s != OK for s in want_st)
        assert (pts == np.stack(want_pts)).all(), compressed


@pytest.mark.parametrize("group", GROUPS)
def test_unchecked_mode(gpu, group):
    """checked = 0 is legal for both forms: an off-curve uncompressed point is returned as read (`deserialize_unchecked`); an
    off-subgroup compressed G2 point is returned with status 0 (`deserialize_compressed` leaves that test to its caller);
    encoding errors are still reported"""
    base, recs = _base(group)
    off = _bump_last_element(recs[False][1])
    bit7 = bytearray(recs[False][2])
    bit7[0] |= 0x80
    pts, st, n_bad = _decode_raw(gpu, group, recs[False][0] + off + bytes(bit7), False, False)
    assert list(st) == [OK, OK, BAD] and n_bad == 1
    assert (pts[0] == base[0]).all() and not pts[2].any()
    elems = [int.from_bytes(off[i:i + 32], "big") for i in range(0, len(off), 32)]
    as_read = [e for pair in zip(*[iter(elems)] * group) for e in reversed(pair)]  # c0 first
    assert (pts[1] == synth.to_mont(as_read, Q, 4).reshape(-1)).all()
    assert not O.on_curve(0, group, pts[1])
    assert list(_decode_raw(gpu, group, recs[False][0] + off + bytes(bit7), False, True)[1]) == [OK, OFF, BAD]
    data = [recs[True][0], recs[True][3]]
    want = [base[0], base[3]]
    if group == 2:
        p = _off_subgroup_g2(synth.XorShift(77))
        data.append(P.encode(2, p, True))
        want.append(p)
    pts, st, n_bad = _decode_raw(gpu, group, b"".join(data), True, False)
    assert not st.any() and n_bad == 0 and (pts == np.stack(want)).all()
    if group == 2:
        assert list(_decode_raw(gpu, group, b"".join(data), True, True)[1]) == [OK, OK, SUB]


@pytest.mark.parametrize("group", GROUPS)
def test_coordinates_are_reduced_mod_q(gpu, group):
    """`from_be_bytes_mod_order`: a first element stored as x + q (< 2^254, so that it stays clear of the flags) and every other
    element stored as v + k q for EVERY k with v + k q < 2^256 -- on points where k = 5 fits, v < 2^256 - 5 q ~ 0.29 q --
    decode to the limbs of the canonical record with status 0; re-encoding gives the canonical bytes"""
    base, recs = _base(group)
    for compressed in (True, False):
        nel = group * (1 if compressed else 2)
        data, want, canon = [], [], []
        for e in range(nel):
            limit, ks = ((1 << 254) - Q, (1,)) if e == 0 else ((1 << 256) - 5 * Q, (1, 2, 3, 4, 5))
            i = next(i for i, r in enumerate(recs[compressed])
                     if base[i].any() and (int.from_bytes(r[32 * e:32 * e + 32], "big") & ((1 << 254) - 1 if e == 0 else -1)) < limit)
            rec = recs[compressed][i]
            flags = rec[0] & 0xC0 if e == 0 else 0
            v = int.from_bytes(rec[32 * e:32 * e + 32], "big") & ((1 << 254) - 1 if e == 0 else (1 << 256) - 1)
            assert v + ks[-1] * Q < (1 << 254 if e == 0 else 1 << 256)
            assert e == 0 or v + 6 * Q >= 1 << 256  # 5 is every k there is
            for k in ks:
                b = bytearray(rec)
                b[32 * e:32 * e + 32] = (v + k * Q).to_bytes(32, "big")
                b[32 * e] |= flags
                assert bytes(b) != rec
                data.append(bytes(b))
                want.append(base[i])
                canon.append(rec)
        assert len(data) == 1 + 5 * (nel - 1)
        for rec, p in zip(data, want):
            got = P.decode(group, rec, compressed)
            assert got[0] == OK and (got[1] == p).all()
        pts, st, n_bad = _decode_raw(gpu, group, b"".join(data), compressed, True)
        assert not st.any() and n_bad == 0, (compressed, list(st))
        assert (pts == np.stack(want)).all(), compressed
        assert gpu.ppot_points_encode(group, pts, compressed) == b"".join(canon)


def _neg(group, p):
    y = synth.from_mont(np.asarray(p[4 * group:]).reshape(group, 4), Q)
    out = np.array(p, dtype=np.uint64)
    out[4 * group:] = synth.to_mont([(Q - c) % Q for c in y], Q, 4).reshape(-1)
    return out


@pytest.mark.parametrize("group", GROUPS)
def test_both_greatest_choices(gpu, group):
    """for 200 points the compressed records of P and -P differ in bit 7 of byte 0 and nowhere else, and each decodes to its
    own point. The order on Fq2 looks at c1 first; a G2 point with y.c1 = 0, where c0 decides, turns up with probability 1 / q
    per try, so no search reaches one: that branch is not asserted here."""
    base, _ = _base(group)
    pos = np.stack([p for p in base[:201] if p.any()])[:200]
    neg = np.stack([_neg(group, p) for p in pos])
    nb = gpu.ppot_point_bytes(group, True)
    ep, en = gpu.ppot_points_encode(group, pos, True), gpu.ppot_points_encode(group, neg, True)
    assert ep == P.encode_many(group, pos, True) and en == P.encode_many(group, neg, True)
    for i in range(200):
        a, b = ep[i * nb:(i + 1) * nb], en[i * nb:(i + 1) * nb]
        assert a[0] ^ b[0] == 0x80 and a[1:] == b[1:], i
    highs = sum(ep[i * nb] >> 7 for i in range(200))
    assert 0 < highs < 200
    for enc, want in ((ep, pos), (en, neg)):
        pts, st = gpu.ppot_points_decode(group, enc, True)
        assert not st.any() and (pts == want).all()


def test_arguments(gpu):
    """Bn254 only; group 1 or 2"""
    base, recs = _base(1)
    out = np.zeros((1, 8), dtype=np.uint64)
    args = (recs[True][0], ctypes.c_size_t(1), 1, 1, out.ctypes.data_as(ctypes.c_void_p), None, None)
    assert gpu.LIB.mg_ppot_points_decode(0, 1, *args) == 0 and (out[0] == base[0]).all()
    for curve, group in ((1, 1), (0, 3)):
        rc = gpu.LIB.mg_ppot_points_decode(curve, group, *args)
        assert rc != 0
        with pytest.raises(gpu.MantaGpuError):
            gpu._chk(rc, "mg_ppot_points_decode")
        rc = gpu.LIB.mg_ppot_points_encode(curve, group, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), 1,
                                           ctypes.create_string_buffer(64))
        with pytest.raises(gpu.MantaGpuError):
            gpu._chk(rc, "mg_ppot_points_encode")
    with pytest.raises(gpu.MantaGpuError):
        gpu.ppot_points_decode(3, recs[True][0], True)
