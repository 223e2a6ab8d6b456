"""GPU batched point codec (mg_points_decode / mg_points_check / mg_points_encode / mg_proofs_decode): arkworks 0.3
short-Weierstrass encodings of G1 / G2 on BN254 and BLS12-381, decoded and checked (curve, subgroup [r]P == O) one point
per lane. Yardsticks: the CPU oracle's serialize / deserialize / on_curve / g_mul, the reference's committed verifying-key
bytes, and the host single-proof decoder mg_proof_decode."""
import ctypes

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
from manta_rs_amd import ceremony, keygen, synth
from vk_fixtures import VK, VK_FILES

pytestmark = pytest.mark.gpu
CASES = [(0, 1), (0, 2), (1, 1), (1, 2)]
CHUNK = 1 << 16  # points on the device per launch (mantagpu.h)
OK, BAD, OFF, SUB = 0, 1, 2, 3


def _fq(curve):
    return synth.FQ_MODULUS[curve], synth.FQ_LIMBS[curve] * 8


def _base_points(curve, group, n, seed):
    pts = H.random_points(curve, group, n, seed=seed)
    pts[n // 3] = 0  # infinity inside the batch
    return pts


def _expected(curve, group, pts, compressed):
    return b"".join(O.serialize(curve, group, p, compressed) for p in pts)


@pytest.mark.parametrize("curve,group", CASES)
def test_round_trip_every_size(gpu, curve, group):
    """encode == the oracle's serialize byte for byte; decode(checked) gives the limbs back with every status 0 -- for
    n = 0, 1, 63, 64, 65, 1000 and one n above the staging chunk, compressed and uncompressed."""
    base = _base_points(curve, group, 1000, seed=300 + 10 * curve + group)
    for compressed in (True, False):
        want = _expected(curve, group, base, compressed)
        nb = gpu.point_bytes(curve, group, compressed)
        for n in (0, 1, 63, 64, 65, 1000):
            enc = gpu.points_encode(curve, group, base[:n], compressed)
            assert enc == want[:n * nb], (n, compressed)
            pts, st = gpu.points_decode(curve, group, enc, compressed)
            assert pts.shape == (n, gpu.affine_limbs(curve, group)) and st.shape == (n,)
            assert (st == OK).all(), (n, compressed, np.flatnonzero(st)[:5])
            assert (pts == base[:n]).all(), (n, compressed)
        big = CHUNK + 37
        reps = -(-big // 1000)
        pts_big = np.tile(base, (reps, 1))[:big]
        enc = gpu.points_encode(curve, group, pts_big, compressed)
        assert enc == (want * reps)[:big * nb]
        pts, st = gpu.points_decode(curve, group, enc, compressed)
        assert (st == OK).all() and (pts == pts_big).all()
        assert (gpu.points_check(curve, group, pts_big) == OK).all()


def test_reference_verifying_key_bytes(gpu):
    """every compressed point of the six committed verifying-key files, one batch per group: equal to the fixtures' parse,
    and re-encoding gives the files' bytes"""
    g1_bytes, g1_want, g2_bytes, g2_want = [], [], [], []
    for name in sorted(VK_FILES):
        vk = VK(name)
        g1_bytes += [vk.alpha_bytes] + vk.abc_bytes
        g1_want += [vk.alpha] + vk.abc
        g2_bytes += vk.g2_bytes
        g2_want += vk.g2
    for group, data, want in ((1, g1_bytes, g1_want), (2, g2_bytes, g2_want)):
        pts, st = gpu.points_decode(0, group, data)
        assert (st == OK).all()
        assert (pts == np.stack(want)).all()
        assert gpu.points_encode(0, group, pts) == b"".join(data)


def _le(v, nb):
    return int(v).to_bytes(nb, "little")


def _coords(curve, group, enc, compressed):
    """the canonical integers of an encoding (flags cleared) -- x (and y), each 1 or 2 base-field elements"""
    q, fb = _fq(curve)
    k = len(enc) // fb
    vals = [int.from_bytes(enc[i * fb:(i + 1) * fb], "little") for i in range(k)]
    vals[-1] &= ~(0xC0 << (8 * fb - 8))
    return vals


def _no_root_x(curve, group, rng):
    """a compressed encoding whose x^3 + b has no square root"""
    q, fb = _fq(curve)
    while True:
        xs = [rng.field(q) for _ in range(group)]
        enc = b"".join(_le(x, fb) for x in xs)
        ok, _ = O.deserialize(curve, group, enc, True)
        if not ok:
            return enc


def _off_subgroup(curve, group, rng):
    """a point on the curve outside the subgroup: O.deserialize on a random x checks neither"""
    q, fb = _fq(curve)
    r = synth.FR_MODULUS[curve]
    rk = synth.ints_to_limbs([r], 4)[0]
    while True:
        enc = b"".join(_le(rng.field(q), fb) for _ in range(group))
        ok, p = O.deserialize(curve, group, enc, True)
        if ok and O.on_curve(curve, group, p) and O.g_mul(curve, group, p, rk).any():
            return enc, p


def _decode_raw(gpu, curve, group, data, compressed, checked):
    nb = gpu.point_bytes(curve, group, compressed)
    n = len(data) // nb
    out = np.zeros((n, gpu.affine_limbs(curve, group)), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    n_bad = ctypes.c_size_t(12345)
    rc = gpu.LIB.mg_points_decode(curve, group, bytes(data), ctypes.c_size_t(n), int(compressed), int(checked),
                                  out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_bad))
    assert rc == 0
    return out, st, n_bad.value


@pytest.mark.parametrize("curve,group", CASES)
def test_rejections_mixed_into_good_batches(gpu, curve, group):
    """each bad encoding sits between good points, with its exact status; the good points still decode, n_bad is exact"""
    q, fb = _fq(curve)
    rng = synth.XorShift(900 + 10 * curve + group)
    good = H.random_points(curve, group, 300, seed=400 + 10 * curve + group)
    for compressed in (True, False):
        enc = [O.serialize(curve, group, p, compressed) for p in good]
        nb = len(enc[0])
        cases = []  # (encoding, status, expected limbs or None)
        # x >= p: x + p in the first coordinate (BN254 G1: a point with x + p < 2^254, so that no flag bit is touched)
        for i, e in enumerate(enc):
            if not good[i].any():
                continue
            x0 = int.from_bytes(e[:fb], "little") & ((1 << (8 * fb - 2)) - 1)
            if x0 + q < 1 << (8 * fb - 2):
                flags = e[fb - 1] & 0xC0 if (group == 1 and compressed) else 0
                b = bytearray(e)
                b[:fb] = _le(x0 + q, fb)
                b[fb - 1] |= flags
                cases.append((bytes(b), BAD, None))
                break
        both = bytearray(enc[5])
        both[-1] |= 0xC0
        cases.append((bytes(both), BAD, None))
        if compressed:
            cases.append((_no_root_x(curve, group, rng), OFF, None))
        else:
            y = bytearray(enc[6])
            yc0 = int.from_bytes(y[group * fb:(group + 1) * fb], "little")
            y[group * fb:(group + 1) * fb] = _le((yc0 + 1) % q, fb)
            cases.append((bytes(y), OFF, None))
        # off the subgroup (BN254 G1 has cofactor 1: every on-curve point is in it)
        enc_s, p_s = _off_subgroup(curve, group, rng) if (curve, group) != (0, 1) else (None, None)
        if enc_s is not None:
            cases.append((O.serialize(curve, group, p_s, compressed), SUB, None))
        else:
            for _ in range(20):
                e = b"".join(_le(rng.field(q), fb) for _ in range(group))
                ok, p = O.deserialize(curve, group, e, True)
                if ok:
                    cases.append((O.serialize(curve, group, p, compressed), OK, p))
        # infinity: canonical -> OK (zeros); a canonical non-zero x is ignored (verify.cpp); a non-canonical x is rejected
        # although mo_point_deserialize would accept it (it returns at the flag); infinity + "greatest" is no SWFlags value
        inf = bytearray(nb)
        inf[-1] = 0x40
        cases.append((bytes(inf), OK, None))
        inf5 = bytearray(inf)
        inf5[0] = 5
        cases.append((bytes(inf5), OK, None))
        infbad = bytearray(b"\xff" * nb)
        infbad[-1] = 0x7F
        assert O.deserialize(curve, group, bytes(infbad), compressed)[0]
        cases.append((bytes(infbad), BAD, None))
        infg = bytearray(inf)
        infg[-1] = 0xC0
        cases.append((bytes(infg), BAD, None))
        # build the batch: good points with the cases spread between them
        data, want_st, want_pts = [], [], []
        gi = 0
        for ci, (b, s, p) in enumerate(cases):
            for _ in range(7 + ci):
                data.append(enc[gi % len(enc)])
                want_st.append(OK)
                want_pts.append(good[gi % len(enc)])
                gi += 1
            data.append(b)
            want_st.append(s)
            want_pts.append(p if p is not None else np.zeros_like(good[0]))
        pts, st, n_bad = _decode_raw(gpu, curve, group, b"".join(data), compressed, True)
        assert list(st) == want_st, (compressed, [(i, int(a), b) for i, (a, b) in enumerate(zip(st, want_st)) if a != b])
        assert n_bad == sum(s != OK for s in want_st)
        assert (pts == np.stack(want_pts)).all(), compressed


@pytest.mark.parametrize("curve,group", CASES)
def test_unchecked_mode(gpu, curve, group):
    """checked = 0 (uncompressed only, as the proving-key reader): an off-curve point is accepted as read, a coordinate
    >= p is still rejected; compressed + unchecked is an argument error"""
    q, fb = _fq(curve)
    good = H.random_points(curve, group, 3, seed=77)
    e = bytearray(O.serialize(curve, group, good[1], False))
    yc0 = int.from_bytes(e[group * fb:(group + 1) * fb], "little")
    e[group * fb:(group + 1) * fb] = _le((yc0 + 1) % q, fb)
    bad = bytearray(e)
    bad[:fb] = _le(q, fb)
    data = O.serialize(curve, group, good[0], False) + bytes(e) + bytes(bad)
    pts, st, n_bad = _decode_raw(gpu, curve, group, data, False, False)
    assert list(st) == [OK, OK, BAD] and n_bad == 1
    assert (pts[0] == good[0]).all()
    vals = _coords(curve, group, bytes(e), False)
    assert (pts[1] == synth.to_mont(vals, q, synth.FQ_LIMBS[curve]).reshape(-1)).all()
    assert not O.on_curve(curve, group, pts[1])
    _, st, _ = _decode_raw(gpu, curve, group, data, False, True)
    assert list(st) == [OK, OFF, BAD]
    with pytest.raises(gpu.MantaGpuError):
        gpu.points_decode(curve, group, O.serialize(curve, group, good[0], True), compressed=True, checked=False)


@pytest.mark.parametrize("curve,group", CASES)
def test_check_points_in_memory(gpu, curve, group):
    """mg_points_check: good points and infinity pass; a coordinate >= q, an off-curve point and an off-subgroup point
    carry their status"""
    q, _ = _fq(curve)
    nl = synth.FQ_LIMBS[curve]
    pts = H.random_points(curve, group, 200, seed=55).copy()
    pts[3] = 0
    want = np.zeros(200, dtype=np.uint8)
    pts[10, :nl] = synth.ints_to_limbs([q], nl)[0]
    want[10] = BAD
    pts[20, -1] ^= 1
    want[20] = OFF
    if (curve, group) != (0, 1):
        _, p = _off_subgroup(curve, group, synth.XorShift(5 + curve + group))
        pts[30] = p
        want[30] = SUB
    assert (gpu.points_check(curve, group, pts) == want).all()
    assert gpu.points_check(curve, group, pts[:0]).shape == (0,)


def _fuzz(curve, proof, kind, rng):
    q, fb = _fq(curve)
    b = bytearray(proof)
    if kind == 0:  # flip a byte
        i = rng.next() % len(b)
        b[i] ^= 1 << (rng.next() % 8)
    elif kind == 1:  # A's x made non-canonical (BLS12-381 has room above p; BN254: the top bit below the flags)
        x = int.from_bytes(b[:fb], "little") & ((1 << (8 * fb - 2)) - 1)
        flags = b[fb - 1] & 0xC0
        b[:fb] = _le(x + q if x + q < 1 << (8 * fb - 2) else (1 << (8 * fb - 2)) - 1, fb)
        b[fb - 1] |= flags
    else:  # B off the subgroup (BN254 G2 and BLS12-381 G2 have a cofactor)
        _, p = _off_subgroup(curve, 2, rng)
        b[fb:3 * fb] = O.serialize(curve, 2, p, True)
    return bytes(b)


@pytest.mark.parametrize("curve", [0, 1])
def test_proofs_decode_matches_the_host_decoder(gpu, curve):
    """k = 256 proofs from GPU proving with distinct assignments, ~10 % fuzzed: ok[i] == (mg_proof_decode accepts proof i),
    identical points where it does; the decoded good proofs pass the batch verifier"""
    k = 256
    c0 = synth.make_circuit(curve, 120, 90, 4, seed=1700 + curve)
    pk = keygen.generate(c0, synth.from_mont(H.toxic(curve, seed=41), synth.FR_MODULUS[curve]))
    ctx = gpu.ProvingContext(curve, pk)
    ctx.set_r1cs(gpu.R1CS.from_circuit(c0))
    R = synth.Reassigner(c0)
    cs = [R.assign(9000 + i) for i in range(k)]
    rs = H.rand_fr_mont(curve, 2 * k, seed=123)
    proofs = gpu.Groth16.prove_batch(ctx, np.stack([x.z for x in cs]), rs[:k], rs[k:])
    assert len(set(proofs)) == k
    rng = synth.XorShift(31 + curve)
    fuzzed = list(proofs)
    victims = list(range(3, k, 10))
    for j, i in enumerate(victims):
        fuzzed[i] = _fuzz(curve, proofs[i], j % 3, rng)
    pts, ok = gpu.proofs_decode(curve, fuzzed)
    assert pts.shape[0] == k and ok.shape == (k,)
    for i in range(k):
        try:
            want = gpu.proof_decode(curve, fuzzed[i])
            host_ok = True
        except gpu.MantaGpuError:
            host_ok = False
        assert bool(ok[i]) == host_ok, i
        if host_ok:
            assert (pts[i] == want).all(), i
        else:
            assert not pts[i].any(), i
    assert not ok[[v for j, v in enumerate(victims) if j % 3]].any()  # non-canonical x, off-subgroup B
    good = [i for i in range(k) if i not in victims]
    assert ok[good].all()
    vctx = gpu.VerifyingContext(curve, pk)
    inputs = np.stack([cs[i].z[1:c0.P] for i in good])
    rnd = np.random.RandomState(9).randint(1, 1 << 62, size=(len(good), 2)).astype(np.uint64)
    assert gpu.groth16_verify_batch(vctx, inputs, [pts[i] for i in good], rnd) is True
    assert gpu.proofs_decode(curve, b"")[0].shape[0] == 0


@pytest.mark.parametrize("curve", [0, 1])
def test_state_check(gpu, curve):
    """ceremony.state_check (mpc.rs:79-100) passes on a generated key and names the swapped-in off-subgroup b_g2_query
    entry; an off-curve a_query entry is found first (G1 before G2)"""
    c = synth.make_circuit(curve, 60, 50, 3, seed=2100 + curve)
    pk = keygen.generate(c, synth.from_mont(H.toxic(curve, seed=43), synth.FR_MODULUS[curve]))
    assert ceremony.state_check(curve, pk) is None
    _, p = _off_subgroup(curve, 2, synth.XorShift(77 + curve))
    pk.b_g2_query = pk.b_g2_query.copy()
    pk.b_g2_query[17] = p
    assert ceremony.state_check(curve, pk) == ("b_g2_query", 17)
    pk.a_query = pk.a_query.copy()
    pk.a_query[4, -1] ^= 1
    assert ceremony.state_check(curve, pk) == ("a_query", 4)


@pytest.mark.parametrize("curve", [0, 1])
def test_accumulator_codec(gpu, curve):
    """Accumulator.encode / decode (kzg.rs field order) round-trip in both forms after an update; the encoding is the
    oracle's point by point; one corrupted power is reported by field and index"""
    n1, n2 = 15, 8
    r = synth.FR_MODULUS[curve]
    g1 = np.tile(O.generator(curve, 1), (n1, 1))
    g2 = np.tile(O.generator(curve, 2), (n2, 1))
    acc = ceremony.Accumulator(curve, g1, g2, g1[:n2], g1[:n2], g2[0])
    acc.update(0x1234567 % r, 0xabcdef % r, 0x7777 % r)
    for compressed in (True, False):
        data = acc.encode(compressed)
        want = b"".join(_expected(curve, g, getattr(acc, f).reshape(-1, gpu.affine_limbs(curve, g)), compressed)
                        for f, g in ceremony.Accumulator.FIELDS)
        assert data == want
        back = ceremony.Accumulator.decode(curve, data, n1, n2, compressed)
        for f, _ in ceremony.Accumulator.FIELDS:
            assert (getattr(back, f) == getattr(acc, f).reshape(getattr(back, f).shape)).all(), f
        # corrupt alpha_tau_powers_g1[3]: both flag bits
        off = n1 * gpu.point_bytes(curve, 1, compressed) + n2 * gpu.point_bytes(curve, 2, compressed)
        nb = gpu.point_bytes(curve, 1, compressed)
        bad = bytearray(data)
        bad[off + 4 * nb - 1] |= 0xC0
        with pytest.raises(ceremony.AccumulatorDecodeError) as ei:
            ceremony.Accumulator.decode(curve, bytes(bad), n1, n2, compressed)
        assert (ei.value.field, ei.value.index, ei.value.status) == ("alpha_tau_powers_g1", 3, BAD)
