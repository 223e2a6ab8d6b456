"""Perpetual Powers of Tau files on the GPU (manta_rs_amd/ppot.py): a small ceremony (32 powers) written in both forms, a
sub-accumulator of 8 powers read back from it (`read_subaccumulator`), every decode error by field, index and variant, the
key `ceremony.initialize` makes of what was read, `Accumulator.verify_transform`, the contribution proof of a response file
and the two hashes. Yardsticks: the accumulator the file was written from, tests/ppot_ref.py, the CPU oracle and hashlib."""
import hashlib
import mmap

import numpy as np
import pytest

import oracle_lib as O
import ppot_ref as P
from manta_rs_amd import ceremony, ppot, synth

pytestmark = pytest.mark.gpu
POWERS, SUB = 32, 8
R = P.R
HEADER = bytes(range(64))
TAU, ALPHA, BETA = 0x1234567 % R, 0xABCDEF % R, 0x7777 % R
RHO = [(0x9E3779B97F4A7C15 * (i + 1)) % R for i in range(2 * POWERS)]
KEY_ARRAYS = ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "gamma_g2", "delta_g2", "gamma_abc_g1", "l_query", "a_query",
              "b_g1_query", "b_g2_query", "h_query")


def _fresh(n2):
    g1 = np.tile(O.generator(0, 1), (2 * n2 - 1, 1))
    g2 = np.tile(O.generator(0, 2), (n2, 1))
    return ceremony.Accumulator(0, g1, g2, g1[:n2], g1[:n2], g2[0])


def _sub(acc, n2):
    return ceremony.Accumulator(0, acc.tau_powers_g1[:2 * n2 - 1], acc.tau_powers_g2[:n2], acc.alpha_tau_powers_g1[:n2],
                                acc.beta_tau_powers_g1[:n2], acc.beta_g2)


def _equal(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f, _ in ceremony.Accumulator.FIELDS)


@pytest.fixture(scope="module")
def acc(gpu):
    a = _fresh(POWERS)
    a.update(TAU, ALPHA, BETA)
    return a


@pytest.fixture(scope="module")
def files(gpu, acc):
    """the ceremony's file in both forms, keyed by `compressed`: written once, never changed"""
    return {c: ppot.write_accumulator(acc, HEADER, c) for c in (True, False)}


def _span(element, compressed, powers=POWERS, count=None):
    """byte range of the first `count` points of an element"""
    _, g = ppot.ELEMENTS[element]
    n = {"TauG1": 2 * SUB - 1, "BetaG2": 1}.get(element, SUB) if count is None else count
    start = P.position(element, 0, compressed, powers)
    return start, start + n * P.point_bytes(g, compressed)


class Recorder:
    """no buffer itself: hands out slices of one and records which"""

    def __init__(self, data):
        self.data, self.slices = memoryview(data), []

    def __len__(self):
        return len(self.data)

    def __getitem__(self, s):
        assert isinstance(s, slice) and s.step is None
        self.slices.append((s.start, s.stop))
        return self.data[s]


def test_written_file_is_the_reference_layout(gpu, acc, files):
    for compressed in (True, False):
        want = HEADER + b"".join(P.encode_many(g, getattr(acc, f), compressed) for f, g in ppot.ELEMENTS.values())
        assert files[compressed] == want
        assert len(want) == P.position("BetaG2", 0, compressed, POWERS) + P.point_bytes(2, compressed)
    with pytest.raises(ValueError):
        ppot.write_accumulator(acc, HEADER[:63], True)
    with pytest.raises(ValueError):
        ppot.write_accumulator(ceremony.Accumulator(0, acc.tau_powers_g1, acc.tau_powers_g2[:5], acc.alpha_tau_powers_g1,
                                                    acc.beta_tau_powers_g1, acc.beta_g2), HEADER, True)


def test_read_subaccumulator(gpu, acc, files, tmp_path):
    """the first 15 / 8 / 8 / 8 powers and beta_g2 of a 32-power file, exactly; the same from an mmap; only the five spans are
    ever sliced; the powers check out; a compressed response and an uncompressed challenge of one accumulator read back equal"""
    want = _sub(acc, SUB)
    got = {}
    for compressed in (True, False):
        got[compressed] = ppot.read_subaccumulator(files[compressed], SUB, compressed, ceremony_powers=POWERS)
        assert _equal(got[compressed], want), compressed
        assert got[compressed].tau_powers_g1.shape == (15, 8) and got[compressed].tau_powers_g2.shape == (8, 16)
        assert got[compressed].alpha_tau_powers_g1.shape == (8, 8) and got[compressed].beta_g2.shape == (1, 16)
        path = tmp_path / f"challenge_{int(compressed)}"
        path.write_bytes(files[compressed])
        with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            assert _equal(ppot.read_subaccumulator(mm, SUB, compressed, ceremony_powers=POWERS), want)
            assert ppot.file_hash(mm) == hashlib.blake2b(files[compressed], digest_size=64).digest()
        rec = Recorder(files[compressed])
        assert _equal(ppot.read_subaccumulator(rec, SUB, compressed, ceremony_powers=POWERS), want)
        assert sorted(rec.slices) == sorted(_span(e, compressed) for e in ppot.ELEMENTS)
    assert _equal(got[True], got[False])
    assert got[True].check_powers(RHO) == ""
    full = ppot.read_subaccumulator(files[True], POWERS, True, ceremony_powers=POWERS)
    assert _equal(full, acc)
    with pytest.raises(ValueError):
        ppot.read_subaccumulator(files[True][:-1], SUB, True, ceremony_powers=POWERS)
    with pytest.raises(ValueError):
        ppot.read_subaccumulator(files[True], POWERS + 1, True, ceremony_powers=POWERS)
    with pytest.raises(ValueError):  # an uncompressed file is no compressed one of twice the size: too short for 64 powers
        ppot.read_subaccumulator(files[True], SUB, False, ceremony_powers=POWERS)


def _record(element, index, compressed):
    _, g = ppot.ELEMENTS[element]
    nb = P.point_bytes(g, compressed)
    start = P.position(element, index, compressed, POWERS)
    return start, start + nb


def _off_curve(data, element, index, compressed):
    """uncompressed: y (y.c0) + 1; compressed: the next x whose x^3 + b has no root"""
    _, g = ppot.ELEMENTS[element]
    a, b = _record(element, index, compressed)
    rec = bytearray(data[a:b])
    if not compressed:
        rec[-32:] = ((int.from_bytes(rec[-32:], "big") + 1) % P.Q).to_bytes(32, "big")
    else:
        rec[0] &= 0x3F
        while P.decode(g, bytes(rec), True)[0] != P.OFF:
            rec[-32:] = ((int.from_bytes(rec[-32:], "big") + 1) % P.Q).to_bytes(32, "big")
    data[a:b] = rec


def _off_subgroup_g2():
    rng = synth.XorShift(4242)
    rk = synth.ints_to_limbs([R], 4)[0]
    while True:
        enc = b"".join(rng.field(P.Q).to_bytes(32, "little") for _ in range(2))
        ok, p = O.deserialize(0, 2, enc, True)
        if ok and O.on_curve(0, 2, p) and O.g_mul(0, 2, p, rk).any():
            return p


def test_every_decode_error_by_field_index_and_variant(gpu, files, tmp_path):
    """one corrupted record per field, one at a time; then two in one field (the encoding error wins over the earlier curve
    error) and two in two fields (the earlier field wins); an error leaves no view of the caller's buffer behind, so an mmap
    still closes while the exception and its traceback are held"""
    off2 = _off_subgroup_g2()
    d = bytearray(files[False])
    d[_record("TauG1", 9, False)[0]] |= 0x80
    (tmp_path / "bad").write_bytes(d)
    with open(tmp_path / "bad", "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        with pytest.raises(ppot.PpotDecodeError) as held:
            ppot.read_subaccumulator(mm, SUB, False, ceremony_powers=POWERS)
    assert (held.value.field, held.value.index, held.value.variant) == ("tau_powers_g1", 9, "ExpectedUncompressed")

    def expect(data, compressed, field, index, variant):
        with pytest.raises(ppot.PpotDecodeError) as ei:
            ppot.read_subaccumulator(bytes(data), SUB, compressed, ceremony_powers=POWERS)
        assert (ei.value.field, ei.value.index, ei.value.variant) == (field, index, variant), str(ei.value)

    for compressed in (True, False):
        fresh = lambda: bytearray(files[compressed])  # noqa: E731
        if not compressed:
            d = fresh()
            d[_record("TauG1", 9, False)[0]] |= 0x80
            expect(d, False, "tau_powers_g1", 9, "ExpectedUncompressed")
            d = fresh()
            d[_record("BetaG2", 0, False)[0]] |= 0xC0  # bit 7 is looked at first
            expect(d, False, "beta_g2", 0, "ExpectedUncompressed")
        d = fresh()
        d[_record("AlphaG1", 3, compressed)[0]] |= 0x40  # the infinity flag on a record that is not zero
        expect(d, compressed, "alpha_tau_powers_g1", 3, "PointAtInfinity")
        d = fresh()
        a, b = _record("TauG2", 4, compressed)
        d[a:b] = P.encode(2, off2, compressed)
        expect(d, compressed, "tau_powers_g2", 4, "NotInSubgroup")
        for element, index, field in (("BetaG1", 7, "beta_tau_powers_g1"), ("BetaG2", 0, "beta_g2"), ("TauG1", 14, "tau_powers_g1")):
            d = fresh()
            _off_curve(d, element, index, compressed)
            expect(d, compressed, field, index, "NotOnCurve")
        d = fresh()
        _off_curve(d, "TauG1", 15, compressed)  # past the 15 powers that are read: not looked at
        assert ppot.read_subaccumulator(bytes(d), SUB, compressed, ceremony_powers=POWERS) is not None
        # a curve error at index 2, an encoding error at 5: the encoding error is named. Uncompressed that is the reference's
        # order; compressed it is the documented rule of `ppot._first_error`, where the reference would meet the missing root first
        d = fresh()
        _off_curve(d, "BetaG1", 2, compressed)
        d[_record("BetaG1", 5, compressed)[0]] |= 0x40
        expect(d, compressed, "beta_tau_powers_g1", 5, "PointAtInfinity")
        a, b = _record("TauG2", 1, compressed)
        d[a:b] = P.encode(2, off2, compressed)
        expect(d, compressed, "tau_powers_g2", 1, "NotInSubgroup")
        d[_record("TauG1", 0, compressed)[0]] |= 0x40
        expect(d, compressed, "tau_powers_g1", 0, "PointAtInfinity")


def test_initialize_from_the_file(gpu, acc, files):
    """the phase-2 key of a D = 8 circuit from the sub-accumulator read from the file == the key from the slices of the object
    the file was written from, array for array; `state_check` passes on it"""
    c = synth.make_circuit(0, 5, 6, 2, seed=84)
    assert c.D == SUB
    read = ppot.read_subaccumulator(files[True], SUB, True, ceremony_powers=POWERS)
    pk, want = ceremony.initialize(read, c), ceremony.initialize(_sub(acc, SUB), c)
    for k in KEY_ARRAYS:
        assert np.array_equal(getattr(pk, k), getattr(want, k)), k
        assert getattr(pk, k).any(), k
    assert ceremony.state_check(0, pk) is None


def _times(group, point, k):
    return ceremony.batch_mul_fixed_scalar(0, group, np.asarray(point).reshape(1, -1), k)[0]


def test_verify_transform(gpu, acc):
    """two successive states of an 8-power accumulator and the honest certificate -- per scalar s the pair (s H, H) that
    `RatioProof::verify` returns as (matching_point, challenge_point), H = the G2 generator here -- then one thing wrong at a
    time, each with the reference's variant"""
    tau, alpha, beta = 0x51EDC0DE % R, 0xFACADE % R, 0xB0BA % R
    last = _sub(acc, SUB)
    nxt = _sub(acc, SUB)
    nxt.update(tau, alpha, beta)
    h = O.generator(0, 2)
    cert = tuple((_times(2, h, s), h) for s in (tau, alpha, beta))
    verify = ceremony.Accumulator.verify_transform
    assert verify(last, nxt, cert, RHO) == ""
    assert verify(last, nxt, ((_times(2, h, tau + 1), h), cert[1], cert[2]), RHO) == "TauMultiplication"
    assert verify(last, nxt, (cert[0], cert[2], cert[2]), RHO) == "AlphaMultiplication"
    assert verify(last, nxt, (cert[0], cert[1], cert[0]), RHO) == "BetaMultiplication"

    def tampered(field, index, k=3):
        t = _sub(nxt, SUB)
        v = np.array(getattr(t, field), dtype=np.uint64)
        v[index] = _times(1 if v.shape[1] == 8 else 2, v[index], k)
        setattr(t, field, v)
        return t

    assert verify(last, tampered("beta_g2", 0), cert, RHO) == "BetaMultiplication"
    assert verify(last, tampered("tau_powers_g2", 4), cert, RHO) == "TauG1Powers"  # the G2 powers against tau G1
    assert verify(last, tampered("tau_powers_g1", 9), cert, RHO) == "TauG2Powers"  # the G1 powers against tau G2
    assert verify(last, tampered("alpha_tau_powers_g1", 4), cert, RHO) == "AlphaG1Powers"
    assert verify(last, tampered("beta_tau_powers_g1", 4), cert, RHO) == "BetaG1Powers"
    assert verify(last, tampered("tau_powers_g1", 0), cert, RHO) == "PrimeSubgroupGeneratorG1"
    assert verify(last, tampered("tau_powers_g2", 0), cert, RHO) == "PrimeSubgroupGeneratorG2"


def _proof_points(acc):
    """nine points in file order: any six G1 and three G2 points of the ceremony will do"""
    return {"tau_ratio": acc.tau_powers_g1[1:3], "alpha_ratio": acc.alpha_tau_powers_g1[2:4],
            "beta_ratio": acc.beta_tau_powers_g1[4:6], "tau_matching_point": acc.tau_powers_g2[1],
            "alpha_matching_point": acc.tau_powers_g2[2], "beta_matching_point": acc.beta_g2[0]}


def _proof_bytes(proof):
    return (b"".join(P.encode_many(1, proof[k], False) for k in ppot.PROOF_G1)
            + b"".join(P.encode(2, proof[k], False) for k in ppot.PROOF_G2))


def test_read_kzg_proof(gpu, acc, files):
    """nine points written behind the compressed accumulator of a 32-power response come back equal; infinity among them,
    a file cut short and a record off the curve are refused"""
    proof = _proof_points(acc)
    assert len(files[True]) == ppot.proof_position(POWERS) == 64 + (63 + 2 * 32) * 32 + 33 * 64
    response = files[True] + _proof_bytes(proof)
    got = ppot.read_kzg_proof(response, ceremony_powers=POWERS)
    assert list(got) == list(ppot.PROOF_G1 + ppot.PROOF_G2)
    for k, v in proof.items():
        assert np.array_equal(got[k], v), k
    assert all(np.array_equal(v, proof[k]) for k, v in ppot.read_kzg_proof(Recorder(response), ceremony_powers=POWERS).items())
    for name, at in (("alpha_ratio", 3 * 64), ("beta_matching_point", 6 * 64 + 2 * 128)):
        bad = bytearray(response)
        nb = 64 if at < 6 * 64 else 128
        bad[len(files[True]) + at:len(files[True]) + at + nb] = b"\x40" + bytes(nb - 1)
        with pytest.raises(ValueError, match=name) as ei:
            ppot.read_kzg_proof(bytes(bad), ceremony_powers=POWERS)
        assert not isinstance(ei.value, ppot.PpotDecodeError)
    with pytest.raises(ValueError):
        ppot.read_kzg_proof(response[:-1], ceremony_powers=POWERS)
    bad = bytearray(response)
    bad[len(files[True]) + 64 + 63] ^= 1  # tau_ratio[1].y
    with pytest.raises(ppot.PpotDecodeError) as ei:
        ppot.read_kzg_proof(bytes(bad), ceremony_powers=POWERS)
    assert (ei.value.field, ei.value.index, ei.value.variant) == ("tau_ratio", 1, "NotOnCurve")


def test_response_hash_and_file_hash(gpu, acc, files):
    """`Configuration::response` (ppot/kzg.rs:85-118): Blake2b-512 over the accumulator in arkworks uncompressed form, the
    challenge, then the three ratio proofs one after the other, each ratio.0 | ratio.1 | matching_point in arkworks
    COMPRESSED form (`RatioProof`'s derived serializer, ratio.rs:50-63) -- every byte from the oracle's serialize, assembled
    here and hashed by hashlib. It is not the hash over `Proof::serialize`'s PPoT records, ratios first."""
    sub = _sub(acc, SUB)
    proof = _proof_points(acc)
    challenge = hashlib.blake2b(b"challenge", digest_size=64).digest()
    stream = b"".join(O.serialize(0, g, p, False) for f, g in ceremony.Accumulator.FIELDS for p in getattr(sub, f))
    stream += challenge
    for s in ("tau", "alpha", "beta"):
        r0, r1 = proof[s + "_ratio"]
        stream += O.serialize(0, 1, r0, True) + O.serialize(0, 1, r1, True) + O.serialize(0, 2, proof[s + "_matching_point"], True)
    assert len(stream) == (15 + 8 + 8) * 64 + 9 * 128 + 64 + 3 * (32 + 32 + 64)
    assert ppot.response_hash(sub, challenge, proof) == hashlib.blake2b(stream, digest_size=64).digest()
    wrong = stream[:-3 * 128] + (b"".join(P.encode_many(1, proof[k], True) for k in ppot.PROOF_G1)
                                 + b"".join(P.encode(2, proof[k], True) for k in ppot.PROOF_G2))
    assert ppot.response_hash(sub, challenge, proof) != hashlib.blake2b(wrong, digest_size=64).digest()
    with pytest.raises(ValueError):
        ppot.response_hash(sub, challenge[:32], proof)
    for data in (files[True], files[False], b""):
        assert ppot.file_hash(data) == hashlib.blake2b(data, digest_size=64).digest()
