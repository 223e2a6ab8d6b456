"""Per-item verdicts in one pass: `mg_groth16_verify_each` (k proofs of one key, what `mg_groth16_verify` answers for each) and
`mg_pairing_check_each` (independent pairing products, what `mg_pairing_check` answers for each). The verdicts are exact, so
every comparison is element for element with the single call on the same row, and with the oracle where it can read the row."""
import threading

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
from manta_rs_amd import ceremony, keygen, synth

pytestmark = pytest.mark.gpu

_BLOCKS = {}


class _Block:
    pass


def _lim(curve, k):
    return synth.ints_to_limbs([k % synth.FR_MODULUS[curve]], 4)[0]


def _proof_bytes(gpu, curve, row):
    w1 = gpu.affine_limbs(curve, 1)
    return (gpu.point_serialize(curve, 1, row[:w1]) + gpu.point_serialize(curve, 2, row[w1:3 * w1]) +
            gpu.point_serialize(curve, 1, row[3 * w1:]))


def _block(gpu, curve):
    """seven proofs of seven assignments of one circuit (one with r = 0), rows 1 and 3..6 spoiled; the single call's verdicts
    and the oracle's are computed once and shared"""
    if curve in _BLOCKS:
        return _BLOCKS[curve]
    b = _Block()
    c = synth.make_circuit(curve, 600, 420, 7, seed=1900 + curve)
    r = synth.FR_MODULUS[curve]
    g1 = O.g_mul(curve, 1, keygen.generator(curve, 1), _lim(curve, 0xabcdef))
    g2 = O.g_mul(curve, 2, keygen.generator(curve, 2), _lim(curve, 0x123457))
    b.pk = keygen.generate(c, synth.from_mont(H.toxic(curve, seed=41), r), g1, g2)
    ctx = gpu.ProvingContext(curve, b.pk)
    ctx.set_r1cs(gpu.R1CS.from_circuit(c))
    b.vctx = gpu.VerifyingContext(curve, b.pk)
    rs = H.rand_fr_mont(curve, 15, seed=196)
    R = synth.Reassigner(c)
    cs = [R.assign(8100 + q) for q in range(7)]
    b.inputs = np.stack([x.z[1:c.P] for x in cs])
    rows = []
    for q, x in enumerate(cs):
        r_ = np.zeros(4, np.uint64) if q == 2 else rs[2 * q]
        rows.append(gpu.proof_decode(curve, gpu.Groth16.prove_with_randomness(ctx, x.z, r_, rs[2 * q + 1])))
    b.rows = np.stack(rows)
    w1 = gpu.affine_limbs(curve, 1)
    b.inputs[1, 2] = rs[14]                                                      # row 1: one public input replaced
    for row, sl, g in ((3, slice(0, w1), 1), (4, slice(w1, 3 * w1), 2), (5, slice(3 * w1, 4 * w1), 1)):
        b.rows[row, sl] = O.g_mul(curve, g, b.rows[row, sl], _lim(curve, 3))      # rows 3, 4, 5: [3]A, [3]B, [3]C
    b.rows[6] = 0                                                                # row 6: all zeros (as mg_proofs_decode leaves a reject)
    b.single = [gpu.groth16_verify(b.vctx, b.inputs[q], b.rows[q]) for q in range(7)]
    b.oracle = [O.groth16_verify(curve, b.pk, b.inputs[q], _proof_bytes(gpu, curve, b.rows[q])) == 1 for q in range(6)]
    _BLOCKS[curve] = b
    return b


@pytest.mark.parametrize("curve", [0, 1])
def test_verdicts_equal_the_single_call_and_the_oracle(gpu, curve):
    b = _block(gpu, curve)
    got = gpu.groth16_verify_each(b.vctx, b.inputs, b.rows)
    assert got.dtype == bool and got.shape == (7,)
    assert got.tolist() == b.single
    assert got[:6].tolist() == b.oracle == [True, False, True, False, False, False]
    for pick in ([0], [3], [0, 1, 2]):                                           # k = 1 (a good row, a bad row) and k = 3
        got = gpu.groth16_verify_each(b.vctx, b.inputs[pick], b.rows[pick])
        assert got.tolist() == [b.single[q] for q in pick], pick
    # proof bytes are taken like decoded rows
    as_bytes = [_proof_bytes(gpu, curve, b.rows[q]) for q in (0, 1, 2)]
    assert gpu.groth16_verify_each(b.vctx, b.inputs[:3], as_bytes).tolist() == b.single[:3]


def test_key_without_public_inputs(gpu):
    """P = 1: no MSM, every prepared-inputs point is gamma_abc_g1[0]"""
    curve = 0
    c = synth.make_circuit(curve, 64, 40, 1, seed=1950)
    pk = keygen.generate(c, synth.from_mont(H.toxic(curve, seed=42), synth.FR_MODULUS[curve]))
    ctx = gpu.ProvingContext(curve, pk)
    ctx.set_r1cs(gpu.R1CS.from_circuit(c))
    vctx = gpu.VerifyingContext(curve, pk)
    rs = H.rand_fr_mont(curve, 6, seed=197)
    R = synth.Reassigner(c)
    rows = np.stack([gpu.proof_decode(curve, gpu.Groth16.prove_with_randomness(ctx, R.assign(8200 + q).z, rs[2 * q], rs[2 * q + 1]))
                     for q in range(3)])
    w1 = gpu.affine_limbs(curve, 1)
    rows[1, 3 * w1:] = O.g_mul(curve, 1, rows[1, 3 * w1:], _lim(curve, 3))
    none = np.zeros((0, 4), dtype=np.uint64)
    single = [gpu.groth16_verify(vctx, none, rows[q]) for q in range(3)]
    assert single == [True, False, True]
    assert gpu.groth16_verify_each(vctx, None, rows).tolist() == single
    assert gpu.groth16_verify_each(vctx, np.zeros((3, 0, 4), dtype=np.uint64), rows).tolist() == single


def test_across_the_chunk_boundary(gpu):
    """VERIFY_EACH_CHUNK + 1 rows: the last one is alone in its chunk and carries its own verdict"""
    b = _block(gpu, 0)
    k = gpu.VERIFY_EACH_CHUNK + 1
    idx = np.arange(k) % 7
    got = gpu.groth16_verify_each(b.vctx, b.inputs[idx], b.rows[idx])
    want = np.array(b.single)[idx]
    assert got.shape == (k,) and (got == want).all(), np.nonzero(got != want)[0][:10]
    assert want[-1] == b.single[(k - 1) % 7]
    # shifted by two, so that the lone row of the last chunk is one with the opposite verdict
    idx2 = (np.arange(k) + 2) % 7
    assert bool(want[-1]) != b.single[idx2[-1]]
    got2 = gpu.groth16_verify_each(b.vctx, b.inputs[idx2], b.rows[idx2])
    assert (got2 == np.array(b.single)[idx2]).all()


def _pairing_groups(curve):
    """eight groups of two pairs: five of the form ((aG, bH), (-abG, H)), two with a wrong scalar, one with an infinity member on
    each side"""
    G, Hh = O.generator(curve, 1), O.generator(curve, 2)
    g1s, g2s = [], []
    for t, (a, bb, ab) in enumerate([(2, 3, 6), (5, 7, 35), (11, 13, 143), (17, 19, 323), (23, 29, 667), (3, 5, 16), (7, 11, 76)]):
        g1s.append(np.stack([O.g_mul(curve, 1, G, _lim(curve, a)), ceremony.g1_neg(curve, O.g_mul(curve, 1, G, _lim(curve, ab)))]))
        g2s.append(np.stack([O.g_mul(curve, 2, Hh, _lim(curve, bb)), Hh]))
    g1s.append(np.stack([np.zeros_like(G), G]))
    g2s.append(np.stack([Hh, np.zeros_like(Hh)]))
    return np.stack(g1s), np.stack(g2s)


@pytest.mark.parametrize("curve", [0, 1])
def test_pairing_check_each(gpu, curve):
    g1, g2 = _pairing_groups(curve)
    single = [gpu.pairing_check(curve, g1[t], g2[t]) for t in range(g1.shape[0])]
    assert single == [True] * 5 + [False, False, True]
    assert gpu.pairing_check_each(curve, g1, g2).tolist() == single
    if curve == 0:  # across the chunk boundary
        n = gpu.VERIFY_EACH_CHUNK + 1
        idx = (np.arange(n) + 5) % 8                       # the lone group of the last chunk is a false one
        assert single[idx[-1]] is False
        got = gpu.pairing_check_each(curve, g1[idx], g2[idx])
        assert (got == np.array(single)[idx]).all()
    # groups of three: e(2G, 3H) e(5G, 7H) e(-41G, H) = 1, and the same with -42G
    G, Hh = O.generator(curve, 1), O.generator(curve, 2)
    mul1 = lambda k: O.g_mul(curve, 1, G, _lim(curve, k))
    mul2 = lambda k: O.g_mul(curve, 2, Hh, _lim(curve, k))
    t1 = np.stack([np.stack([mul1(2), mul1(5), ceremony.g1_neg(curve, mul1(k))]) for k in (41, 42)])
    t2 = np.stack([np.stack([mul2(3), mul2(7), Hh])] * 2)
    assert [gpu.pairing_check(curve, t1[t], t2[t]) for t in range(2)] == [True, False]
    assert gpu.pairing_check_each(curve, t1, t2).tolist() == [True, False]
    # groups of one: e(O, H) = 1, e(G, H) != 1
    o1 = np.stack([np.zeros_like(G), G]).reshape(2, 1, -1)
    o2 = np.stack([Hh, Hh]).reshape(2, 1, -1)
    assert gpu.pairing_check_each(curve, o1, o2).tolist() == [True, False]
    # ceremony.same_each agrees with ceremony.same
    pairs = [((g1[t, 0], g2[t, 0]), (ceremony.g1_neg(curve, g1[t, 1]), g2[t, 1])) for t in (0, 4, 5, 6)]
    want = [ceremony.same(curve, *p) for p in pairs]
    assert want == [True, True, False, False]
    assert ceremony.same_each(curve, pairs).tolist() == want


def test_arguments(gpu):
    b = _block(gpu, 0)
    sentinel = np.full(8, 0xA5, dtype=np.uint8)
    assert gpu.groth16_verify_each(b.vctx, b.inputs[:0], b.rows[:0], out=sentinel).shape == (0,)
    g1, g2 = _pairing_groups(0)
    assert gpu.pairing_check_each(0, g1[:0], g2[:0], out=sentinel).shape == (0,)
    assert (sentinel == 0xA5).all()
    for g in (0, 65):
        with pytest.raises(gpu.MantaGpuError):
            gpu.pairing_check_each(0, np.zeros((2, g, g1.shape[2]), np.uint64), np.zeros((2, g, g2.shape[2]), np.uint64), out=sentinel)
    assert (sentinel == 0xA5).all()
    with pytest.raises(ValueError):
        gpu.groth16_verify_each(b.vctx, b.inputs[:, :-1], b.rows)
    with pytest.raises(ValueError):
        gpu.pairing_check_each(0, g1, g2[:-1])
    # after the refused calls the next valid ones still answer correctly
    assert gpu.groth16_verify_each(b.vctx, b.inputs, b.rows, out=sentinel).tolist() == b.single
    assert sentinel[:7].tolist() == [int(v) for v in b.single] and sentinel[7] == 0xA5
    assert gpu.pairing_check_each(0, g1, g2).tolist() == [True] * 5 + [False, False, True]


def test_from_several_threads_beside_a_batch_check(gpu):
    b = _block(gpu, 0)
    res, errs = [[] for _ in range(3)], []

    def job(t):
        try:
            for _ in range(4):
                res[t].append(gpu.groth16_verify_each(b.vctx, b.inputs, b.rows).tolist())
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errs.append(e)

    threads = [threading.Thread(target=job, args=(t,)) for t in range(3)]
    for th in threads:
        th.start()
    rnd = np.random.RandomState(6).randint(1, 1 << 62, size=(2, 2)).astype(np.uint64)
    batch = [gpu.groth16_verify_batch(b.vctx, b.inputs[[0, 2]], list(b.rows[[0, 2]]), rnd) for _ in range(4)]
    for th in threads:
        th.join()
    assert not errs, errs
    assert all(len(r) == 4 and all(v == b.single for v in r) for r in res)
    assert batch == [True] * 4
