"""GPU tests of the batched Schnorr authorization signatures (mg_schnorr_challenges, mg_signatures_verify, mg_signatures_sign),
limb for limb and status for status against the pure-Python restatement of tests/schnorr_ref.py (hashlib's Blake2s, the affine
curve of tests/edwards_ref.py). A scalar multiplication of the model costs about 8 ms, so keys and nonce points come from walks
(one model addition each: pk_i = pk_0 + i D for sk_i = sk_0 + i d), the model verifies a few dozen distinct lanes once, and the
larger batches tile them."""
import ctypes
import functools
import random

import numpy as np
import pytest

import edwards_ref as E
import schnorr_ref as S
import utxo_ref as U
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu

R, L = S.R, S.L
G = E.generator()
FILES = [U.read(n) for n in U.FILES]
EDGE_LENGTHS = [0, 1, 2, 3, 35, 36, 37, 99, 100, 101]  # streams of 92, 93..95, 127 / 128 / 129 and 191 / 192 / 193 bytes
STRIDE = 304  # the rows of the small batches: a multiple of 4 that holds 300 bytes
MAX = 1 << 16  # MG_SIGNATURE_MAX_MESSAGE
SIZES = [1, 63, 64, 65, 257]


def mont_points(points):
    return synth.to_mont([c for p in points for c in p], R, 4).reshape(-1, 8)


def scalars(vals):
    return synth.ints_to_limbs(vals, 4)


def key_walk(n, seed):
    """n pairs (scalar, scalar * G) with the scalars in an arithmetic progression: one model addition per pair"""
    rng = random.Random(seed)
    k, d = rng.randrange(1, L), rng.randrange(1, L)
    p, step = E.mul(G, k), E.mul(G, d)
    out = []
    for _ in range(n):
        out.append((k, p))
        k, p = (k + d) % L, E.add(p, step)
    return out


def rows(messages, stride, seed):
    """messages -> ([n, stride] uint8 with garbage behind each message, lengths [n] uint32)"""
    buf = np.frombuffer(random.Random(seed).randbytes(len(messages) * stride), dtype=np.uint8).reshape(len(messages), stride).copy()
    for i, m in enumerate(messages):
        buf[i, :len(m)] = np.frombuffer(m, dtype=np.uint8)
    return buf, np.array([len(m) for m in messages], dtype=np.uint32)


@pytest.fixture(scope="module")
def model(gpu):
    m = gpu.UtxoModel(*FILES)
    yield m
    m.close()


# ---- challenges -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def challenge_lanes():
    """one wave of 64 lanes with 64 different lengths between 0 and 300, then the edge lengths; lane 5's pk and lane 6's R are
    the identity"""
    rng = random.Random(201)
    lengths = [0, 300] + rng.sample(range(1, 300), 62)
    lengths += EDGE_LENGTHS
    n = len(lengths)
    pks, rps = [p for _, p in key_walk(n, 203)], [p for _, p in key_walk(n, 205)]
    pks[5], rps[6] = E.IDENTITY, E.IDENTITY
    msgs = [rng.randbytes(k) for k in lengths]
    return pks, rps, msgs, [S.challenge(pk, rp, m) for pk, rp, m in zip(pks, rps, msgs)]


def test_challenges_equal_the_model(gpu, model):
    pks, rps, msgs, want = challenge_lanes()
    assert len({len(m) for m in msgs[:64]}) == 64 and [len(m) for m in msgs[64:]] == EDGE_LENGTHS
    pk, rp = mont_points(pks), mont_points(rps)
    buf, lens = rows(msgs, STRIDE, seed=1)
    got = model.schnorr_challenges(pk, rp, buf, lens)
    assert synth.limbs_to_ints(got) == want
    other, _ = rows(msgs, STRIDE, seed=2)  # other garbage behind every message: nothing changes
    assert (other != buf).any() and (model.schnorr_challenges(pk, rp, other, lens) == got).all()
    for n in (1, 63, 65):
        assert (model.schnorr_challenges(pk[:n], rp[:n], buf[:n], lens[:n]) == got[:n]).all(), n


@pytest.mark.parametrize("stride", [0, 4, 36, 100, 2048])
def test_challenges_without_lengths_hash_the_whole_row(gpu, model, stride):
    pks, rps, _, _ = challenge_lanes()
    n = 70
    rng = random.Random(207 + stride)
    msgs = [rng.randbytes(stride) for _ in range(n)]
    buf = np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(n, stride)
    got = model.schnorr_challenges(mont_points(pks[:n]), mont_points(rps[:n]), buf)
    assert synth.limbs_to_ints(got) == [S.challenge(pk, rp, m) for pk, rp, m in zip(pks, rps, msgs)]


# ---- verification -----------------------------------------------------------------------------------------------------------
def raw(point):
    """an affine point as the 8 limbs the device reads"""
    return mont_points([point])[0]


@functools.lru_cache(maxsize=None)
def base():
    """The distinct lanes of the verification tests, each (pk limbs, R limbs, s, message, the model's status, what it is). The
    model sees the integers the limbs stand for; a coordinate of p or more is given to it as such."""
    rng = random.Random(211)
    n_valid = 24
    keys, nonces = key_walk(n_valid + 2, 213), key_walk(n_valid + 2, 215)
    lengths = EDGE_LENGTHS + [300, 64, 28, 220] + [rng.randrange(301) for _ in range(10)] + [150, 10]
    assert len(lengths) == n_valid + 2
    sigs = []
    for (sk, pk), (k, rp), ln in zip(keys, nonces, lengths):
        msg = rng.randbytes(ln)
        sigs.append((pk, rp, (k + sk * S.challenge(pk, rp, msg)) % L, msg))
    lanes = [(raw(pk), raw(rp), s, msg, S.verify(G, pk, msg, s, rp), "valid") for pk, rp, s, msg in sigs[:n_valid]]
    assert all(l[4] == S.OK for l in lanes)

    def add(pk, rp, s, msg, what, want, pk_raw=None, rp_raw=None):
        st = S.verify(G, pk, msg, s, rp)
        assert st == want, (what, st)
        lanes.append((raw(pk) if pk_raw is None else pk_raw, raw(rp) if rp_raw is None else rp_raw, s, msg, st, what))

    pk, rp, s, msg = sigs[n_valid]
    flipped = bytearray(msg)
    flipped[len(msg) // 2] ^= 1
    add(pk, rp, s, bytes(flipped), "one message byte altered", S.MISMATCH)
    add(pk, rp, s, msg + b"\0", "a zero byte appended", S.MISMATCH)
    add(pk, rp, (s + 1) % L, msg, "s altered", S.MISMATCH)
    add(pk, E.add(rp, G), s, msg, "R altered", S.MISMATCH)
    add(sigs[0][0], rp, s, msg, "another key's pk", S.MISMATCH)
    assert s + L < 1 << 256  # it satisfies the equation as an integer, and is refused for its encoding
    add(pk, rp, s + L, msg, "s + l", S.BAD_ENCODING)
    big = synth.ints_to_limbs([synth.limbs_to_ints(raw(pk)[:4])[0] + R], 4)[0]
    add((pk[0] + R, pk[1]), rp, s, msg, "pk.x >= p", S.BAD_ENCODING, pk_raw=np.concatenate([big, raw(pk)[4:]]))
    big = synth.ints_to_limbs([synth.limbs_to_ints(raw(rp)[4:])[0] + R], 4)[0]
    add(pk, (rp[0], rp[1] + R), s, msg, "R.y >= p", S.BAD_ENCODING, rp_raw=np.concatenate([raw(rp)[:4], big]))
    zero = np.zeros(8, dtype=np.uint64)
    add((0, 0), rp, s, msg, "pk = (0, 0)", S.BAD_ENCODING, pk_raw=zero)
    add(pk, (0, 0), s, msg, "R = (0, 0)", S.BAD_ENCODING, rp_raw=zero)
    add(pk, (rp[0], (rp[1] + 1) % R), s, msg, "R off the curve", S.BAD_ENCODING)
    (k, rp0) = nonces[n_valid + 1]
    add(E.IDENTITY, rp0, k, msg, "sk = 0", S.DEGENERATE)
    sk, pk1 = keys[n_valid + 1]
    add(pk1, E.IDENTITY, sk * S.challenge(pk1, E.IDENTITY, msg) % L, msg, "k = 0", S.OK)
    order2 = (0, R - 1)  # on the curve, outside the subgroup: the complete law makes the lane well defined
    assert E.on_curve(order2) and not E.in_subgroup(order2)
    lanes.append((raw(order2), raw(rp), s, msg, S.verify(G, order2, msg, s, rp), "pk = (0, -1)"))
    # a signature the order-2 key would accept: h even makes h pk the identity, so (s, R) = (k, k G) satisfies the equation --
    # and is the degenerate case; h odd leaves R + pk != s G
    for t in range(64):
        m2 = msg + bytes([t])
        if S.challenge(order2, rp0, m2) % 2 == 0:
            st = S.verify(G, order2, m2, k, rp0)
            assert st == S.DEGENERATE
            lanes.append((raw(order2), raw(rp0), k, m2, st, "pk = (0, -1), h even"))
            break
    return lanes


def tiled(n, lanes=None, stride=STRIDE, seed=3):
    lanes = lanes or base()
    pick = [lanes[i % len(lanes)] for i in range(n)]
    buf, lens = rows([l[3] for l in pick], stride, seed)
    return (np.stack([l[0] for l in pick]), np.stack([l[1] for l in pick]), scalars([l[2] for l in pick]), buf, lens,
            [l[4] for l in pick])


@pytest.mark.parametrize("n", SIZES)
def test_verify_statuses_equal_the_model(gpu, model, n):
    kinds = {l[5]: l[4] for l in base()}
    assert set(kinds.values()) == {S.OK, S.BAD_ENCODING, S.DEGENERATE, S.MISMATCH} and len(base()) < 63
    pk, rp, sc, buf, lens, want = tiled(n)
    st, n_ok = model.verify_signatures(pk, rp, sc, buf, lens)
    assert list(st) == want, [(i, base()[i % len(base())][5]) for i in range(n) if st[i] != want[i]]
    assert n_ok == want.count(S.OK)
    count = ctypes.c_size_t(0)  # status = NULL is accepted
    p, sz = gpu._p, gpu._sz
    assert gpu.LIB.mg_signatures_verify(model._h, p(pk), p(rp), p(sc), p(buf), sz(STRIDE), p(lens), sz(n), None,
                                        ctypes.byref(count)) == 0
    assert count.value == n_ok
    assert gpu.LIB.mg_signatures_verify(model._h, p(pk), p(rp), p(sc), p(buf), sz(STRIDE), p(lens), sz(n), p(st), None) == 0


def test_verify_across_pass_boundaries(gpu, model):
    """stride = MG_SIGNATURE_MAX_MESSAGE makes a device pass 256 lanes: 600 lanes are three passes, with a bad lane on each
    side of both boundaries and two messages that fill, and all but fill, their rows"""
    n, per_pass = 600, (16 << 20) // MAX
    assert per_pass == 256
    lanes = [l for l in base() if l[5] == "valid"]
    rng = random.Random(217)
    (sk, pk), (k, rp) = key_walk(1, 219)[0], key_walk(1, 221)[0]
    for ln in (MAX, MAX - 3):
        msg = rng.randbytes(ln)
        s = (k + sk * S.challenge(pk, rp, msg)) % L
        lanes.append((raw(pk), raw(rp), s, msg, S.OK, "valid, long"))
    assert S.verify(G, pk, msg, s, rp) == S.OK
    pk_a, rp_a, sc, buf, lens, want = tiled(n, lanes, stride=MAX, seed=5)
    assert want == [S.OK] * n and int(lens.max()) == MAX
    bad = [per_pass - 1, per_pass, 2 * per_pass - 1, 2 * per_pass, n - 1]
    for j, i in enumerate(bad):
        if j % 2:
            sc[i, 0] ^= np.uint64(1)  # s altered
        else:
            rp_a[i] = rp_a[i - 1]  # the neighbour's R
        want[i] = S.MISMATCH
    for i in bad:  # the model on the altered lanes themselves
        got = S.verify(G, tuple(synth.from_mont(pk_a[i].reshape(2, 4), R)), bytes(buf[i, :lens[i]]),
                       synth.limbs_to_ints(sc[i:i + 1])[0], tuple(synth.from_mont(rp_a[i].reshape(2, 4), R)))
        assert got == S.MISMATCH, i
    st, n_ok = model.verify_signatures(pk_a, rp_a, sc, buf, lens)
    assert list(st) == want and n_ok == n - len(bad)


# ---- signing ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signing_lanes():
    rng = random.Random(223)
    pairs = [(L - 1, L - 1), (0, rng.randrange(1, L)), (rng.randrange(1, L), 0), (1, 1), (L - 1, 1)]
    pairs += [(rng.randrange(L), rng.randrange(L)) for _ in range(7)]
    msgs = [rng.randbytes(ln) for ln in [100, 0, 3, 36, 37] + [rng.randrange(301) for _ in range(7)]]
    return pairs, msgs, [S.sign(G, sk, k, m) for (sk, k), m in zip(pairs, msgs)]


def test_sign_equals_the_model_and_verifies(gpu, model):
    pairs, msgs, want = signing_lanes()
    n = len(pairs)
    sk, k = scalars([a for a, _ in pairs]), scalars([b for _, b in pairs])
    buf, lens = rows(msgs, STRIDE, seed=7)
    s, rp, pk = model.sign(sk, k, buf, lens)
    assert synth.limbs_to_ints(s) == [w[0] for w in want]
    assert (rp == mont_points([w[1] for w in want])).all() and (pk == mont_points([w[2] for w in want])).all()
    s2, rp2, none = model.sign(sk, k, buf, lens, pks=False)  # pks_out = NULL
    assert none is None and (s2 == s).all() and (rp2 == rp).all()
    st, n_ok = model.verify_signatures(pk, rp, s, buf, lens)
    model_st = [S.verify(G, w[2], m, w[0], w[1]) for w, m in zip(want, msgs)]
    assert model_st == [S.OK, S.DEGENERATE] + [S.OK] * (n - 2)  # sk = 0 signs what the ledger refuses
    assert list(st) == model_st and n_ok == n - 1


@pytest.mark.parametrize("n", [64, 257])
def test_gpu_signed_batches_verify(gpu, model, n):
    """more lanes than a block, every message the whole row (lengths = NULL); the challenges the signer used are the ones
    mg_schnorr_challenges gives, and s = k + sk h mod l"""
    rng = random.Random(227 + n)
    sks, ks = [rng.randrange(1, L) for _ in range(n)], [rng.randrange(L) for _ in range(n)]
    buf = np.frombuffer(rng.randbytes(n * 128), dtype=np.uint8).reshape(n, 128)
    s, rp, pk = model.sign(scalars(sks), scalars(ks), buf)
    h = synth.limbs_to_ints(model.schnorr_challenges(pk, rp, buf))
    assert synth.limbs_to_ints(s) == [(k + sk * hh) % L for sk, k, hh in zip(sks, ks, h)]
    st, n_ok = model.verify_signatures(pk, rp, s, buf)
    assert not st.any() and n_ok == n
    buf2 = buf.copy()
    buf2[n // 2, 127] ^= 0x80  # the last byte of one row
    st, n_ok = model.verify_signatures(pk, rp, s, buf2)
    assert [i for i in range(n) if st[i]] == [n // 2] and st[n // 2] == S.MISMATCH and n_ok == n - 1
