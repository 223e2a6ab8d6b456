"""GPU tests of the AES-GCM notes (mg_light_notes_*, mg_outgoing_notes_*), the address partition and the Merkle shard index, byte
for byte and status for status against the pure-Python restatement of tests/light_note_ref.py. A scalar multiplication of the
model costs about 8 ms, so the batches are built on walks: with the keys rk_i = rk_0 + i D and a handful of randomness values r,
the agreed points r rk_i = r rk_0 + i (r D) cost one model addition each, and with one key rk and the randomness r_i = r_0 + i d
the agreed points r_i rk and the ephemeral keys r_i G do. The model's cipher takes about 4 ms a note; each batch is sealed by
the model once and shared by the tests that use it."""
import functools
import random
import threading

import numpy as np
import pytest

import edwards_ref as E
import light_note_ref as N
import utxo_ref as U
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu

R, L = N.R, N.L
G = E.generator()
FILES = [U.read(n) for n in U.FILES]
KINDS = ("light", "outgoing")
FIELDS = {"light": 3, "outgoing": 2}
SEALED = {"light": N.LIGHT_SEALED, "outgoing": N.OUTGOING_SEALED}
SEAL = {"light": N.light_seal, "outgoing": N.outgoing_seal}
UNSEAL = {"light": N.light_unseal, "outgoing": N.outgoing_unseal}
TO_BYTES = {"light": N.light_bytes, "outgoing": N.outgoing_bytes}
CHUNK = 1 << 16  # MG_EDWARDS_CHUNK


def mont_points(points):
    return synth.to_mont([c for p in points for c in p], R, 4).reshape(len(points), 8)


def mont_fields(rows, kind):
    return synth.to_mont([v for row in rows for v in row], R, 4).reshape(len(rows), FIELDS[kind], 4)


def scalars(vals):
    return synth.ints_to_limbs(vals, 4)


def notes_array(notes, kind):
    """sealed notes, None where a lane is refused -> [n, bytes] uint8 with zeros there"""
    joined = b"".join(bytes(SEALED[kind]) if x is None else x for x in notes)
    return np.frombuffer(joined, dtype=np.uint8).reshape(len(notes), SEALED[kind])


def walk(start, step, n):
    out, p = [], start
    for _ in range(n):
        out.append(p)
        p = E.add(p, step)
    return out


def rand_fields(rng, kind):
    return [rng.randrange(R) for _ in range(FIELDS[kind] - 1)] + [rng.randrange(N.U128)]


@pytest.fixture(scope="module")
def model(gpu):
    m = gpu.UtxoModel(*FILES)
    yield m
    m.close()


# ---- sealing ----------------------------------------------------------------------------------------------------------------
EDGE_VALUES = [0, N.U128 - 1, N.U128, R - 1]  # the last two are no u128: MG_NOTE_BAD_VALUE and zeros
SIZES = [0, 1, 63, 64, 65, 257]  # nothing, one lane, a wave and its neighbours, a block of 256 and one more


def edge_fields(rng, kind, i):
    """lanes 1..8: the value at 0, 2^128 - 1, 2^128 and r - 1; then randomness / id at 0 and r - 1"""
    f = rand_fields(rng, kind)
    if 1 <= i <= 4:
        f[-1] = EDGE_VALUES[i - 1]
    elif 5 <= i <= 8:
        f[(i - 5) % (len(f) - 1)] = 0 if i < 7 else R - 1
    return f


@functools.lru_cache(maxsize=None)
def light_batch():
    """257 light notes to 257 receiving keys under four randomness values (0 and l - 1 among them); lane 9's key is the identity.
    -> (keys, randomness, plaintexts, the model's epks / notes / statuses)"""
    rng = random.Random(301)
    n = 257
    rs = [rng.randrange(1, L), rng.randrange(1, L), 0, L - 1]
    rk0, d = E.mul(G, rng.randrange(1, L)), E.mul(G, rng.randrange(1, L))
    keys = walk(rk0, d, n)
    agreed = [walk(E.mul(rk0, r), E.mul(d, r), n) for r in rs]
    epk = [E.mul(G, r) for r in rs]
    keys[9] = E.IDENTITY
    rand = [rs[i % 4] for i in range(n)]
    plain = [edge_fields(rng, "light", i) for i in range(n)]
    sealed = [N.light_seal(E.IDENTITY if i == 9 else agreed[i % 4][i], plain[i]) for i in range(n)]
    assert N.light_encrypt(G, keys[5], rand[5], plain[5]) == (epk[5 % 4], sealed[5][0], N.OK)  # the walk against the plain model
    epks = [epk[i % 4] if st == N.OK else (0, 0) for i, (_, st) in enumerate(sealed)]
    return keys, rand, plain, epks, [x for x, _ in sealed], [st for _, st in sealed]


@functools.lru_cache(maxsize=None)
def outgoing_batch():
    """257 outgoing notes to ONE receiving key under the randomness r_0 + i d, lane 9's randomness 0"""
    rng = random.Random(303)
    n = 257
    rk = E.mul(G, rng.randrange(1, L))
    r0, d = rng.randrange(1, L), rng.randrange(1, L)
    rand = [(r0 + i * d) % L for i in range(n)]
    agreed, epk = walk(E.mul(rk, r0), E.mul(rk, d), n), walk(E.mul(G, r0), E.mul(G, d), n)
    rand[9], agreed[9], epk[9] = 0, E.IDENTITY, E.IDENTITY
    plain = [edge_fields(rng, "outgoing", i) for i in range(n)]
    sealed = [N.outgoing_seal(agreed[i], plain[i]) for i in range(n)]
    assert N.outgoing_encrypt(G, rk, rand[6], plain[6]) == (epk[6], sealed[6][0], N.OK)
    epks = [epk[i] if st == N.OK else (0, 0) for i, (_, st) in enumerate(sealed)]
    return rk, rand, plain, epks, [x for x, _ in sealed], [st for _, st in sealed]


@pytest.mark.parametrize("n", SIZES)
def test_light_encrypt_equals_the_model(gpu, model, n):
    keys, rand, plain, epks, notes, status = (x[:n] for x in light_batch())
    assert n < 5 or (status[3] == status[4] == N.BAD_VALUE and status.count(N.BAD_VALUE) == 2)
    rk, rnd, pt = mont_points(keys), scalars(rand), mont_fields(plain, "light")
    epk, ct, st = model.light_encrypt(rk, rnd, pt)
    assert list(st) == status
    assert (ct == notes_array(notes, "light")).all() and (epk == mont_points(epks)).all()
    none, ct2, st2 = model.light_encrypt(rk, rnd, pt, epks=False)  # epk_out = NULL changes nothing else
    assert none is None and (ct2 == ct).all() and (st2 == st).all()
    if n:  # the ephemeral key is the Poseidon note's
        cipher = gpu.NoteCipher(U.read("incoming-base-encryption-scheme.dat"), mont_points([G]))
        good = st == N.OK
        assert (cipher.encrypt(rk, rnd, pt)[0][good] == epk[good]).all()
        cipher.close()


@pytest.mark.parametrize("n", SIZES)
def test_outgoing_encrypt_equals_the_model(gpu, model, n):
    rk, rand, plain, epks, notes, status = outgoing_batch()
    rand, plain, epks, notes, status = (x[:n] for x in (rand, plain, epks, notes, status))
    assert n < 5 or (status[3] == status[4] == N.BAD_VALUE and status.count(N.BAD_VALUE) == 2)
    epk, ct, st = model.outgoing_encrypt(mont_points([rk]), scalars(rand), mont_fields(plain, "outgoing"))
    assert list(st) == status
    assert (ct == notes_array(notes, "outgoing")).all() and (epk == mont_points(epks)).all()


def test_the_identity_as_the_outgoing_receiving_key(gpu, model):
    """every agreed point is the identity, whose encoding is 32 zero bytes: all notes share one key, the ephemeral keys differ"""
    rng = random.Random(305)
    rand = [rng.randrange(L) for _ in range(5)]
    plain = [rand_fields(rng, "outgoing") for _ in rand]
    epk, ct, st = model.outgoing_encrypt(mont_points([E.IDENTITY]), scalars(rand), mont_fields(plain, "outgoing"))
    assert not st.any() and (epk == mont_points([E.mul(G, r) for r in rand])).all()
    assert (ct == notes_array([N.outgoing_seal(E.IDENTITY, f)[0] for f in plain], "outgoing")).all()


# ---- opening ----------------------------------------------------------------------------------------------------------------
BAD_LANES = {3: "a flipped body bit", 64: "a flipped tag bit", 65: "a wrong epk", 100: "a note for another viewing key",
             129: "an id of r behind a valid tag"}


@functools.lru_cache(maxsize=None)
def open_batch(kind):
    """130 notes to the address of one viewing key, five of them spoiled as BAD_LANES says -> (vk, epks, notes, the model's
    plaintexts / statuses)"""
    rng = random.Random(307 + len(kind))
    n = 130
    vk, other_vk = rng.randrange(1, L), rng.randrange(1, L)
    rk = E.mul(G, vk)
    r0, d = rng.randrange(1, L), rng.randrange(1, L)
    agreed, epks = walk(E.mul(rk, r0), E.mul(rk, d), n), walk(E.mul(G, r0), E.mul(G, d), n)
    plain = [rand_fields(rng, kind) for _ in range(n)]
    plain[0][-1], plain[1][-1], plain[2][0], plain[5][0] = 0, N.U128 - 1, 0, R - 1
    notes = [bytearray(SEAL[kind](a, f)[0]) for a, f in zip(agreed, plain)]
    body = SEALED[kind] - 16
    notes[3][body // 2] ^= 0x04
    notes[64][body + 9] ^= 0x80
    epks[65] = epks[66]
    notes[100] = bytearray(SEAL[kind](E.mul(E.mul(G, other_vk), (r0 + 100 * d) % L), plain[100])[0])
    forged = list(plain[129])
    forged[-2] = R  # the id: the field in front of the value
    notes[129] = bytearray(N.gcm_encrypt(N.note_key(agreed[129]), N.NONCE, TO_BYTES[kind](forged)))
    want = []
    for i in range(n):
        a = E.mul(epks[i], vk) if i in BAD_LANES else agreed[i]
        want.append(UNSEAL[kind](a, bytes(notes[i])))
    assert E.mul(epks[7], vk) == agreed[7]
    return vk, epks, [bytes(x) for x in notes], [f for f, _ in want], [st for _, st in want]


@pytest.mark.parametrize("kind", KINDS)
def test_open_rejects_exactly_the_bad_lanes(gpu, model, kind):
    vk, epks, notes, fields, status = open_batch(kind)
    n = len(notes)
    assert {i: status[i] for i in range(n) if status[i]} == {3: N.BAD_TAG, 64: N.BAD_TAG, 65: N.BAD_TAG, 100: N.BAD_TAG,
                                                             129: N.BAD_VALUE}
    ep, ct = mont_points(epks), notes_array(notes, kind)
    if kind == "light":
        pt, ok, st, tried = model.light_open(scalars([vk])[0], ep, ct)
        assert tried == n
    else:
        pt, ok, st = model.outgoing_open(scalars([vk])[0], ep, ct)
    assert list(st) == status and list(ok) == [s == N.OK for s in status]
    want = mont_fields([f if f is not None else [0] * FIELDS[kind] for f in fields], kind)
    assert (pt == want).all() and not pt[[3, 64, 65, 100, 129]].any()
    # status = NULL is accepted
    p, sz = gpu._p, gpu._sz
    vkl, pt2, ok2 = scalars([vk])[0], np.zeros_like(pt), np.zeros(n, dtype=np.uint8)
    if kind == "light":
        rc = gpu.LIB.mg_light_notes_open(model._h, p(vkl), p(ep), p(ct), None, sz(n), p(pt2), p(ok2), None, None)
    else:
        rc = gpu.LIB.mg_outgoing_notes_open(model._h, p(vkl), p(ep), p(ct), sz(n), p(pt2), p(ok2), None)
    assert rc == 0 and (pt2 == pt).all() and (ok2.astype(bool) == ok).all()


# ---- the address partition, the shard index, and the scan behind them ----------------------------------------------------------
def test_address_partitions_equal_the_model(gpu, model):
    rng = random.Random(311)
    keys = walk(E.mul(G, rng.randrange(1, L)), E.mul(G, rng.randrange(1, L)), 255) + [E.IDENTITY, G]
    assert len(keys) == 257
    got = model.address_partitions(mont_points(keys))
    assert list(got) == [N.address_partition(k) for k in keys]
    assert len(set(got)) > 100  # a hash, not a constant


def test_merkle_shard_indices_equal_the_model(gpu):
    rng = random.Random(313)
    leaves = [0, R - 1, 1, (1 << 255) % R] + [rng.randrange(R) for _ in range(253)]
    assert len(leaves) == 257
    got = gpu.merkle_shard_indices(synth.to_mont(leaves, R, 4))
    assert list(got) == [N.merkle_shard(v) for v in leaves]


@functools.lru_cache(maxsize=None)
def ledger():
    """1 000 ledger notes of which 13 are sealed to the wallet's address or made to look so:
      9 carry the wallet's byte: 7 open, one has a flipped tag bit, one is sealed to another key
      3 would open but carry another byte
    and 988 are other people's notes (random bytes under ephemeral keys off a walk) carrying other bytes."""
    rng = random.Random(317)
    n = 1000
    vk = rng.randrange(1, L)
    rk = E.mul(G, vk)
    mine = N.address_partition(rk)
    special = rng.sample(range(n), 12)
    opens, bad_tag, other_key, wrong_byte = special[:7], special[7], special[8], special[9:]
    e0, step = E.mul(G, rng.randrange(1, L)), E.mul(G, rng.randrange(1, L))
    epks = walk(e0, step, n)  # the agreed point of lane i with the wallet is vk e_0 + i (vk step)
    agreed = walk(E.mul(e0, vk), E.mul(step, vk), n)
    notes = [rng.randbytes(N.LIGHT_SEALED) for _ in range(n)]
    parts = [rng.choice([b for b in range(256) if b != mine]) for _ in range(n)]
    fields = {}
    for i in opens + [bad_tag] + wrong_byte:
        fields[i] = rand_fields(rng, "light")
        notes[i] = N.light_seal(agreed[i], fields[i])[0]
    flipped = bytearray(notes[bad_tag])
    flipped[-1] ^= 1
    notes[bad_tag] = bytes(flipped)
    notes[other_key] = N.light_seal(E.mul(epks[other_key], rng.randrange(1, L)), rand_fields(rng, "light"))[0]
    for i in opens + [bad_tag, other_key]:
        parts[i] = mine
    sample = [i for i in range(n) if i not in special][::25]  # the model on 40 of the 988: random bytes carry no valid tag
    assert len(sample) == 40 and all(N.light_unseal(agreed[i], notes[i]) == (None, N.BAD_TAG) for i in sample)
    assert N.light_unseal(agreed[bad_tag], notes[bad_tag])[1] == N.light_unseal(agreed[other_key], notes[other_key])[1] == N.BAD_TAG
    assert all(N.light_unseal(agreed[i], notes[i]) == (fields[i], N.OK) for i in opens + wrong_byte)
    return vk, epks, notes, parts, sorted(opens), bad_tag, other_key, sorted(wrong_byte), fields


def test_scan_tries_only_the_wallets_partition(gpu, model):
    vk, epks, notes, parts, opens, bad_tag, other_key, wrong_byte, fields = ledger()
    n = len(notes)
    vkl, ep, ct = scalars([vk])[0], mont_points(epks), notes_array(notes, "light")
    parts = np.array(parts, dtype=np.uint8)
    assert model.address_partitions(mont_points([E.mul(G, vk)]))[0] == parts[opens[0]] and (parts == parts[opens[0]]).sum() == 9
    pt, ok, st, tried = model.light_open(vkl, ep, ct, partitions=parts)
    assert tried == 9
    want = np.full(n, N.OTHER_PARTITION, dtype=np.uint8)
    want[opens], want[[bad_tag, other_key]] = N.OK, N.BAD_TAG
    assert (st == want).all() and [i for i in range(n) if ok[i]] == opens
    want_pt = np.zeros((n, 3, 4), dtype=np.uint64)
    want_pt[opens] = mont_fields([fields[i] for i in opens], "light")
    assert (pt == want_pt).all()  # zeros everywhere else, the three notes with a wrong byte included
    # partitions = NULL: every lane goes through the key agreement, and the three open too
    pt, ok, st, tried = model.light_open(vkl, ep, ct)
    assert tried == n
    all_open = sorted(opens + wrong_byte)
    assert len(all_open) == 10 and [i for i in range(n) if ok[i]] == all_open
    assert (np.delete(st, all_open) == N.BAD_TAG).all() and not st[all_open].any()
    want_pt[wrong_byte] = mont_fields([fields[i] for i in wrong_byte], "light")
    assert (pt == want_pt).all()


# ---- more than one device pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_open_of_encrypt_across_the_pass_boundary(gpu, model, kind):
    """n = MG_EDWARDS_CHUNK + 1: the second pass holds one lane. Open-of-encrypt is the identity on every lane; 32 lanes, the last
    of the first pass and the first of the second among them, are the model's."""
    n = CHUNK + 1
    rng = random.Random(331 + len(kind))
    vk = rng.randrange(1, L)
    rk = E.mul(G, vk)
    raw = np.frombuffer(rng.randbytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
    raw[:, 3] &= np.uint64((1 << 56) - 1)  # below 2^248 < l
    rand = synth.limbs_to_ints(raw)
    nf = FIELDS[kind]
    plain = np.frombuffer(rng.randbytes(32 * nf * n), dtype=np.uint64).reshape(n, nf, 4).copy()
    plain[:, :, 3] &= np.uint64((1 << 60) - 1)  # reduced Montgomery words of whatever elements
    values = [rng.randrange(N.U128) for _ in range(n)]
    plain[:, nf - 1] = synth.to_mont(values, R, 4)
    if kind == "light":
        epk, ct, st = model.light_encrypt(np.tile(mont_points([rk]), (n, 1)), raw, plain)
        pt, ok, st2, tried = model.light_open(scalars([vk])[0], epk, ct)
        assert tried == n
    else:
        epk, ct, st = model.outgoing_encrypt(mont_points([rk]), raw, plain)
        pt, ok, st2 = model.outgoing_open(scalars([vk])[0], epk, ct)
    assert not st.any() and not st2.any() and ok.all() and (pt == plain).all()
    for i in [0, CHUNK - 1, CHUNK] + rng.sample(range(1, CHUNK - 1), 29):
        fields = synth.from_mont(plain[i], R)
        assert fields[-1] == values[i]
        want_epk, want_note, _ = (N.light_encrypt if kind == "light" else N.outgoing_encrypt)(G, rk, rand[i], fields)
        assert bytes(ct[i]) == want_note and (epk[i] == mont_points([want_epk])[0]).all(), i


# ---- two host threads ------------------------------------------------------------------------------------------------------------
def test_two_threads_run_different_calls_at_once(gpu, model):
    keys, rand, plain, _, _, _ = light_batch()
    vk, epks, notes, _, _ = open_batch("outgoing")
    rk, rnd, pt = mont_points(keys), scalars(rand), mont_fields(plain, "light")
    vkl, ep, ct = scalars([vk])[0], mont_points(epks), notes_array(notes, "outgoing")
    seal = lambda: model.light_encrypt(rk, rnd, pt)
    scan = lambda: (model.outgoing_open(vkl, ep, ct), model.address_partitions(rk))
    want_seal, want_scan = seal(), scan()
    got, errors = {}, []

    def run(name, call):
        try:
            got[name] = [call() for _ in range(4)]
        except Exception as e:  # a thread's exception would otherwise be lost
            errors.append(e)

    threads = [threading.Thread(target=run, args=("seal", seal)), threading.Thread(target=run, args=("scan", scan))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for res in got["seal"]:
        assert all((a == b).all() for a, b in zip(res, want_seal))
    for (opened, parts) in got["scan"]:
        assert all((a == b).all() for a, b in zip(opened, want_scan[0])) and (parts == want_scan[1]).all()
