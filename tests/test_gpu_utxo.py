"""GPU tests of the batched UTXO derivation (mg_utxos_mint, mg_utxos_open, mg_viewing_keys), limb for limb against the
pure-Python restatement of tests/utxo_ref.py (pinned to the reference's parameter files by test_utxo_host.py). The model costs
about 5 ms per UTXO, so one set of 257 lanes is computed once and shared; the batch across a chunk boundary is checked whole
through the independent route of three `PoseidonHasher.hash` calls with numpy glue, and on 256 sampled lanes against the model."""
import functools
import random
import threading

import numpy as np
import pytest

import edwards_ref as E
import poseidon_ref as P
import utxo_ref as U
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu

R, L, U128 = U.R, U.L, U.U128
MODEL = U.Model()
G = MODEL.g
FILES = [U.read(n) for n in U.FILES]
CHUNK = 1 << 16
POSEIDON_BLOCK = 256  # lanes per block of the Poseidon and UTXO kernels
SIZES = [1, 63, 64, 65, POSEIDON_BLOCK + 1]
N = max(SIZES)


def mont(vals):
    return synth.to_mont([int(v) for v in vals], R, 4)


def ints(arr):
    return synth.from_mont(np.asarray(arr, dtype=np.uint64).reshape(-1, 4), R)


def mont_points(points):
    return mont([c for p in points for c in p]).reshape(-1, 8)


def mont_rows(rows, width):
    return mont([w for r in rows for w in r]).reshape(-1, width, 4)


def walk(n, seed):
    """n distinct subgroup points by a walk P, P + H, P + 2H, ..: one model addition each"""
    rng = random.Random(seed)
    p, h = E.mul(G, rng.randrange(1, L)), E.mul(G, rng.randrange(1, L))
    out = []
    for _ in range(n):
        out.append(p)
        p = E.add(p, h)
    return out


def rows_or_zeros(rows, width):
    """model outputs (a row of ints, or None for a lane that is not OK) -> [n, width, 4] Montgomery, zeros for None"""
    return mont_rows([r if r is not None else (0,) * width for r in rows], width)


@functools.lru_cache(maxsize=None)
def batch():
    """N lanes with the edge cases first: both flags; asset value 0 and 2^128 - 1; id r - 1; randomness 0"""
    rng = random.Random(101)
    plain = [(rng.randrange(R), rng.randrange(R), rng.randrange(U128)) for _ in range(N)]
    flags = [rng.randrange(2) for _ in range(N)]
    plain[0], flags[0] = (0, R - 1, U128 - 1), 0
    plain[1], flags[1] = (0, R - 1, U128 - 1), 1
    plain[2], flags[2] = (rng.randrange(R), 0, 0), 0
    plain[3], flags[3] = (rng.randrange(R), 0, 0), 1
    plain[4], flags[4] = (R - 1, 1, 1), 1
    plain[5], flags[5] = (1, R - 1, 0), 0
    return plain, flags


@functools.lru_cache(maxsize=None)
def keys():
    """per-lane receiving keys (the identity first), the address of the opening tests and the authorization key"""
    rks = [E.IDENTITY] + walk(N - 1, seed=103)
    vk = random.Random(107).randrange(1, L)
    return rks, vk, MODEL.receiving_key(vk), walk(1, seed=109)[0]


@functools.lru_cache(maxsize=None)
def minted(shared_key):
    """the model's mint of every lane, to per-lane keys or all to the address"""
    plain, flags = batch()
    rks, _, addr, _ = keys()
    return [MODEL.mint(addr if shared_key else rks[i], plain[i], flags[i]) for i in range(N)]


@pytest.fixture(scope="module")
def model(gpu):
    m = gpu.UtxoModel(*FILES)
    yield m
    m.close()


@pytest.mark.parametrize("n", SIZES)
def test_mint_matches_the_model(gpu, model, n):
    plain, flags = batch()
    rks = keys()[0]
    utxos, items, st = model.mint(mont_points(rks[:n]), mont_rows(plain[:n], 3), flags[:n])
    want = minted(False)[:n]
    assert not st.any() and all(w[2] == U.OK for w in want)
    assert (utxos == mont_rows([w[0] for w in want], 4)).all()
    assert (items == mont([w[1] for w in want])).all()


@pytest.mark.parametrize("n", SIZES)
def test_open_of_mint_matches_the_model(gpu, model, n):
    plain, flags = batch()
    _, vk, addr, pak = keys()
    want = minted(True)[:n]
    pt = mont_rows(plain[:n], 3)
    utxos, items, st = model.mint(np.repeat(mont_points([addr]), n, axis=0), pt, flags[:n])
    assert not st.any() and (utxos == mont_rows([w[0] for w in want], 4)).all()
    vk_limbs = gpu.edwards_scalars([vk])[0]
    st1, items1, nul1, ok1 = model.open(vk_limbs, pt, utxos)
    st2, items2, nul2, ok2 = model.open(vk_limbs, pt, utxos, pak=mont_points([pak])[0])
    assert not st1.any() and not st2.any() and ok1 == ok2 == n and nul1 is None
    assert (items1 == items).all() and (items2 == items).all()
    assert (items == mont([w[1] for w in want])).all()
    assert (nul2 == mont([MODEL.nullifier(pak, w[1]) for w in want])).all()


def test_identity_as_address_and_as_authorization_key(gpu, model):
    """viewing key 0 gives the address (0, 1); pak = (0, 1) is on the curve"""
    plain, flags = batch()
    n = 8
    pt = mont_rows(plain[:n], 3)
    ident = mont_points([E.IDENTITY])
    utxos, items, st = model.mint(np.repeat(ident, n, axis=0), pt, flags[:n])
    want = [MODEL.mint(E.IDENTITY, plain[i], flags[i]) for i in range(n)]
    assert not st.any() and (utxos == mont_rows([w[0] for w in want], 4)).all()
    st, items2, nul, n_ok = model.open(gpu.edwards_scalars([0])[0], pt, utxos, pak=ident[0])
    assert not st.any() and n_ok == n and (items2 == items).all()
    assert (nul == mont([MODEL.nullifier(E.IDENTITY, w[1]) for w in want])).all()


def test_every_way_to_fail(gpu, model):
    plain, flags = (list(x) for x in batch())
    _, vk, addr, pak = keys()
    n = 200
    plain, flags = plain[:n], flags[:n]
    kinds = {10: "cm_low", 11: "cm_high", 20: "pid", 21: "pval", 30: "flip0", 31: "flip1", 63: "flag2", 64: "secret_big",
             65: "public_big", 128: "both", 0: "cm_low", n - 1: "pid"}
    for i, k in kinds.items():  # the flag each case needs
        flags[i] = {"pid": 1, "pval": 1, "flip1": 1, "public_big": 1, "flip0": 0, "secret_big": 0}.get(k, flags[i])
    plain[30] = plain[31] = (5, 6, 7)  # a non-zero asset: flipping the flag changes the secret half
    plain[64] = (plain[64][0], plain[64][1], U128)
    plain[65] = (plain[65][0], plain[65][1], U128)
    records = [MODEL.reconstruct(flags[i], plain[i], addr) for i in range(n)]  # reconstruct ignores the u128 bound
    clean = [MODEL.open(addr, plain[i], records[i], pak) for i in range(n)]
    ut = mont_rows(records, 4)
    one = mont([1])[0]
    for i, k in kinds.items():
        if k == "cm_low":
            ut[i, 3, 0] ^= np.uint64(1)
        if k in ("cm_high", "both"):
            ut[i, 3, 3] ^= np.uint64(1)
            assert synth.limbs_to_ints(ut[i, 3:4])[0] < R
        if k == "pid":
            ut[i, 1] = mont([(records[i][1] + 1) % R])[0]
        if k == "pval":
            ut[i, 2] = mont([(records[i][2] + 1) % U128])[0]
        if k == "flip0":
            ut[i, 0] = one
        if k == "flip1":
            ut[i, 0] = 0
        if k in ("flag2", "both"):
            ut[i, 0] = mont([2])[0]
    want_st = [clean[i][0] for i in range(n)]
    assert [i for i in range(n) if want_st[i] != U.OK] == [64, 65]  # the model agrees these two are encoding failures only
    for i, k in kinds.items():
        want_st[i] = U.BAD_ENCODING if k in ("flag2", "secret_big", "public_big", "both") else U.MISMATCH
    pt = mont_rows(plain, 3)
    vk_limbs = gpu.edwards_scalars([vk])[0]
    st, items, nul, n_ok = model.open(vk_limbs, pt, ut, pak=mont_points([pak])[0])
    assert list(st) == want_st
    assert n_ok == n - len(kinds)
    want_items = rows_or_zeros([None if i in kinds else (clean[i][1],) for i in range(n)], 1).reshape(n, 4)
    want_nul = rows_or_zeros([None if i in kinds else (clean[i][2],) for i in range(n)], 1).reshape(n, 4)
    assert (items == want_items).all() and (nul == want_nul).all()
    for i in kinds:
        assert not items[i].any() and not nul[i].any(), i
    # the model on the tampered records themselves, where they are still field elements below r
    tampered = [tuple(ints(ut[i])) for i in kinds]
    for i, rec in zip(kinds, tampered):
        assert MODEL.open(addr, plain[i], rec, pak)[0] == want_st[i], (i, kinds[i])
    # without nullifiers the statuses and items are the same
    st2, items2, nul2, n_ok2 = model.open(vk_limbs, pt, ut)
    assert list(st2) == want_st and (items2 == want_items).all() and nul2 is None and n_ok2 == n_ok
    # the wrong viewing key: every lane mismatches, but for the badly encoded ones
    st3, items3, nul3, n_ok3 = model.open(gpu.edwards_scalars([(vk + 1) % L])[0], pt, ut, pak=mont_points([pak])[0])
    assert list(st3) == [U.BAD_ENCODING if s == U.BAD_ENCODING else U.MISMATCH for s in want_st]
    assert n_ok3 == 0 and not items3.any() and not nul3.any()
    # mint refuses a flag byte of 2 and a value of 2^128, and leaves the neighbours alone
    fl = np.array(flags, dtype=np.uint8)
    fl[63] = 2
    utxos, items4, st4 = model.mint(np.repeat(mont_points([addr]), n, axis=0), pt, fl)
    bad = [63, 64, 65]
    assert list(st4) == [U.BAD_ENCODING if i in bad else U.OK for i in range(n)]
    want_utxos, want_items4 = mont_rows(records, 4), mont([MODEL.item(r) for r in records])
    want_utxos[bad], want_items4[bad] = 0, 0
    assert (utxos == want_utxos).all() and (items4 == want_items4).all()


def test_viewing_keys_cover_every_quotient(gpu, model):
    paks = [E.IDENTITY] + walk(N - 1, seed=71)
    hashes = [MODEL.h2.hash(list(p)) for p in paks]
    assert {h // L for h in hashes} == set(range(8))  # seed 71 was chosen so that every quotient of `rem_mod_prime` occurs
    want = [MODEL.viewing_key(p) for p in paks]
    assert want == [h % L for h in hashes]
    vks, rks = model.viewing_keys(mont_points(paks))
    got = synth.limbs_to_ints(vks)
    assert all(v < L for v in got) and got == want
    assert (rks == gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, mont_points([G]), vks)).all()
    for i in (0, 1, N - 1):
        assert (rks[i] == mont_points([MODEL.receiving_key(want[i])])[0]).all(), i
    vks2, none = model.viewing_keys(mont_points(paks), recv_keys=False)
    assert none is None and (vks2 == vks).all()
    for n in SIZES[:-1]:
        v, r = model.viewing_keys(mont_points(paks[:n]))
        assert (v == vks[:n]).all() and (r == rks[:n]).all(), n


def test_chunk_boundary_against_the_hasher_route_and_the_model(gpu, model):
    n = CHUNK + 1
    rng = random.Random(113)
    _, vk, addr, pak = keys()
    plain = [(rng.randrange(R), rng.randrange(R), rng.randrange(U128)) for _ in range(n)]
    flags = np.array([rng.randrange(2) for _ in range(n)], dtype=np.uint8)
    pt = mont_rows(plain, 3)
    rk = mont_points([addr])
    utxos, items, st = model.mint(np.repeat(rk, n, axis=0), pt, flags)
    assert not st.any()
    # the route a caller had before: three hash calls and host glue
    h5, h4, h3 = (gpu.PoseidonHasher(gpu.BN254, t, f, p, d) for d, (t, f, p) in zip(FILES[:3], U.SHAPES[:3]))
    tr = flags.astype(bool)[:, None]
    zero = np.zeros((n, 4), dtype=np.uint64)
    in5 = np.stack([pt[:, 0], np.where(tr, zero, pt[:, 1]), np.where(tr, zero, pt[:, 2]),
                    np.repeat(rk[:, :4], n, axis=0), np.repeat(rk[:, 4:], n, axis=0)], axis=1)
    cm = h5.hash(in5)
    rec = np.stack([np.where(tr, mont([1]), zero), np.where(tr, pt[:, 1], zero), np.where(tr, pt[:, 2], zero), cm], axis=1)
    assert (utxos == rec).all()
    want_items = h4.hash(rec)
    assert (items == want_items).all()
    pk = mont_points([pak])
    want_nul = h3.hash(np.stack([np.repeat(pk[:, :4], n, axis=0), np.repeat(pk[:, 4:], n, axis=0), want_items], axis=1))
    bad = [0, n // 3, CHUNK - 1, CHUNK]  # a mismatch on both sides of the boundary
    tampered = utxos.copy()
    for i in bad:
        tampered[i, 3, 0] ^= np.uint64(1)
    stat, items2, nul, n_ok = model.open(gpu.edwards_scalars([vk])[0], pt, tampered, pak=pk[0])
    assert [i for i in range(n) if stat[i]] == sorted(bad) and all(stat[i] == U.MISMATCH for i in bad) and n_ok == n - len(bad)
    want_items[bad], want_nul[bad] = 0, 0
    assert (items2 == want_items).all() and (nul == want_nul).all()
    idx = sorted(set([0, 1, CHUNK - 2, CHUNK - 1, CHUNK, n - 1] + rng.sample(range(n), 250)))  # at most 256 lanes
    for i in idx:
        w_utxo, w_item, w_st = MODEL.mint(addr, plain[i], int(flags[i]))
        assert w_st == U.OK and tuple(ints(utxos[i])) == w_utxo and ints(items[i]) == [w_item], i
        if i not in bad:
            assert ints(nul[i]) == [MODEL.nullifier(pak, w_item)], i


def test_four_threads_share_one_model(gpu, model):
    n = 3000
    _, vk, addr, pak = keys()
    vk_limbs, pk, rk = gpu.edwards_scalars([vk])[0], mont_points([pak])[0], mont_points([addr])
    work = []
    for t in range(4):
        rng = random.Random(127 + t)
        pt = mont_rows([(rng.randrange(R), rng.randrange(R), rng.randrange(U128)) for _ in range(n)], 3)
        fl = np.array([rng.randrange(2) for _ in range(n)], dtype=np.uint8)
        utxos, items, st = model.mint(np.repeat(rk, n, axis=0), pt, fl)
        assert not st.any()
        utxos[t::7, 3, 0] ^= np.uint64(1)  # a different set of mismatches per thread
        work.append((pt, utxos, model.open(vk_limbs, pt, utxos, pak=pk)))
        assert work[-1][2][3] == n - len(range(t, n, 7))
    got, errors = [None] * 4, []

    def run(t):
        try:
            for _ in range(3):
                got[t] = model.open(vk_limbs, work[t][0], work[t][1], pak=pk)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for t in range(4):
        for w, g_ in zip(work[t][2][:3], got[t][:3]):
            assert (w == g_).all(), t
        assert got[t][3] == work[t][2][3]


def test_models_do_not_share_constants(gpu, model):
    """a second model whose commitment hasher has one round key changed gives other commitments, the first model's stay"""
    data, params = P.load(U.FILES[0])
    params.keys[7] = (params.keys[7] + 1) % R
    other_ref = U.Model([params.encode()] + FILES[1:])
    other = gpu.UtxoModel(params.encode(), *FILES[1:])
    plain, flags = batch()
    rks = keys()[0]
    n = 65
    args = (mont_points(rks[:n]), mont_rows(plain[:n], 3), flags[:n])
    u1, i1, _ = model.mint(*args)
    u2, i2, _ = other.mint(*args)
    u3, i3, _ = model.mint(*args)
    assert (u1 == u3).all() and (i1 == i3).all()
    assert (u1[:, :3] == u2[:, :3]).all() and not (u1[:, 3] == u2[:, 3]).all(axis=1).any()
    assert not (i1 == i2).all(axis=1).any()
    want = [other_ref.mint(rks[i], plain[i], flags[i]) for i in range(8)]
    assert (u2[:8] == mont_rows([w[0] for w in want], 4)).all() and (i2[:8] == mont([w[1] for w in want])).all()
    assert (u1 == mont_rows([w[0] for w in minted(False)[:n]], 4)).all()
    other.close()
