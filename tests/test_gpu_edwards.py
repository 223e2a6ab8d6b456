"""GPU tests of the embedded curve and the Poseidon note encryption (mg_edwards_*, mg_notes_*), limb for limb against the
pure-Python restatement of tests/edwards_ref.py (affine formulas, pinned to the reference's parameter files by
test_edwards_host.py). Where the model is too slow for a whole batch (one scalar multiplication costs it milliseconds), the
batch is checked through group identities -- commutativity, (l - 1) P = -P, [l] P = O -- and a 256-lane sample against the
model."""
import random
import threading

import numpy as np
import pytest

import edwards_ref as E
from manta_rs_amd import synth
from test_edwards_host import mont_points, read

pytestmark = pytest.mark.gpu

R, L = E.R, E.L
G = E.generator()
CHUNK = 1 << 16
SMALL = [E.IDENTITY, (0, R - 1), (1, 0), (R - 1, 0)]  # orders 1, 2, 4, 4


def to_points(arr):
    v = synth.from_mont(np.asarray(arr, dtype=np.uint64).reshape(-1, 4), R)
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def mont(vals):
    return synth.to_mont([int(v) for v in vals], R, 4)


def ints(arr):
    return synth.from_mont(np.asarray(arr, dtype=np.uint64).reshape(-1, 4), R)


def walk(n, seed):
    """n distinct subgroup points by a walk P, P + H, P + 2H, ..: one model addition each"""
    rng = random.Random(seed)
    p, h = E.mul(G, rng.randrange(1, L)), E.mul(G, rng.randrange(1, L))
    out = []
    for _ in range(n):
        out.append(p)
        p = E.add(p, h)
    return out


def rand_scalars(n, seed):
    """[n, 4] limbs of scalars below 2^250 < l"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 58) - 1)
    return a


def scalar_ints(a):
    return synth.limbs_to_ints(a)


def order8_point():
    """a point of order exactly 8 (outside the subgroup): [l] of a curve point whose cofactor part has full order"""
    for x in range(2, 1000):
        y = E.y_from_x(x, False)
        if y is None:
            continue
        t = E.mul((x, y), L)
        if E.mul(t, 4) != E.IDENTITY:
            return t
    raise AssertionError("no point of order 8 found")


def test_decode_encode_round_trip_and_rejections(gpu):
    pts = walk(4096, seed=1)
    t8 = order8_point()
    assert E.mul(t8, 8) == E.IDENTITY and E.mul(t8, 4) != E.IDENTITY
    mixed = E.add(t8, pts[0])  # order 8 times a subgroup point: on the curve, outside the subgroup
    good = pts + [E.neg(p) for p in pts[:64]]
    enc = b"".join(E.encode(p) for p in good)
    got, st = gpu.edwards_decode(enc)
    assert not st.any()
    assert (got == mont_points(good)).all()
    assert gpu.edwards_encode(got) == enc
    assert not gpu.edwards_check(got).any()
    # both y signs of one x: the subgroup point, and its mirror (x, -y) = -(P + order-2 point), outside the subgroup
    for p in pts[:8]:
        mirror = (p[0], R - p[1])
        e = E.encode(mirror)
        assert e[:31] == E.encode(p)[:31] and e[31] ^ E.encode(p)[31] == 0x80
        got1, st1 = gpu.edwards_decode(e)
        assert st1[0] == gpu.POINT_NOT_IN_SUBGROUP and not got1.any()
        got0, st0 = gpu.edwards_decode(e, checked=False)
        assert st0[0] == gpu.POINT_OK and (got0 == mont_points([mirror])).all()
    # special encodings, each against the model
    x_noroot = next(x for x in range(2, 100) if E.y_from_x(x, False) is None)
    cases = [E.encode(p) for p in SMALL + [t8, mixed, E.neg(mixed)]]
    cases += [bytes(31) + b"\x80",  # x = 0 with the flag: still the identity
              R.to_bytes(32, "little"), (R + 1).to_bytes(32, "little"), (R | (1 << 255)).to_bytes(32, "little"),
              (1 << 254).to_bytes(32, "little"), bytes([255] * 32),  # x >= p
              x_noroot.to_bytes(32, "little"), (x_noroot | (1 << 255)).to_bytes(32, "little"),  # no root
              (R - 1).to_bytes(32, "little"), ((R - 1) | (1 << 255)).to_bytes(32, "little")]  # (-1, 0), y = 0 either flag
    for checked in (True, False):
        got, st = gpu.edwards_decode(b"".join(cases), checked=checked)
        for i, c in enumerate(cases):
            want, wst = E.decode(c, checked=checked)
            assert st[i] == wst, (i, checked, st[i], wst)
            if want is None:
                assert not got[i].any(), i
            else:
                assert (got[i] == mont_points([want])[0]).all(), (i, checked)
    # encode and check of the special points
    special = SMALL + [t8, mixed, G, (5, 7)]
    m = mont_points(special)
    assert gpu.edwards_encode(m) == b"".join(E.encode(p) for p in special)
    assert list(gpu.edwards_check(m)) == [E.check(p) for p in special]
    unreduced = m[6:7].copy()
    unreduced[0, :4] = synth.ints_to_limbs([R], 4)[0]  # a coordinate equal to p
    assert gpu.edwards_check(unreduced)[0] == gpu.POINT_BAD_ENCODING
    _, st = gpu.edwards_decode(b"".join(cases))
    n_bad = sum(1 for c in cases if E.decode(c)[1] != E.OK)
    assert int((st != 0).sum()) == n_bad


def test_mul_shapes_match_the_model(gpu):
    rng = random.Random(11)
    pts = SMALL + [order8_point(), G] + walk(26, seed=2)
    scalars = [0, 1, 2, L - 1] + [rng.randrange(L) for _ in range(4)]
    mp = mont_points(pts)
    for k in scalars:  # n points x one scalar
        got = gpu.edwards_mul(gpu.EDWARDS_MUL_SHARED_SCALAR, mp, gpu.edwards_scalars([k]))
        assert (got == mont_points([E.mul(p, k) for p in pts])).all(), k
    ks = scalars + [rng.randrange(L) for _ in range(24)]
    for base in (G, pts[7], E.IDENTITY, (0, R - 1), (1, 0)):  # n scalars x one base
        got = gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, mont_points([base]), gpu.edwards_scalars(ks))
        assert (got == mont_points([E.mul(base, k) for k in ks])).all(), base
    ks = (scalars * 4)[:len(pts)]  # n scalars x n points: every edge scalar meets small-order and ordinary points
    ks[8:] = [rng.randrange(L) for _ in ks[8:]]
    for rot in range(4):
        kk = ks[rot:] + ks[:rot]
        got = gpu.edwards_mul(gpu.EDWARDS_MUL_PAIRWISE, mp, gpu.edwards_scalars(kk))
        assert (got == mont_points([E.mul(p, k) for p, k in zip(pts, kk)])).all(), rot
    # addition: P + P, P + (-P), with the identity and the small-order points, unrelated points
    a = pts + pts + pts
    b = pts + [E.neg(p) for p in pts] + pts[5:] + pts[:5]
    got = gpu.edwards_add(mont_points(a), mont_points(b))
    assert (got == mont_points([E.add(p, q) for p, q in zip(a, b)])).all()


def test_key_derivation_with_the_production_generator(gpu):
    rng = random.Random(13)
    sks = [1, 2, L - 1] + [rng.randrange(1, L) for _ in range(61)]
    got = gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, mont_points([G]), gpu.edwards_scalars(sks))
    assert (got == mont_points([E.mul(G, k) for k in sks])).all()
    assert gpu.edwards_encode(got[:1]) == read("group-generator.dat")


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_diffie_hellman_commutes_across_a_chunk_boundary(gpu, n):
    """a (b G) = b (a G) on every lane, through all three shapes; every result is in the subgroup ([l] P = O through
    mg_edwards_check) and (l - 1) P = -P; a 256-lane sample against the model"""
    g = mont_points([G])
    a, b = rand_scalars(n, seed=n), rand_scalars(n, seed=n + 7)
    a[0], b[1] = 0, 0  # a zero scalar on either side
    ag = gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, g, a)
    bg = gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, g, b)
    ab = gpu.edwards_mul(gpu.EDWARDS_MUL_PAIRWISE, bg, a)
    ba = gpu.edwards_mul(gpu.EDWARDS_MUL_PAIRWISE, ag, b)
    assert (ab == ba).all()
    assert (ab[0] == mont_points([E.IDENTITY])[0]).all() and (ab[1] == mont_points([E.IDENTITY])[0]).all()
    assert not gpu.edwards_check(ab).any()
    # one shared scalar over the whole batch against the pairwise kernel given that scalar in every lane
    k = rand_scalars(1, seed=3 * n)
    shared = gpu.edwards_mul(gpu.EDWARDS_MUL_SHARED_SCALAR, ag, k)
    assert (shared == gpu.edwards_mul(gpu.EDWARDS_MUL_PAIRWISE, ag, np.repeat(k, n, axis=0))).all()
    minus = gpu.edwards_mul(gpu.EDWARDS_MUL_SHARED_SCALAR, ag, gpu.edwards_scalars([L - 1]))
    neg = ag.copy()
    x = ints(ag[:, :4])
    neg[:, :4] = mont([(R - v) % R for v in x])
    assert (minus == neg).all()
    assert (gpu.edwards_add(minus, ag) == mont_points([E.IDENTITY])[0]).all()
    idx = sorted(set([0, 1, 2, n - 1, n - 2] + random.Random(n).sample(range(n), 251)))[:256]
    ai, bi, ki = scalar_ints(a[idx]), scalar_ints(b[idx]), scalar_ints(k)[0]
    assert (ab[idx] == mont_points([E.mul(G, x * y % L) for x, y in zip(ai, bi)])).all()
    assert (shared[idx[:32]] == mont_points([E.mul(G, x * ki % L) for x in ai[:32]])).all()


def cipher(gpu):
    return gpu.NoteCipher(read("incoming-base-encryption-scheme.dat"), mont_points([G]))


def rand_plaintexts(n, seed):
    rng = random.Random(seed)
    return [[rng.randrange(R), rng.randrange(R), rng.randrange(1 << 128)] for _ in range(n)]


def test_encrypt_matches_the_model(gpu):
    c, model = cipher(gpu), E.Cipher.load()
    rng = random.Random(17)
    n = 48
    sks = [rng.randrange(1, L) for _ in range(n)]
    rnd = [1, L - 1] + [rng.randrange(1, L) for _ in range(n - 2)]
    pks = [E.mul(G, k) for k in sks]
    pts = rand_plaintexts(n, seed=19)
    pts[0], pts[1], pts[2] = [0, 0, 0], [R - 1, R - 1, (1 << 128) - 1], [1, 2, 3]
    epk, ct, tag = c.encrypt(mont_points(pks), gpu.edwards_scalars(rnd), mont([w for p in pts for w in p]).reshape(n, 3, 4))
    for i in range(n):
        w_epk, w_ct, w_tag = E.note_encrypt(model, G, pks[i], rnd[i], pts[i])
        assert to_points(epk[i]) == [w_epk], i
        assert ints(ct[i]) == w_ct and ints(tag[i]) == [w_tag], i
    for i in range(n):  # each receiver opens their own note
        pt, ok, st = c.decrypt(gpu.edwards_scalars([sks[i]])[0], epk[i:i + 1], ct[i:i + 1], tag[i:i + 1])
        assert ok[0] and st[0] == gpu.NOTE_OK and ints(pt[0]) == pts[i], i


@pytest.mark.parametrize("n", [1000, CHUNK + 1])
def test_decrypt_of_encrypt_is_the_identity_on_every_lane(gpu, n):
    c = cipher(gpu)
    vk = random.Random(n).randrange(1, L)
    pk = gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, mont_points([G]), gpu.edwards_scalars([vk]))
    pts = mont([w for p in rand_plaintexts(n, seed=n + 1) for w in p]).reshape(n, 3, 4)
    epk, ct, tag = c.encrypt(np.repeat(pk, n, axis=0), rand_scalars(n, seed=n + 2) + np.uint64(1), pts)
    pt, ok, st = c.decrypt(gpu.edwards_scalars([vk])[0], epk, ct, tag)
    assert ok.all() and not st.any()
    assert (pt == pts).all()


def test_decrypt_rejects_exactly_the_bad_notes(gpu):
    """a ledger of notes of which a known subset is not ours (another viewing key), or has a flipped tag, a flipped ciphertext
    word, or an asset value of 2^128 or more: exactly those lanes come back ok = 0 with zero plaintext, every other lane
    ok = 1 with its plaintext"""
    c = cipher(gpu)
    n = 3000
    rng = random.Random(23)
    vk, other = rng.randrange(1, L), rng.randrange(1, L)
    pk, pk2 = (gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, mont_points([G]), gpu.edwards_scalars([k])) for k in (vk, other))
    kinds = ["ok"] * n
    for kind in ("foreign", "tag", "ct0", "ct1", "ct2", "value", "value_max"):
        for i in rng.sample([j for j in range(n) if kinds[j] == "ok"], 37):
            kinds[i] = kind
    kinds[0], kinds[n - 1], kinds[63], kinds[64] = "foreign", "tag", "value", "ct2"
    plain = rand_plaintexts(n, seed=29)
    for i, k in enumerate(kinds):
        if k == "value":
            plain[i][2] = 1 << 128
        if k == "value_max":
            plain[i][2] = R - 1
    pts = mont([w for p in plain for w in p]).reshape(n, 3, 4)
    keys = np.stack([pk2[0] if k == "foreign" else pk[0] for k in kinds])
    epk, ct, tag = c.encrypt(keys, rand_scalars(n, seed=31) + np.uint64(1), pts)
    one = mont([1])[0]
    for i, k in enumerate(kinds):
        if k == "tag":
            tag[i] = mont([(ints(tag[i])[0] + 1) % R])[0]
        if k.startswith("ct"):
            j = int(k[2])
            ct[i, j] = mont([(ints(ct[i, j])[0] + 1) % R])[0]
    assert one.any()
    pt, ok, st = c.decrypt(gpu.edwards_scalars([vk])[0], epk, ct, tag)
    want_st = [gpu.NOTE_OK if k == "ok" else gpu.NOTE_BAD_VALUE if k.startswith("value") else gpu.NOTE_BAD_TAG for k in kinds]
    assert list(st) == want_st
    assert list(ok) == [k == "ok" for k in kinds]
    for i, k in enumerate(kinds):
        if k == "ok":
            assert (pt[i] == pts[i]).all(), i
        else:
            assert not pt[i].any(), (i, k)
    # the model agrees on a sample of every kind
    model = E.Cipher.load()
    seen = {}
    for i, k in enumerate(kinds):
        if seen.setdefault(k, 0) < 3:
            seen[k] += 1
            w_pt, w_ok = E.note_decrypt(model, vk, to_points(epk[i])[0], ints(ct[i]), ints(tag[i])[0])
            assert w_ok == bool(ok[i]) and (w_pt is None or w_pt == ints(pt[i])), (i, k)


def test_two_host_threads(gpu):
    c = cipher(gpu)
    n = 5000
    g = mont_points([G])
    vk = gpu.edwards_scalars([random.Random(37).randrange(1, L)])
    pk = gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, g, vk)
    sc = [rand_scalars(n, seed=41 + t) + np.uint64(1) for t in range(2)]
    pts = [mont([w for p in rand_plaintexts(n, seed=43 + t) for w in p]).reshape(n, 3, 4) for t in range(2)]
    want = []
    for t in range(2):
        epk, ct, tag = c.encrypt(np.repeat(pk, n, axis=0), sc[t], pts[t])
        want.append((gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, g, sc[t]), epk, ct, tag))
    got, errors = [None, None], []

    def work(t):
        try:
            for _ in range(3):
                fixed = gpu.edwards_mul(gpu.EDWARDS_MUL_FIXED_BASE, g, sc[t])
                epk, ct, tag = c.encrypt(np.repeat(pk, n, axis=0), sc[t], pts[t])
                pt, ok, _ = c.decrypt(vk[0], epk, ct, tag)
                got[t] = (fixed, epk, ct, tag, pt, ok)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for t in range(2):
        for w, g_ in zip(want[t], got[t][:4]):
            assert (w == g_).all(), t
        assert got[t][5].all() and (got[t][4] == pts[t]).all(), t
