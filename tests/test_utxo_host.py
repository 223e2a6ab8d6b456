"""CPU tests of the batched UTXO derivation (mg_utxo_model_*, mg_utxos_*, mg_viewing_keys): the Python restatement the GPU tests
check against (tests/utxo_ref.py) loads the reference's parameter files at the shapes the checkfiles record; the committed files
carry the reference's digests; mg_utxo_model_create decodes on the host; and every argument check of the C ABI answers
MG_ERROR_INVALID_ARGUMENT before any device work, so these run without a GPU."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest

import edwards_ref as E
import poseidon_ref as P
import utxo_ref as U
from manta_rs_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ED_CHECK = json.load(open(os.path.join(P.PARAM_DIR, "edwards_checkfile.json")))
INVALID = 1  # MG_ERROR_INVALID_ARGUMENT
R, L = U.R, U.L
FILES = [U.read(n) for n in U.FILES]


def mont_points(points):
    return synth.to_mont([c for p in points for c in p], R, 4).reshape(-1, 8)


def test_model_loads_the_files_at_the_recorded_shapes():
    m = U.Model()
    for name, params, (t, full, partial) in zip(U.FILES, (m.h5, m.h4, m.h3), U.SHAPES):
        rec = P.CHECKFILE[name]
        assert (rec["width"], rec["full_rounds"], rec["partial_rounds"]) == (t, full, partial) == (params.t, params.full, params.partial)
        assert params.encode() == U.read(name)
    t, full, partial = U.SHAPES[3]
    assert ED_CHECK[U.FILES[3]]["bytes"] == 32 * ((full + partial) * t + t * t + 1) == len(FILES[3])
    assert m.h2.encode() == FILES[3] and (m.h2.t, m.h2.full, m.h2.partial) == (3, 8, 55)
    assert ED_CHECK[U.FILES[4]]["bytes"] == 32 and m.g == E.generator()


@pytest.mark.parametrize("name", U.FILES)
def test_parameter_fixture_digests(name):
    from manta_rs_amd import api
    want = (P.CHECKFILE.get(name) or ED_CHECK[name])["blake3"]
    assert api.blake3(U.read(name)).hex() == want


def test_reduction_mod_l():
    assert 7 * L < R < 8 * L
    rng = random.Random(3)
    edge = [0, 1, L - 1, L, L + 1, R - 1] + [k * L + d for k in range(1, 8) for d in (-1, 0, 1)]
    seen = set()
    for v in edge + [rng.randrange(R) for _ in range(2000)]:
        got, q = U.rem_mod_l(v)
        assert got == v % L and q == v // L
        seen.add(q)
    assert seen == set(range(8))


def test_model_statement_is_consistent():
    """mint then open agree; a transparent record carries the asset in the clear and commits to (0, 0)"""
    m = U.Model()
    rng = random.Random(5)
    vk = rng.randrange(1, L)
    rk, pak = m.receiving_key(vk), E.mul(m.g, rng.randrange(1, L))
    pt = (rng.randrange(R), rng.randrange(R), rng.randrange(U.U128))
    for flag in (0, 1):
        utxo, item, st = m.mint(rk, pt, flag)
        assert st == U.OK and utxo[0] == flag
        assert utxo[1:3] == ((pt[1], pt[2]) if flag else (0, 0))
        assert utxo[3] == m.h5.hash([pt[0]] + ([0, 0] if flag else [pt[1], pt[2]]) + list(rk))
        assert item == m.h4.hash(list(utxo))
        assert m.open(rk, pt, utxo, pak) == (U.OK, item, m.h3.hash([pak[0], pak[1], item]))
        assert m.open(rk, pt, (1 - flag,) + utxo[1:])[0] == U.MISMATCH
        assert m.open(rk, pt, utxo[:3] + ((utxo[3] + 1) % R,))[0] == U.MISMATCH
        assert m.open(E.mul(rk, 2), pt, utxo)[0] == U.MISMATCH
        assert m.open(rk, pt, (2,) + utxo[1:])[0] == U.BAD_ENCODING
    assert m.mint(rk, (pt[0], pt[1], U.U128), 0)[2] == U.BAD_ENCODING and m.mint(rk, pt, 2)[2] == U.BAD_ENCODING
    assert m.viewing_key(pak) == m.h2.hash(list(pak)) % L


def _create(curve, files):
    from manta_rs_amd import api
    h = ctypes.c_void_p()
    keep = [bytes(b) for b in files]
    arg = api._UtxoFiles(*[api._UtxoFile(b, len(b)) for b in keep])
    rc = api.LIB.mg_utxo_model_create(curve, ctypes.byref(arg), ctypes.byref(h))
    return rc, h


def order8_point():
    for x in range(2, 1000):
        y = E.y_from_x(x, False)
        if y is not None:
            t = E.mul((x, y), L)
            if E.mul(t, 4) != E.IDENTITY:
                return t
    raise AssertionError("no point of order 8 found")


def test_model_create_accepts_the_production_files_and_rejects_malformed_ones():
    from manta_rs_amd import api
    rc, h = _create(0, FILES)
    assert rc == 0 and h.value
    api.LIB.mg_utxo_model_destroy(h)

    def rejected(files, curve=0):
        rc, h = _create(curve, files)
        assert rc == INVALID and not h.value

    rejected(FILES, curve=1)  # BLS12-381 has no embedded curve here
    for i in range(4):
        for bad in (FILES[i][:-32], FILES[i][:-1], FILES[i] + bytes(32)):  # truncated, a byte short, one element too long
            rejected(FILES[:i] + [bad] + FILES[i + 1:])
        for pos in (0, len(FILES[i]) // 32 - 1):  # an element equal to r: the first round key, the domain tag
            bad = bytearray(FILES[i])
            bad[32 * pos:32 * pos + 32] = R.to_bytes(32, "little")
            rejected(FILES[:i] + [bytes(bad)] + FILES[i + 1:])
        ok = bytearray(FILES[i])
        ok[-32:] = (R - 1).to_bytes(32, "little")  # r - 1 is canonical
        rc, h = _create(0, FILES[:i] + [bytes(ok)] + FILES[i + 1:])
        assert rc == 0
        api.LIB.mg_utxo_model_destroy(h)
    for i, j in ((0, 1), (1, 2), (2, 3), (0, 3)):  # two files swapped: the widths differ, so the lengths do
        sw = list(FILES)
        sw[i], sw[j] = sw[j], sw[i]
        rejected(sw)
    g = FILES[4]
    x_noroot = next(x for x in range(2, 100) if E.y_from_x(x, False) is None)
    flipped = bytearray(g)
    flipped[31] ^= 0x80  # the other root: on the curve, outside the subgroup
    t8 = order8_point()
    assert E.on_curve(t8) and E.mul(t8, 8) == E.IDENTITY and E.mul(t8, 4) != E.IDENTITY
    for bad in (g[:31], g + b"\0", x_noroot.to_bytes(32, "little"), R.to_bytes(32, "little"), bytes(flipped), E.encode(t8),
                E.encode((1, 0)), bytes(32)):
        rejected(FILES[:4] + [bad])
    other = E.encode(E.mul(E.generator(), 12345))  # any point of order l will do as a generator
    rc, h = _create(0, FILES[:4] + [other])
    assert rc == 0
    api.LIB.mg_utxo_model_destroy(h)
    assert api.LIB.mg_utxo_model_create(0, None, ctypes.byref(ctypes.c_void_p())) == INVALID
    with pytest.raises(api.MantaGpuError):
        api.UtxoModel(*FILES[:3], FILES[3][:-1], FILES[4])


def test_argument_checks_need_no_gpu():
    from manta_rs_amd import api
    m = api.UtxoModel(*FILES)
    g = mont_points([E.generator()])
    pts = np.repeat(g, 3, axis=0)
    pt, ut = np.zeros((3, 3, 4), dtype=np.uint64), np.zeros((3, 4, 4), dtype=np.uint64)
    fl = np.zeros(3, dtype=np.uint8)
    vk = api.edwards_scalars([5])[0]
    off = mont_points([(E.generator()[0], 5)])[0]

    def invalid(call):
        with pytest.raises(api.MantaGpuError) as e:
            call()
        assert e.value.status == INVALID

    invalid(lambda: m.open(api.edwards_scalars([L])[0], pt, ut))  # a viewing key >= l
    invalid(lambda: m.open(api.edwards_scalars([(1 << 256) - 1])[0], pt, ut))
    invalid(lambda: m.open(vk, pt, ut, pak=off))  # a pak off the curve
    unreduced = g[0].copy()
    unreduced[:4] = synth.ints_to_limbs([R], 4)[0]
    invalid(lambda: m.open(vk, pt, ut, pak=unreduced))
    lib, p, sz = api.LIB, api._p, api._sz
    st, items, nul = np.zeros(3, dtype=np.uint8), np.zeros((3, 4), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
    n_ok = ctypes.c_size_t(7)
    # one of pak / nullifiers_out without the other
    assert lib.mg_utxos_open(m._h, p(vk), p(g), p(pt), p(ut), sz(3), p(st), p(items), None, ctypes.byref(n_ok)) == INVALID
    assert lib.mg_utxos_open(m._h, p(vk), None, p(pt), p(ut), sz(3), p(st), p(items), p(nul), ctypes.byref(n_ok)) == INVALID
    # NULL arrays with n > 0, a NULL model, a NULL viewing key
    for args in ((None, p(ut), p(st), p(items)), (p(pt), None, p(st), p(items)), (p(pt), p(ut), None, p(items)),
                 (p(pt), p(ut), p(st), None)):
        assert lib.mg_utxos_open(m._h, p(vk), None, args[0], args[1], sz(3), args[2], args[3], None, None) == INVALID
    assert lib.mg_utxos_open(None, p(vk), None, p(pt), p(ut), sz(3), p(st), p(items), None, None) == INVALID
    assert lib.mg_utxos_open(m._h, None, None, p(pt), p(ut), sz(3), p(st), p(items), None, None) == INVALID
    good = [p(pts), p(pt), p(fl), sz(3), p(ut), p(items), p(st)]
    for k in (0, 1, 2, 4, 5, 6):
        args = list(good)
        args[k] = None
        assert lib.mg_utxos_mint(m._h, *args) == INVALID, k
    assert lib.mg_utxos_mint(None, *good) == INVALID
    vks = np.zeros((3, 4), dtype=np.uint64)
    assert lib.mg_viewing_keys(m._h, None, sz(3), p(vks), None) == INVALID
    assert lib.mg_viewing_keys(m._h, p(pts), sz(3), None, None) == INVALID
    assert lib.mg_viewing_keys(None, p(pts), sz(3), p(vks), None) == INVALID
    # n = 0 succeeds without a device and touches nothing
    assert lib.mg_utxos_mint(m._h, None, None, None, sz(0), None, None, None) == 0
    assert lib.mg_utxos_open(m._h, p(vk), None, None, None, sz(0), None, None, None, None) == 0
    assert lib.mg_viewing_keys(m._h, None, sz(0), None, None) == 0
    u, i, s = m.mint(pts[:0], pt[:0], fl[:0])
    assert u.shape == (0, 4, 4) and i.shape == (0, 4) and s.shape == (0,)
    s, i, nl, ok = m.open(vk, pt[:0], ut[:0], pak=g[0])
    assert s.shape == (0,) and i.shape == (0, 4) and nl.shape == (0, 4) and ok == 0
    v, r = m.viewing_keys(pts[:0])
    assert v.shape == (0, 4) and r.shape == (0, 8)
    m.close()


def test_no_gpu_is_an_error_not_a_fallback():
    from manta_rs_amd import api
    try:
        n = api.device_count()
    except api.MantaGpuError:
        n = 0
    if n:
        return  # the GPU suite covers the compute paths
    m = api.UtxoModel(*FILES)
    g = mont_points([E.generator()])
    pt, ut = np.zeros((1, 3, 4), dtype=np.uint64), np.zeros((1, 4, 4), dtype=np.uint64)
    vk = api.edwards_scalars([1])[0]
    for call in (lambda: m.mint(g, pt, [0]), lambda: m.open(vk, pt, ut), lambda: m.open(vk, pt, ut, pak=g[0]),
                 lambda: m.viewing_keys(g), lambda: m.viewing_keys(g, recv_keys=False)):
        with pytest.raises(api.MantaGpuError) as e:
            call()
        assert e.value.status in (2, 3)  # MG_ERROR_HIP / MG_ERROR_OUT_OF_MEMORY: the device's refusal, never a result


def test_constants_match_the_header():
    from manta_rs_amd import api
    hdr = open(os.path.join(HERE, "..", "include", "mantagpu.h")).read()
    for name, val, ref in (("MG_UTXO_OK", api.UTXO_OK, U.OK), ("MG_UTXO_BAD_ENCODING", api.UTXO_BAD_ENCODING, U.BAD_ENCODING),
                           ("MG_UTXO_MISMATCH", api.UTXO_MISMATCH, U.MISMATCH)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val == ref
