"""The batched UTXO derivation on the GPU (mg_utxos_mint, mg_utxos_open, mg_viewing_keys): one JSON line, also written to
profiles/utxo_bench.json.

  mint_2^16 / _2^20           records and items per second, mg_utxos_mint (host arrays in and out)
  open_2^16 / _2^20           UTXOs checked per second with items and nullifier commitments, mg_utxos_open
  viewing_keys_2^16 / _2^20   viewing keys with their receiving keys per second, mg_viewing_keys
  composition_2^16            the route a caller had before: three mg_poseidon_hash calls (widths 6, 5, 4) with the selection, the
                              limb-wise compare and the broadcast of the keys in numpy, alternated with mg_utxos_open in this
                              process on the same batch; `ratio` = its median over mg_utxos_open's
  roofline                    v_mad_u64_u32 issue of open at 2^20 and of the viewing-key hash at 2^20 as fractions of the peak
                              mg_clock_probe measures in the same run (the calls include the host copies, so these are lower
                              bounds on the kernels'): 128 per Montgomery product, 3t + t^2 products per full and 3 + t^2 per
                              partial round -- 2 616 + 1 888 + 1 269 = 5 773 per opened UTXO, 804 per viewing key

Every figure is the median of --reps calls after one warm-up call.

    python tools/utxo_bench.py [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MADS_PER_MUL = 128
P_TOP = 0x30644e72e131a029  # the top limb of r: limbs below it are a reduced element


def muls(t, full, partial):
    return full * (3 * t + t * t) + partial * (3 + t * t)


MULS_OPEN = muls(6, 8, 56) + muls(5, 8, 56) + muls(4, 8, 55)
MULS_VK = muls(3, 8, 55)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, reps):
    fn()
    return statistics.median(timed(fn) for _ in range(reps))


def composed_open(hashers, one, rk, pak, pt, utxos):
    """status, items, nullifiers of mg_utxos_open from three hash calls and numpy (encoding checks left out: the batch is clean)"""
    h5, h4, h3 = hashers
    n = pt.shape[0]
    tr = (utxos[:, 0] == one).all(axis=1)[:, None]
    zero = np.zeros((n, 4), dtype=np.uint64)
    in5 = np.stack([pt[:, 0], np.where(tr, zero, pt[:, 1]), np.where(tr, zero, pt[:, 2]), np.broadcast_to(rk[:4], (n, 4)),
                    np.broadcast_to(rk[4:], (n, 4))], axis=1)
    cm = h5.hash(in5)
    rec = np.stack([utxos[:, 0], np.where(tr, pt[:, 1], zero), np.where(tr, pt[:, 2], zero), cm], axis=1)
    ok = (rec == utxos).all(axis=(1, 2))
    items = h4.hash(utxos)
    nul = h3.hash(np.stack([np.broadcast_to(pak[:4], (n, 4)), np.broadcast_to(pak[4:], (n, 4)), items], axis=1))
    items[~ok], nul[~ok] = 0, 0
    return np.where(ok, 0, 2).astype(np.uint8), items, nul


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from manta_rs_amd import api, synth
    import torch
    import utxo_ref as U

    api.init(0)
    files = [U.read(n) for n in U.FILES]
    model = api.UtxoModel(*files)
    hashers = [api.PoseidonHasher(api.BN254, t, f, p, d) for d, (t, f, p) in zip(files[:3], U.SHAPES[:3])]
    rng = np.random.default_rng(2026)
    out = {"tool": "utxo_bench", "reps": a.reps, "chunk": api.EDWARDS_CHUNK, "muls_per_open": MULS_OPEN, "muls_per_viewing_key": MULS_VK}
    g = synth.to_mont(list(U.Model().g), U.R, 4).reshape(1, 8)
    one = synth.to_mont([1], U.R, 4)[0]
    vk = rng.integers(0, 1 << 64, size=4, dtype=np.uint64)
    vk[3] &= np.uint64((1 << 57) - 1)  # below l
    rk = api.edwards_mul(api.EDWARDS_MUL_FIXED_BASE, g, vk.reshape(1, 4))[0]
    pak = api.edwards_mul(api.EDWARDS_MUL_FIXED_BASE, g, np.array([[7, 0, 0, 0]], dtype=np.uint64))[0]

    def elements(shape):
        x = rng.integers(0, 1 << 64, size=shape + (4,), dtype=np.uint64)
        x[..., 3] %= np.uint64(P_TOP)
        return x

    for lg in (16, 20):
        n = 1 << lg
        pt = elements((n, 3))
        pt[:, 2] = api.field_op("bn254_fr", "from_canonical", np.ascontiguousarray(pt[:, 2] * np.array([1, 1, 0, 0], dtype=np.uint64)))
        flags = rng.integers(0, 2, size=n, dtype=np.uint8)
        keys = np.ascontiguousarray(np.broadcast_to(rk, (n, 8)))
        mint_ms = median_ms(lambda: model.mint(keys, pt, flags), a.reps)
        utxos, items, st = model.mint(keys, pt, flags)
        assert not st.any()
        utxos[::5, 3, 0] ^= np.uint64(1)  # a fifth of the ledger is not ours
        open_ms = median_ms(lambda: model.open(vk, pt, utxos, pak=pak), a.reps)
        st, items2, nul, n_ok = model.open(vk, pt, utxos, pak=pak)
        assert n_ok == n - len(range(0, n, 5)) and (items2[1::5] == items[1::5]).all()
        paks = elements((n, 2)).reshape(n, 8)
        vk_ms = median_ms(lambda: model.viewing_keys(paks), a.reps)
        out[f"mint_2^{lg}"] = {"ms": round(mint_ms, 3), "per_s": round(n / mint_ms * 1e3)}
        out[f"open_2^{lg}"] = {"ms": round(open_ms, 3), "per_s": round(n / open_ms * 1e3)}
        out[f"viewing_keys_2^{lg}"] = {"ms": round(vk_ms, 3), "per_s": round(n / vk_ms * 1e3)}
        if lg == 16:
            c_st, c_items, c_nul = composed_open(hashers, one, rk, pak, pt, utxos)
            assert (c_st == st).all() and (c_items == items2).all() and (c_nul == nul).all(), "the composition and mg_utxos_open disagree"
            base, new = [], []
            for _ in range(a.reps):
                base.append(timed(lambda: composed_open(hashers, one, rk, pak, pt, utxos)))
                new.append(timed(lambda: model.open(vk, pt, utxos, pak=pak)))
            bm, nm = statistics.median(base), statistics.median(new)
            out["composition_2^16"] = {"route": "three mg_poseidon_hash calls and numpy glue (parent commit)", "ms": round(bm, 3),
                                       "mg_utxos_open_ms": round(nm, 3), "ratio": round(bm / nm, 2)}

    mhz, mad_per_us_simd, _ = api.clock_probe()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    peak = mad_per_us_simd * 1e6 * 4 * cus  # wave-level v_mad_u64_u32 per second, whole chip
    out["roofline"] = {"clock_probe_mhz": round(mhz, 1), "probe_mad_per_us_per_simd": round(mad_per_us_simd, 2), "cus": cus,
                       "open_2^20_fraction_of_mad_issue_peak": round(out["open_2^20"]["per_s"] * MULS_OPEN * MADS_PER_MUL / 64.0 / peak, 4),
                       "viewing_keys_2^20_hash_fraction_of_mad_issue_peak":
                           round(out["viewing_keys_2^20"]["per_s"] * MULS_VK * MADS_PER_MUL / 64.0 / peak, 4)}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "utxo_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
