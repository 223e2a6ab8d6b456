"""Batched Poseidon and Merkle hashing on the GPU (mg_poseidon_*, mg_merkle_*): one JSON line, also written to
profiles/poseidon_bench.json.

  hash_2^16 / hash_2^20   BN254 Poseidon2 hashes (utxo-accumulator-model parameters, width 3) per second, through
                          mg_poseidon_hash (host arrays in and out) and mg_poseidon_hash_device (HBM in and out)
  baseline_2^16           the parent's only GPU route to the same 2^16 digests: the permutation composed from vectorised
                          mg_field_op calls (add keys, x^5, MDS product per round), alternated with mg_poseidon_hash in this
                          process; `speedup` = its median over mg_poseidon_hash's
  tree_2^19               root of a full height-20 tree (2^19 leaves), mg_merkle_tree
  forest_2^20             roots of 256 height-20 trees holding 2^20 leaves, mg_merkle_forest_roots
  roofline                v_mad_u64_u32 issue of hash_device at 2^20 as a fraction of the peak mg_clock_probe measures

Every figure is the median of --reps calls after one warm-up call.

    python tools/poseidon_bench.py [--reps 5]
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

# v_mad_u64_u32 per width-3 hash: 804 Montgomery products (8 x (3 t + t^2) + 55 x (3 + t^2), t = 3) of 128 each, the count in
# the gfx950 disassembly of Fp<Bn254FrCfg>::mul (tools/isa_hist.py); the kernels issue no other v_mad_u64_u32 per round
MADS_PER_HASH = 804 * 128


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, reps):
    fn()
    return statistics.median(timed(fn) for _ in range(reps))


def field_op_hash(api, p_keys, p_mds, tag, inputs, full, partial):
    """the digests composed from mg_field_op: [n, 2, 4] inputs -> [n, 4]"""
    n = inputs.shape[0]
    st = np.concatenate([np.broadcast_to(tag.reshape(1, 1, 4), (n, 1, 4)), inputs], axis=1).reshape(n * 3, 4)
    hf = full // 2
    mds_t = np.ascontiguousarray(np.broadcast_to(p_mds.reshape(1, 9, 4), (n, 9, 4)).reshape(-1, 4))
    for r in range(full + partial):
        keys = np.ascontiguousarray(np.broadcast_to(p_keys[r].reshape(1, 3, 4), (n, 3, 4)).reshape(-1, 4))
        st = api.field_op("bn254_fr", "add", st, keys)
        if r < hf or r >= hf + partial:
            x2 = api.field_op("bn254_fr", "sqr", st)
            st = api.field_op("bn254_fr", "mul", api.field_op("bn254_fr", "sqr", x2), st)
        else:
            w0 = np.ascontiguousarray(st.reshape(n, 3, 4)[:, 0])
            x2 = api.field_op("bn254_fr", "sqr", w0)
            s3 = st.reshape(n, 3, 4).copy()
            s3[:, 0] = api.field_op("bn254_fr", "mul", api.field_op("bn254_fr", "sqr", x2), w0)
            st = s3.reshape(-1, 4)
        # new[i] = sum_j mds[3 i + j] st[j]: one product call over n x 9, two sums over n x 3
        rep = np.ascontiguousarray(np.broadcast_to(st.reshape(n, 1, 3, 4), (n, 3, 3, 4)).reshape(-1, 4))
        pr = api.field_op("bn254_fr", "mul", mds_t, rep).reshape(n, 3, 3, 4)
        acc = api.field_op("bn254_fr", "add", np.ascontiguousarray(pr[:, :, 0].reshape(-1, 4)),
                           np.ascontiguousarray(pr[:, :, 1].reshape(-1, 4)))
        st = api.field_op("bn254_fr", "add", acc, np.ascontiguousarray(pr[:, :, 2].reshape(-1, 4)))
    return st.reshape(n, 3, 4)[:, 0].copy()


def rand_mont(rng, shape):
    x = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    x[..., 3] %= np.uint64(0x30644e72e131a029)  # below r's top limb: canonical
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from manta_rs_amd import api
    import torch

    api.init(0)
    data = open(os.path.join(ROOT, "tests", "golden", "manta_parameters", "utxo-accumulator-model.dat"), "rb").read()
    h = api.PoseidonHasher.decode(api.BN254, data)
    full, partial = h.full_rounds, h.partial_rounds
    # the parameters in Montgomery form for the composed baseline, converted from the canonical bytes by mg_field_op
    els = np.frombuffer(data, dtype=np.uint64).reshape(-1, 4).copy()
    mont = api.field_op("bn254_fr", "from_canonical", els)
    nk = (full + partial) * 3
    p_keys, p_mds, tag = mont[:nk].reshape(-1, 3, 4), mont[nk:nk + 9], mont[-1]
    rng = np.random.default_rng(2026)
    out = {"tool": "poseidon_bench", "reps": a.reps, "hasher": "bn254 Poseidon2 (utxo-accumulator-model.dat, width 3, 8 + 55 rounds)"}

    # baseline vs mg_poseidon_hash at 2^16, alternated
    n = 1 << 16
    x = rand_mont(rng, (n, 2))
    want = h.hash(x)
    got = field_op_hash(api, p_keys, p_mds, tag, x, full, partial)
    assert (got == want).all(), "the composed baseline and mg_poseidon_hash disagree"
    base, new = [], []
    for _ in range(a.reps):
        base.append(timed(lambda: field_op_hash(api, p_keys, p_mds, tag, x, full, partial)))
        new.append(timed(lambda: h.hash(x)))
    bm, nm = statistics.median(base), statistics.median(new)
    out["baseline_2^16"] = {"route": "mg_field_op composition (parent commit)", "ms": round(bm, 2), "hashes_per_s": round(n / bm * 1e3),
                            "mg_poseidon_hash_ms": round(nm, 3), "speedup": round(bm / nm, 1)}

    for lg in (16, 20):
        n = 1 << lg
        x = rand_mont(rng, (n, 2))
        host_ms = median_ms(lambda: h.hash(x), a.reps)
        d_in = api.DeviceBuffer.from_numpy(x)
        d_out = api.DeviceBuffer(n * 32)
        dev_ms = median_ms(lambda: h.hash_device(d_in, n, d_out), a.reps)
        assert (d_out.to_numpy(shape=(n, 4)) == h.hash(x)).all()
        out[f"hash_2^{lg}"] = {"hash_ms": round(host_ms, 3), "hash_per_s": round(n / host_ms * 1e3),
                               "hash_device_ms": round(dev_ms, 3), "hash_device_per_s": round(n / dev_ms * 1e3)}
        d_in.free()
        d_out.free()

    # roofline of hash_device at 2^20
    mhz, mad_per_us_simd, _ = api.clock_probe()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    peak = mad_per_us_simd * 1e6 * 4 * cus  # wave-level v_mad_u64_u32 per second, whole chip
    rate = out["hash_2^20"]["hash_device_per_s"] * MADS_PER_HASH / 64.0
    out["roofline"] = {"mads_per_hash": MADS_PER_HASH, "clock_probe_mhz": round(mhz, 1), "probe_mad_per_us_per_simd": round(mad_per_us_simd, 2),
                       "cus": cus, "fraction_of_mad_issue_peak": round(rate / peak, 3)}

    lv = rand_mont(rng, (1 << 19,))
    out["tree_2^19"] = {"height": 20, "leaves": 1 << 19, "ms": round(median_ms(lambda: api.merkle_tree(h, 20, lv), a.reps), 2)}
    counts = np.full(256, 1 << 12, dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    lv = rand_mont(rng, (1 << 20,))
    out["forest_2^20"] = {"trees": 256, "height": 20, "leaves": 1 << 20,
                          "ms": round(median_ms(lambda: api.merkle_forest_roots(h, 20, lv, off), a.reps), 2)}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "poseidon_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
