"""Batched point codec on the GPU (mg_proofs_decode / mg_points_decode): one JSON line.

  proofs_256          256 BN254 PrivateTransfer-shape proofs (distinct blinding, one assignment) decoded and checked:
                      mg_proofs_decode against the host mg_proof_decode loop, same process, same bytes
  bls381_g1_2^20      2^20 compressed BLS12-381 G1 points, checked (curve + [r]P == O): points/s
  g2_2^16             2^16 compressed G2 points per curve, checked: points/s
  bn254_g2_2^16_formats  the same 2^16 Bn254 G2 points as arkworks and as PPoT records (mg_ppot_points_decode), alternated

GPU figures are the median of five calls after one warm-up call, host bytes in and host limbs out included; the host loop is
timed once over all 256 proofs. The big batches repeat 4 096 distinct points (made on the GPU from the generator): the work
per point does not depend on its value.

    python tools/point_codec_bench.py [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def distinct_points(api, keygen, synth, curve, group, n, seed):
    rng = synth.XorShift(seed)
    r = synth.FR_MODULUS[curve]
    g = np.tile(keygen.generator(curve, group), (n, 1))
    ks = synth.ints_to_limbs([rng.field(r) for _ in range(n)], 4)
    return api.ec_elementwise(curve, group, api.EC_MUL, g, ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--formats-only", action="store_true", help="only the arkworks / PPoT comparison")
    a = ap.parse_args()
    import bench
    from manta_rs_amd import api, keygen, synth

    api.init(0)
    out = {"tool": "point_codec_bench", "reps": a.reps}
    if a.formats_only:
        out["bn254_g2_2^16_formats"] = formats(api, keygen, synth, a.reps)
        print(json.dumps(out))
        return

    ps = bench.ProveSetup("private_transfer", "W")
    k = 256
    rng = synth.XorShift(0x5EED)
    p = synth.FR_MODULUS[ps.curve]
    rs = synth.to_mont([rng.field(p) for _ in range(2 * k)], p, 4).reshape(2, k, 4)
    proofs = api.Groth16.prove_batch(ps.ctx, np.stack([ps.c.z] * k), rs[0], rs[1])
    ps.release_gpu()
    data = b"".join(proofs)
    gpu_ms = median_ms(lambda: api.proofs_decode(ps.curve, data), a.reps)
    pts, ok = api.proofs_decode(ps.curve, data)
    t0 = time.perf_counter()
    host = [api.proof_decode(ps.curve, pr) for pr in proofs]
    host_ms = (time.perf_counter() - t0) * 1e3
    assert ok.all() and all((pts[i] == host[i]).all() for i in range(k)), "GPU and host decoders disagree"
    out["proofs_256"] = {"curve": "bn254", "shape": "private_transfer", "gpu_ms": round(gpu_ms, 3), "host_loop_ms": round(host_ms, 2),
                         "host_over_gpu": round(host_ms / gpu_ms, 1)}

    for curve, group, lg, name in ((1, 1, 20, "bls381_g1_2^20"), (0, 2, 16, "bn254_g2_2^16"), (1, 2, 16, "bls381_g2_2^16")):
        n = 1 << lg
        base = distinct_points(api, keygen, synth, curve, group, 4096, seed=lg + 10 * curve + group)
        enc = api.points_encode(curve, group, base) * (n // 4096)
        ms = median_ms(lambda: api.points_decode(curve, group, enc), a.reps)
        got, st = api.points_decode(curve, group, enc)
        assert (st == 0).all() and (got[:4096] == base).all() and (got[-4096:] == base).all()
        out[name] = {"n": n, "compressed": True, "checked": True, "ms": round(ms, 2), "points_per_s": round(n / ms * 1e3)}
    out["bn254_g2_2^16_formats"] = formats(api, keygen, synth, a.reps)
    print(json.dumps(out))


def formats(api, keygen, synth, reps):
    """the same 2^16 Bn254 G2 points as arkworks and as PPoT compressed records, checked, the two calls alternated"""
    n = 1 << 16
    base = distinct_points(api, keygen, synth, 0, 2, 4096, seed=1717)
    ark = api.points_encode(0, 2, base) * (n // 4096)
    ppot = api.ppot_points_encode(2, base, True) * (n // 4096)
    calls = {"arkworks": lambda: api.points_decode(0, 2, ark), "ppot": lambda: api.ppot_points_decode(2, ppot, True)}
    for fn in calls.values():
        got, st = fn()
        assert (st == 0).all() and (got[:4096] == base).all() and (got[-4096:] == base).all()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {"n": n, "compressed": True, "checked": True,
            **{k + "_ms": {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in ts.items()}}


if __name__ == "__main__":
    main()
