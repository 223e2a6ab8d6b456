"""Phase-2 key initialisation on the GPU (mg_mpc_initialize / mg_qap_columns): one JSON line, also written to
profiles/qap_columns_bench.json. BN254.

  initialize_<shape>     `mpc::initialize` end to end (host arrays in, the key out) on the three manta-pay shapes of
                         synth.make_shape: four group IFFTs of D points, the h_query, and the column sums of 2 nnz(A) +
                         2 nnz(B) + nnz(C) + 2 P entries in G1 and nnz(B) in G2; beside it one G1 and one G2 group IFFT of D points alone
  columns_<shape>_g1/g2  mg_qap_columns alone at those sizes -- G1: the terms A, B, C over one basis; G2: B -- with the
                         stored entries per second
  entries_per_lane_...   the G1 columns of private_transfer with the chunk length of the segmented sum fixed (0 = the default)
  columns_..._uniform_coefficients   the same call with 254-bit coefficients in every entry: what the short ladders are worth
  composition_v2048      what `ceremony.initialize` did before: element-wise multiplication on the GPU, then one host sum per
                         variable (`initialize_by_composition`), alternated in this process with `initialize` on a circuit of
                         2 048 variables; `speedup` = its median over the new call's

Every figure is the median of --reps calls after one warm-up call. The accumulators are honest powers of one tau, made with
mg_fixed_base_mul. No bar is set on any figure: parity with the oracle gates the feature (tests/test_gpu_qap_columns.py), not
a ratio.

    python tools/qap_columns_bench.py [--reps 3] [--shapes to_private,private_transfer,to_public]
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

TAU, ALPHA, BETA = 0x1111111111111111222333, 0x3333333333333333444555, 0x5555555555555555666777


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, reps):
    fn()
    return statistics.median(timed(fn) for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="to_private,private_transfer,to_public")
    a = ap.parse_args()
    from manta_rs_amd import api, ceremony, keygen, synth

    api.init(0)
    curve = api.BN254
    r = synth.FR_MODULUS[curve]

    def multiples(group, ks):
        """[k] G for every k, on the GPU"""
        lim = synth.ints_to_limbs([k % r for k in ks], 4)
        d = api.fixed_base_mul(curve, group, keygen.generator(curve, group), api.DeviceBuffer.from_numpy(lim), len(ks))
        return d.to_numpy(shape=(len(ks), api.affine_limbs(curve, group)))

    def accumulator(D):
        tp = [1] * (2 * D)
        for i in range(1, 2 * D):
            tp[i] = tp[i - 1] * TAU % r
        return ceremony.Accumulator(curve, multiples(1, tp), multiples(2, tp[:D]), multiples(1, [ALPHA * t for t in tp[:D]]),
                                    multiples(1, [BETA * t for t in tp[:D]]), multiples(2, [BETA]))

    out = {"tool": "qap_columns_bench", "reps": a.reps, "curve": "bn254"}
    for name in [s for s in a.shapes.split(",") if s]:
        c = synth.make_shape(curve, name)
        acc = accumulator(c.D)
        nnz = [len(M.col) for M in (c.A, c.B, c.C)]
        g1_entries = 2 * nnz[0] + 2 * nnz[1] + nnz[2] + 2 * c.P
        ms = median_ms(lambda: ceremony.initialize(acc, c), a.reps)
        out[f"initialize_{name}"] = {"m": c.m, "V": c.V, "P": c.P, "D": c.D, "nnz_a_b_c": nnz, "g1_entries": g1_entries,
                                     "g2_entries": nnz[1], "ms": round(ms, 1)}
        # where the rest of the call goes: one of the three G1 IFFTs and the G2 one, through mg_group_ntt (host arrays in and out)
        n1 = median_ms(lambda: ceremony.lagrange_basis(curve, 1, acc.tau_powers_g1, c.D), a.reps)
        n2 = median_ms(lambda: ceremony.lagrange_basis(curve, 2, acc.tau_powers_g2, c.D), a.reps)
        out[f"initialize_{name}"].update(group_ifft_g1_ms=round(n1, 1), group_ifft_g2_ms=round(n2, 1))
        b1, b2 = np.ascontiguousarray(acc.tau_powers_g1[:c.m]), np.ascontiguousarray(acc.tau_powers_g2[:c.m])
        ms1 = median_ms(lambda: api.qap_columns(curve, 1, [b1, b1, b1], [c.A, c.B, c.C], c.V), a.reps)
        ms2 = median_ms(lambda: api.qap_columns(curve, 2, [b2], [c.B], c.V), a.reps)
        out[f"columns_{name}_g1"] = {"entries": sum(nnz), "columns": c.V, "ms": round(ms1, 2), "entries_per_s": round(sum(nnz) / ms1 * 1e3)}
        out[f"columns_{name}_g2"] = {"entries": nnz[1], "columns": c.V, "ms": round(ms2, 2), "entries_per_s": round(nnz[1] / ms2 * 1e3)}

        if name == "private_transfer":  # where the chunk boundaries of the segmented sum go: the library's default against fixed values
            sweep = {}
            for epl in (0, 1, 2, 4, 8, 16, 64):
                sweep[str(epl)] = round(median_ms(lambda: api.qap_columns(curve, 1, [b1, b1, b1], [c.A, c.B, c.C], c.V, entries_per_lane=epl), a.reps), 2)
            out["entries_per_lane_private_transfer_g1_ms"] = sweep
            # what the short ladder is worth: the same matrices with every coefficient replaced by a uniform field element
            rng = synth.XorShift(77)
            dense = [synth.CSR(M.row_ptr, M.col, synth.to_mont([rng.field(r) for _ in range(len(M.col))], r, 4)) for M in (c.A, c.B, c.C)]
            msd = median_ms(lambda: api.qap_columns(curve, 1, [b1, b1, b1], dense, c.V), a.reps)
            out["columns_private_transfer_g1_uniform_coefficients"] = {"entries": sum(nnz), "ms": round(msd, 2), "entries_per_s": round(sum(nnz) / msd * 1e3)}

    # the composition a caller had before, where it is still practical
    c = synth.make_circuit(curve, 2300, 2048, 9, seed=2048)
    acc = accumulator(c.D)
    new_key, old_key = ceremony.initialize(acc, c), ceremony.initialize_by_composition(acc, c)
    for f in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "gamma_abc_g1"):
        assert (np.asarray(getattr(new_key, f)) == np.asarray(getattr(old_key, f))).all(), f
    old, new = [], []
    for _ in range(a.reps):
        old.append(timed(lambda: ceremony.initialize_by_composition(acc, c)))
        new.append(timed(lambda: ceremony.initialize(acc, c)))
    om, nm = statistics.median(old), statistics.median(new)
    out["composition_v2048"] = {"m": c.m, "V": c.V, "D": c.D, "nnz_a_b_c": [len(M.col) for M in (c.A, c.B, c.C)],
                                "route": "mg_group_ntt x4 + mg_ec_elementwise(MG_EC_MUL) per matrix + mg_points_sum per variable",
                                "ms": round(om, 1), "mg_mpc_initialize_ms": round(nm, 1), "speedup": round(om / nm, 2)}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "qap_columns_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
