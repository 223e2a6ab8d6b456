"""The embedded curve and the Poseidon note encryption on the GPU (mg_edwards_*, mg_notes_*): one JSON line, also written to
profiles/edwards_bench.json.

  key_agreement_2^16 / _2^20   `epk * vk` per second: mg_edwards_mul, one shared scalar over n points (host arrays in and out)
  fixed_base_2^16 / _2^20      `G * sk` per second: mg_edwards_mul, n scalars over one base (table built per call, included)
  pairwise_2^16                n scalars x n points
  decrypt_2^16 / _2^20         notes opened per second end to end, mg_notes_decrypt (host arrays in and out)
  encrypt_2^16                 notes encrypted per second, mg_notes_encrypt
  baseline_2^10                the parent's only GPU route to the same key agreement: double-and-add in extended coordinates
                               composed from vectorised mg_field_op calls, alternated with mg_edwards_mul in this process;
                               `speedup` = its median over mg_edwards_mul's
  roofline                     v_mad_u64_u32 issue of the key agreement at 2^20 as a fraction of the peak mg_clock_probe measures
                               in the same run (the call includes the host copies, so this is a lower bound on the kernel's)

Every figure is the median of --reps calls after one warm-up call.

    python tools/edwards_bench.py [--reps 5]
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

P = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
# v_mad_u64_u32 per Montgomery product of Fp<Bn254FrCfg> in the gfx950 disassembly (tools/isa_hist.py): 2 x 8 x 8
MADS_PER_MUL = 128


def muls_shared(k):
    """field products of one lane of the shared-scalar kernel for scalar k: 8 per doubling (one per bit), 8 per addition (one
    per set bit), 2 for d x y, the Fermat inversion (256 squarings + one product per set bit of p - 2) and 2 to normalise"""
    return 8 * k.bit_length() + 8 * bin(k).count("1") + 2 + 256 + bin(P - 2).count("1") + 2


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, reps):
    fn()
    return statistics.median(timed(fn) for _ in range(reps))


def field_op_mul(api, pts, k, d):
    """[n, 8] affine points x scalar k by double-and-add in extended coordinates, every field operation one mg_field_op call
    over the batch; returns projective X, Y, Z (the comparison cross-multiplies)"""
    f = lambda op, a, b=None: api.field_op("bn254_fr", op, a, b) if b is not None else api.field_op("bn254_fr", op, a)
    n = pts.shape[0]
    x, y = np.ascontiguousarray(pts[:, :4]), np.ascontiguousarray(pts[:, 4:])
    dt = f("mul", np.ascontiguousarray(np.broadcast_to(d, (n, 4))), f("mul", x, y))
    xy = f("add", x, y)
    one = api.field_op("bn254_fr", "from_canonical", np.ascontiguousarray(np.broadcast_to(np.array([1, 0, 0, 0], dtype=np.uint64), (n, 4))))
    X, Y, Z, T = np.zeros((n, 4), dtype=np.uint64), one.copy(), one.copy(), np.zeros((n, 4), dtype=np.uint64)
    for bit in bin(k)[2:]:
        A, B = f("sqr", X), f("sqr", Y)
        zz = f("sqr", Z)
        C = f("add", zz, zz)
        E = f("sub", f("sub", f("sqr", f("add", X, Y)), A), B)
        G = f("add", A, B)
        F, H = f("sub", G, C), f("sub", A, B)
        X, Y, Z, T = f("mul", E, F), f("mul", G, H), f("mul", F, G), f("mul", E, H)
        if bit == "1":
            A, B, C = f("mul", X, x), f("mul", Y, y), f("mul", T, dt)
            E = f("sub", f("sub", f("mul", f("add", X, Y), xy), A), B)
            F, G, H = f("sub", Z, C), f("add", Z, C), f("sub", B, A)
            X, Y, Z, T = f("mul", E, F), f("mul", G, H), f("mul", F, G), f("mul", E, H)
    return X, Y, Z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from manta_rs_amd import api, synth
    import torch
    import edwards_ref as E

    api.init(0)
    pdir = os.path.join(ROOT, "tests", "golden", "manta_parameters")
    g = synth.to_mont(list(E.generator()), E.R, 4).reshape(1, 8)
    cipher = api.NoteCipher(open(os.path.join(pdir, "incoming-base-encryption-scheme.dat"), "rb").read(), g)
    rng = np.random.default_rng(2026)
    out = {"tool": "edwards_bench", "reps": a.reps, "curve": "ed_on_bn254", "chunk": api.EDWARDS_CHUNK}

    def scalars(n):
        s = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        s[:, 3] &= np.uint64((1 << 58) - 1)
        s[:, 3] |= np.uint64(1 << 57)  # 250 bits, below l
        return s

    vk = scalars(1)
    vk_int = synth.limbs_to_ints(vk)[0]
    pk = api.edwards_mul(api.EDWARDS_MUL_FIXED_BASE, g, vk)

    # baseline vs mg_edwards_mul at 2^10, alternated
    n = 1 << 10
    pts = api.edwards_mul(api.EDWARDS_MUL_FIXED_BASE, g, scalars(n))
    d = synth.to_mont([E.D], E.R, 4)[0]
    want = api.edwards_mul(api.EDWARDS_MUL_SHARED_SCALAR, pts, vk)
    X, Y, Z = field_op_mul(api, pts, vk_int, d)
    fm = lambda u, v: api.field_op("bn254_fr", "mul", np.ascontiguousarray(u), np.ascontiguousarray(v))
    assert (fm(want[:, :4], Z) == X).all() and (fm(want[:, 4:], Z) == Y).all(), "the composed baseline and mg_edwards_mul disagree"
    base, new = [], []
    for _ in range(a.reps):
        base.append(timed(lambda: field_op_mul(api, pts, vk_int, d)))
        new.append(timed(lambda: api.edwards_mul(api.EDWARDS_MUL_SHARED_SCALAR, pts, vk)))
    bm, nm = statistics.median(base), statistics.median(new)
    out["baseline_2^10"] = {"route": "mg_field_op composition (parent commit), projective result", "ms": round(bm, 1),
                            "per_s": round(n / bm * 1e3), "mg_edwards_mul_ms": round(nm, 3), "speedup": round(bm / nm, 1)}

    for lg in (16, 20):
        n = 1 << lg
        sc = scalars(n)
        fixed_ms = median_ms(lambda: api.edwards_mul(api.EDWARDS_MUL_FIXED_BASE, g, sc), a.reps)
        pts = api.edwards_mul(api.EDWARDS_MUL_FIXED_BASE, g, sc)
        ka_ms = median_ms(lambda: api.edwards_mul(api.EDWARDS_MUL_SHARED_SCALAR, pts, vk), a.reps)
        out[f"fixed_base_2^{lg}"] = {"ms": round(fixed_ms, 3), "per_s": round(n / fixed_ms * 1e3)}
        out[f"key_agreement_2^{lg}"] = {"ms": round(ka_ms, 3), "per_s": round(n / ka_ms * 1e3)}
        pt = rng.integers(0, 1 << 64, size=(n, 3, 4), dtype=np.uint64)
        pt[..., 3] %= np.uint64(0x30644e72e131a029)  # below p's top limb: canonical
        pt[:, 2] = api.field_op("bn254_fr", "from_canonical", np.ascontiguousarray(pt[:, 2] * np.array([1, 1, 0, 0], dtype=np.uint64)))
        keys = np.ascontiguousarray(np.broadcast_to(pk, (n, 8)))
        if lg == 16:
            pw_ms = median_ms(lambda: api.edwards_mul(api.EDWARDS_MUL_PAIRWISE, pts, sc), a.reps)
            out["pairwise_2^16"] = {"ms": round(pw_ms, 3), "per_s": round(n / pw_ms * 1e3)}
            enc_ms = median_ms(lambda: cipher.encrypt(keys, sc, pt), a.reps)
            out["encrypt_2^16"] = {"ms": round(enc_ms, 3), "per_s": round(n / enc_ms * 1e3)}
        epk, ct, tag = cipher.encrypt(keys, sc, pt)
        dec_ms = median_ms(lambda: cipher.decrypt(vk[0], epk, ct, tag), a.reps)
        got, ok, _ = cipher.decrypt(vk[0], epk, ct, tag)
        assert ok.all() and (got == pt).all()
        out[f"decrypt_2^{lg}"] = {"ms": round(dec_ms, 3), "per_s": round(n / dec_ms * 1e3)}

    mhz, mad_per_us_simd, _ = api.clock_probe()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    peak = mad_per_us_simd * 1e6 * 4 * cus  # wave-level v_mad_u64_u32 per second, whole chip
    mads = muls_shared(vk_int) * MADS_PER_MUL
    rate = out["key_agreement_2^20"]["per_s"] * mads / 64.0
    out["roofline"] = {"muls_per_key_agreement": muls_shared(vk_int), "mads_per_key_agreement": mads, "clock_probe_mhz": round(mhz, 1),
                       "probe_mad_per_us_per_simd": round(mad_per_us_simd, 2), "cus": cus,
                       "key_agreement_2^20_fraction_of_mad_issue_peak": round(rate / peak, 3)}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "edwards_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
