"""The batched Schnorr authorization signatures on the GPU (mg_signatures_verify, mg_signatures_sign, mg_schnorr_challenges): one
JSON line, also written to profiles/schnorr_bench.json.

  verify_2^16 / _2^20 x 256 B / 2 KiB   signatures verified per second, mg_signatures_verify (host arrays in, statuses out)
  sign_...                              signatures made per second with their verifying keys, mg_signatures_sign
  challenge_share_...                   mg_schnorr_challenges on the same batch over mg_signatures_verify: the share of a
                                        verification that is the hash and the copy of the message rows (both calls copy them)
  composition_2^16                      the route a caller had before, alternated in this process with mg_signatures_verify on the
                                        same 256-byte batch: mg_edwards_encode of the keys and nonce points, hashlib.blake2s and the
                                        reduction mod l per signature on the host, mg_edwards_mul fixed-base (s G) and pairwise
                                        (h pk), mg_edwards_add (R + h pk) and a numpy compare; `ratio` = its median over the call's

Every figure is the median of --reps calls after one warm-up call. The 2^20 batches tile the 2^16 one (the 2 KiB one is 2 GiB of
message rows on the host).

    python tools/schnorr_bench.py [--reps 5]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAG = b"manta-pay/1.0.0/Schnorr-hash"


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, reps):
    fn()
    return statistics.median(timed(fn) for _ in range(reps))


def composed_verify(api, g, order, pk, rp, s, msg):
    """the statuses of mg_signatures_verify for a batch of well-encoded lanes, from the calls a caller had before"""
    n = pk.shape[0]
    epk, erp = api.edwards_encode(pk), api.edwards_encode(rp)
    rows = msg.tobytes()
    stride = msg.shape[1]
    h = [int.from_bytes(hashlib.blake2s(TAG + epk[32 * i:32 * i + 32] + erp[32 * i:32 * i + 32]
                                        + rows[stride * i:stride * (i + 1)]).digest(), "little") % order for i in range(n)]
    sg = api.edwards_mul(api.EDWARDS_MUL_FIXED_BASE, g, s)
    hpk = api.edwards_mul(api.EDWARDS_MUL_PAIRWISE, pk, api.edwards_scalars(h))
    rhs = api.edwards_add(rp, hpk)
    degenerate, equal = (sg == rp).all(axis=1), (sg == rhs).all(axis=1)
    return np.where(degenerate, api.SIG_DEGENERATE, np.where(equal, api.SIG_OK, api.SIG_MISMATCH)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from manta_rs_amd import api, synth
    import utxo_ref as U

    api.init(0)
    model = api.UtxoModel(*[U.read(n) for n in U.FILES])
    g = synth.to_mont(list(U.Model().g), U.R, 4).reshape(1, 8)
    rng = np.random.default_rng(2027)
    out = {"tool": "schnorr_bench", "reps": a.reps}

    def below_l(n):
        x = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        x[:, 3] &= np.uint64((1 << 57) - 1)
        return x

    n0 = 1 << 16
    sk0, k0 = below_l(n0), below_l(n0)
    for size, label in ((256, "256B"), (2048, "2KiB")):
        msg0 = rng.integers(0, 256, size=(n0, size), dtype=np.uint8)
        for lg in (16, 20):
            n, rep = 1 << lg, 1 << (lg - 16)
            sk, k, msg = np.tile(sk0, (rep, 1)), np.tile(k0, (rep, 1)), np.tile(msg0, (rep, 1))
            sign_ms = median_ms(lambda: model.sign(sk, k, msg), a.reps)
            s, rp, pk = model.sign(sk, k, msg)
            s[::5, 0] ^= np.uint64(1)  # a fifth of the signatures is forged
            verify_ms = median_ms(lambda: model.verify_signatures(pk, rp, s, msg), a.reps)
            st, n_ok = model.verify_signatures(pk, rp, s, msg)
            assert n_ok == n - len(range(0, n, 5)) and not st[1::5].any() and (st[::5] == api.SIG_MISMATCH).all()
            ch_ms = median_ms(lambda: model.schnorr_challenges(pk, rp, msg), a.reps)
            key = f"2^{lg}_{label}"
            out[f"sign_{key}"] = {"ms": round(sign_ms, 3), "per_s": round(n / sign_ms * 1e3)}
            out[f"verify_{key}"] = {"ms": round(verify_ms, 3), "per_s": round(n / verify_ms * 1e3)}
            out[f"challenge_share_{key}"] = {"challenges_ms": round(ch_ms, 3), "share_of_verify": round(ch_ms / verify_ms, 3)}
            if lg == 16 and size == 256:
                c_st = composed_verify(api, g, api.EDWARDS_ORDER, pk, rp, s, msg)
                assert (c_st == st).all(), "the composition and mg_signatures_verify disagree"
                base, new = [], []
                for _ in range(a.reps):
                    base.append(timed(lambda: composed_verify(api, g, api.EDWARDS_ORDER, pk, rp, s, msg)))
                    new.append(timed(lambda: model.verify_signatures(pk, rp, s, msg)))
                bm, nm = statistics.median(base), statistics.median(new)
                out["composition_2^16"] = {"route": "mg_edwards_encode x 2, hashlib.blake2s per signature, mg_edwards_mul fixed-base and "
                                                    "pairwise, mg_edwards_add, numpy compare (parent commit)",
                                           "message_bytes": size, "ms": round(bm, 3), "mg_signatures_verify_ms": round(nm, 3),
                                           "ratio": round(bm / nm, 2)}
            del sk, k, msg, s, rp, pk
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "schnorr_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
