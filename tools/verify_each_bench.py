"""Per-proof verdicts for a block of Groth16 proofs (mg_groth16_verify_each): one JSON line, also written to a file.

BN254, PrivateTransfer shape (27 instance variables), k = 256 and k = 16 proofs of one key (distinct blinding, one assignment),
all in one process, straight through the C ABI on arrays prepared once:

  each_ms        (a) mg_groth16_verify_each over the k rows
  loop_ms        (b) the loop of k mg_groth16_verify calls it replaces -- the fallback mg_groth16_verify_batch used to name
  batch_ms       (c) mg_groth16_verify_batch, which answers with one bit: for scale
  each_spoiled_ms  (a) again with one row's C replaced by another proof's: the time does not depend on the verdicts
  loop_over_each   (b) / (a)

Every figure is the median of five calls after one warm-up call.

    python tools/verify_each_bench.py [--reps 5] [--out profiles/verify_each_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_each_bench.json"))
    a = ap.parse_args()
    import bench
    from manta_rs_amd import api, synth

    api.init(0)
    ps = bench.ProveSetup("private_transfer", "W")
    curve, K = ps.curve, 256
    rng = synth.XorShift(0x5EED)
    p = synth.FR_MODULUS[curve]
    rs = synth.to_mont([rng.field(p) for _ in range(2 * K)], p, 4).reshape(2, K, 4)
    proofs = api.Groth16.prove_batch(ps.ctx, np.stack([ps.c.z] * K), rs[0], rs[1])
    ps.release_gpu()
    rows, ok = api.proofs_decode(curve, proofs)
    assert ok.all()
    vctx = api.VerifyingContext(curve, ps.pk)
    inputs = np.ascontiguousarray(np.stack([ps.c.z[1:ps.c.P]] * K), dtype=np.uint64)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    rnd = np.random.RandomState(7).randint(1, 1 << 62, size=(K, 2)).astype(np.uint64)
    w1 = api.affine_limbs(curve, 1)
    vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    L, h = api.LIB, vctx.handle

    out = {"tool": "verify_each_bench", "curve": "bn254", "shape": "private_transfer", "n_inputs": int(ps.c.P), "reps": a.reps,
           "chunk": api.VERIFY_EACH_CHUNK}
    for k in (256, 16):
        inp, pts = inputs[:k], rows[:k]
        bad = pts.copy()
        bad[k // 2, 3 * w1:] = pts[(k // 2 + 1) % k, 3 * w1:]
        verdicts = np.zeros(k, dtype=np.uint8)
        one = ctypes.c_int(0)
        singles = [(vp(inp[i]), vp(pts[i])) for i in range(k)]

        def each(points=pts):
            rc = L.mg_groth16_verify_each(h, ctypes.c_uint64(k), vp(inp), vp(points), vp(verdicts))
            assert rc == 0, rc

        def loop():
            n_ok = 0
            for x, y in singles:
                rc = L.mg_groth16_verify(h, x, y, ctypes.byref(one))
                assert rc == 0, rc
                n_ok += one.value
            assert n_ok == k

        def batch():
            rc = L.mg_groth16_verify_batch(h, ctypes.c_uint64(k), vp(inp), vp(pts), vp(rnd), ctypes.byref(one))
            assert rc == 0 and one.value == 1, (rc, one.value)

        each_ms = median_ms(each, a.reps)
        assert verdicts.all()
        loop_ms = median_ms(loop, a.reps)
        batch_ms = median_ms(batch, a.reps)
        spoiled_ms = median_ms(lambda: each(bad), a.reps)
        want = np.ones(k, dtype=np.uint8)
        want[k // 2] = 0
        assert (verdicts == want).all(), "the spoiled row, and only it, is rejected"
        out["k_%d" % k] = {"each_ms": round(each_ms, 3), "loop_ms": round(loop_ms, 2), "batch_ms": round(batch_ms, 3),
                           "each_spoiled_ms": round(spoiled_ms, 3), "loop_over_each": round(loop_ms / each_ms, 1)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
