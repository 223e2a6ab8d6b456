"""The R1CS satisfaction check (mg_ctx_r1cs_check / mg_r1cs_check) on the PrivateTransfer shape, BN254, k = 1 / 32 / 256
assignments: wall time per call of both forms, kernel time per call of `r1cs_check_kernel`, and beside it the time of
`spmv3_kernel` -- the kernel that reads the same matrices and assignments -- in the batched proving pass at the same k of ANOTHER
build of the library (the parent commit's, built with tools/build_variant.sh and named with --parent-lib). Writes
profiles/r1cs_check.txt and prints it. No bar is set on any figure: parity with the plain-integer reference gates the feature
(tests/test_gpu_r1cs_check.py), not a ratio.

Every measurement runs in a child process of its own, started from this one (which never opens the GPU): wall times untraced,
kernel times under `rocprofv3 --kernel-trace --stats` (tracing only, no counters), one traced run per library. A child that
fails ends the tool.

    python tools/r1cs_check_bench.py [--reps 10] [--parent-lib manta_rs_amd/lib/libmantagpu_parent.so]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (1, 32, 256)
Z_BYTES, MAX_BATCH, PASS = 64 << 20, 65535, 32   # prover.cpp R1CS_CHECK_Z_BYTES, FrEngine::R1CS_CHECK_MAX_BATCH; proofs per proving pass


def launches(k, V):
    """kernel launches of one check call: the chunk loop's lanes per launch"""
    lanes = min(MAX_BATCH, max(1, Z_BYTES // (V * 32)))
    return -(-k // lanes)


def child(mode, reps):
    import numpy as np
    from manta_rs_amd import api, keygen, synth
    api.init(0)
    curve = api.BN254
    p = synth.FR_MODULUS[curve]
    c = synth.make_shape(curve, "private_transfer")
    rng = synth.XorShift(5)
    ctx = api.ProvingContext(curve, keygen.generate(c, [rng.field(p) for _ in range(5)]))
    ctx.set_r1cs(api.R1CS.from_circuit(c))
    out = {"m": c.m, "V": c.V, "nnz_a_b_c": [len(M.col) for M in (c.A, c.B, c.C)]}
    for k in KS:
        zs = np.ascontiguousarray(np.broadcast_to(c.z, (k,) + c.z.shape))
        if mode == "prove":
            rs = synth.to_mont([rng.field(p) for _ in range(2 * k)], p, 4)
            for _ in range(3 + reps):   # (three warm-up passes: a slot runs eagerly twice before its graphs are captured)
                api.Groth16.prove_batch(ctx, zs, rs[:k], rs[k:])
            continue
        forms = (("context", lambda: ctx.check_assignments(zs)),
                 ("stand_alone", lambda: api.r1cs_check(curve, c.A, c.B, c.C, c.m, c.V, zs)))
        for name, call in forms:
            first, count = call()       # warm-up, and the answer
            assert (first == -1).all() and not count.any()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[f"{name}_k{k}_wall_ms"] = round(statistics.median(ts), 3)
    print("RESULT " + json.dumps(out))


def run_child(mode, reps, lib=None, traced=False):
    """the child's RESULT object and, traced, its kernel dispatches [(name, start, end)] in start order"""
    env = dict(os.environ)
    if lib:
        env["MANTA_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(reps)]
    tmp = tempfile.mkdtemp(prefix="r1cs_check_bench_") if traced else None
    if traced:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "-o", "t", "--"] + cmd
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"child {mode} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        res = [json.loads(l[7:]) for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True) if traced else []:
            for row in csv.DictReader(open(path)):
                rows.append((row["Kernel_Name"], int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
        return (res[0] if res else {}), sorted(rows, key=lambda x: x[1])
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)


def per_call_us(durations, plan, reps):
    """durations of one kernel's dispatches in start order; plan = [(label, dispatches per call, calls)] in the order the child
    made them -> {label: (median, min, max) of the kernel time per call over the last `reps` calls, in us}, or None when the
    trace holds another number of dispatches than the plan says"""
    if len(durations) != sum(per * calls for _, per, calls in plan):
        return None
    out, at = {}, 0
    for label, per, calls in plan:
        sums = [sum(durations[at + i * per: at + (i + 1) * per]) / 1e3 for i in range(calls)][-reps:]
        out[label] = (statistics.median(sums), min(sums), max(sums))
        at += per * calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "manta_rs_amd", "lib", "libmantagpu_parent.so"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    wall, _ = run_child("wall", a.reps)
    V = wall["V"]
    _, trace = run_child("check", a.reps, traced=True)
    dur = [e - s for n, s, e in trace if "r1cs_check_kernel" in n]
    plan = [(f"{form}_k{k}", launches(k, V), 1 + a.reps) for k in KS for form in ("context", "stand_alone")]
    kern = per_call_us(dur, plan, a.reps)
    spmv = None
    if os.path.exists(a.parent_lib):
        _, ptrace = run_child("prove", a.reps, lib=os.path.abspath(a.parent_lib), traced=True)
        pdur = [e - s for n, s, e in ptrace if "spmv3_kernel" in n]
        spmv = per_call_us(pdur, [(f"k{k}", -(-k // PASS), 3 + a.reps) for k in KS], a.reps)
        if spmv is None:
            spmv = {"all": (statistics.median(pdur) / 1e3, min(pdur) / 1e3, max(pdur) / 1e3)} if pdur else {}
    lines = [f"tools/r1cs_check_bench.py --reps {a.reps}: BN254, PrivateTransfer shape (m = {wall['m']}, V = {V}, nnz A | B | C = "
             f"{wall['nnz_a_b_c']}), every assignment satisfied (no atomic is issued)",
             "wall: median ms per call through the Python mirror, arrays prepared once, untraced, a process of its own",
             "kernel: r1cs_check_kernel, us per call = the sum over the call's launches (a launch holds at most "
             f"{min(MAX_BATCH, Z_BYTES // (V * 32))} assignments of this shape), median (min .. max) of {a.reps} calls under rocprofv3 "
             "--kernel-trace --stats, a run of its own",
             "spmv3: spmv3_kernel of the parent commit's library (tools/build_variant.sh) in mg_groth16_prove_batch at the same k, us "
             f"per call = the sum over its passes of {PASS} proofs, same statistic, a traced run of its own; passes of one call overlap "
             "with the MSMs of the passes beside them, the check kernel runs alone", ""]
    lines.append(f"{'k':>4} {'form':<12} {'wall ms':>9} {'kernel us':>32} {'spmv3 us (parent)':>32} {'kernel / spmv3':>15}")

    def fmt(t):
        return "-" if t is None else f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})"

    for k in KS:
        for form in ("context", "stand_alone"):
            kt = kern.get(f"{form}_k{k}") if kern else None
            st = spmv.get(f"k{k}") if spmv else None
            ratio = f"{kt[0] / st[0]:.2f}" if kt and st else "-"
            lines.append(f"{k:>4} {form:<12} {wall[f'{form}_k{k}_wall_ms']:>9.3f} {fmt(kt):>32} {fmt(st):>32} {ratio:>15}")
    if kern is None:
        lines.append(f"(the trace holds {len(dur)} r1cs_check_kernel dispatches, the plan {sum(p * c for _, p, c in plan)}: no per-call split)")
    if spmv is None:
        lines.append(f"(no library at {os.path.relpath(a.parent_lib, ROOT)}: the spmv3_kernel column is empty)")
    elif "all" in spmv:
        lines.append(f"(spmv3_kernel dispatches do not split by call; over all of them: {fmt(spmv['all'])} us per launch)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r1cs_check.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
