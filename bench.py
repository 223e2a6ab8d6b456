#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X Groth16 hot path.

A plain run (`python bench.py --gpus N --steps K --warmup W`) measures the first half alone: it sets up, warms up, times K steps
of the pipelined MSM and prints the line (`metric`, `value`, `ms_per_step`, ...); `--dump-outputs DIR` also writes the point the
last timed step returned. Every other leg described here runs with `--full`.

BASELINE.json's metric has two halves and the `--full` line carries both:

  "G1 MSM Mscalar/s at 2^20"  (the line's `metric` / `value`; configs[1] = "2^20 BLS12-381 G1 variable-base MSM,
      synthetic scalars/bases, 1 MI355X"). A step = one full MSM (digits -> sort -> bucket accumulate -> merge ->
      bucket reduce -> host fold to one affine point) over n = 2^20 scalars already resident in HBM, against bases
      registered (resident, with their 2^(c w) multiples) before timing.
  "Groth16 proofs/sec (manta-pay PrivateTransfer)"  (the line's `proofs` object): whole proofs of the shape-exact
      PrivateTransfer circuit (BN254, D = 2^16, V = 35 175, P = 27) through mg_groth16_prove / _prove_batch --
      sequential latency, two host threads on one context, and batches of 256 -- with its own cpu_baseline.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

N > 1 (weak scaling, the line's `value`): the global MSM has N * 2^20 terms, sharded by contiguous base/scalar range,
one process per GPU; every step ends with an RCCL all_gather of the N partial points (96 B each, xGMI) and the local
N-term sum (manta_rs_amd/distributed.py) -- SURVEY.md section 8(e). value = N * 2^20 * K / t, t = max over ranks. The
same run also measures STRONG scaling (`strong_scaling`: a fixed 2^20-term and a fixed 35 174-term MSM split N ways)
and the proofs half as replicas (no collective).

`roofline` is for the dominant kernel (bucket accumulate), timed live with HIP events on the stream it runs on;
`cpu_baseline` is the arkworks-algorithm CPU restatement (oracle/) on the GPU box's host: 1 thread (what the
reference ships) and all cores (arkworks' `parallel` decomposition), on the same inputs.
"""
import argparse
import json
import os
import shutil
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LOG_N = int(os.environ.get("MANTA_BENCH_LOGN", "20"))  # 20 = the BASELINE config; smaller n only for studies
CURVE = 1  # BLS12-381
WINDOW_BITS = int(os.environ.get("MANTA_BENCH_C", "17"))  # 255 = 15 x 17: fifteen signed windows (scalars above r / 2 are negated)
DEPTH = int(os.environ.get("MANTA_BENCH_DEPTH", "3"))  # MSMs in flight (each on its own stream + workspace)
ALGO_BYTES_PER_SCALAR = 128  # 32 B scalar + 96 B affine G1 base (BLS12-381)
HBM_PEAK_GBPS = 8000.0       # MI355X_MICROARCH.md: 8 TB/s spec
# v_mad_u64_u32 per mixed addition (ec_dev.h madd_lazy): 6 products + 2 squarings + one fused a*b + c*d product with a single
# reduction. Round 4: BLS12-381 Fq is 13 limbs of 30 bits -- 2 K^2 + K = 351 per product, K(K+1)/2 + K^2 + K = 273 per squaring,
# 3 K^2 + K = 520 for the fused one: 3 172 (rounds 2-3, 14 x 28 bits: 6 x 406 + 2 x 315 + 602 = 3 668; round 1: 3 878)
MADS_PER_MIXED_ADD = 6 * 351 + 2 * 273 + 520
MADS_PER_MIXED_ADD_R3 = 6 * 406 + 2 * 315 + 602
PEAK_TMAD_S_ASSUMED = 1024 * 64 / 4.2 * 2.4e9 / 1e12  # 1024 SIMDs x 64 lanes / 4.2 cycles (profiles/r01_ubench2_mad_u64_u32.txt) x an ASSUMED 2.4 GHz

BLS_G1 = (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
          0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)
S0, S1 = 0x243F6A8885A308D313198A2E03707344, 0x9E3779B97F4A7C15F39CC0605CEDC835


def pmc_traffic():
    """HBM traffic of the accumulate kernel measured by THIS run: two child runs of the MSM headline under
    `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes: the two counters do not fit one,
    MI355X_MICROARCH.md "rocprofv3 PMC slots"), per-launch average over the launches of accumulate_chunks. Raw counter values
    (KiB): the 2x correction of the guide applies to wide coalesced streaming reads; this kernel's pattern -- one 128 B gather per
    mixed addition -- was calibrated with a gather-only twin (profiles/r02_pmc_and_gather_calibration.txt) and is not
    under-reported. Returns None when rocprofv3 is not available."""
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not exe:
        return None
    out = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="mg_pmc_", dir="/tmp")
        # one MSM at a time on an ordinary stream: the counters of a dispatch are then that kernel's alone (with three MSMs in flight on
        # hardware queues of their own, the neighbours' digit / sort kernels run beside the accumulate kernel and their bytes land in
        # its sample: 3.0 GB instead of 1.95 GB per launch, round 6)
        env = dict(os.environ, TMPDIR="/tmp", MANTA_BENCH_NO_PMC="1", MANTA_BENCH_DEPTH="1", MANTA_MSM_DEDICATED_QUEUES="0")
        cmd = [exe, "--kernel-trace", "--pmc", counter, "-d", d, "-o", "m", "--", sys.executable, os.path.abspath(__file__), "--full", "--workload", "msm",
               "--quick", "--no-cpu-baseline", "--steps", "3", "--warmup", "1"]
        r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=600)
        dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
        if r.returncode != 0 or not dbs:
            shutil.rmtree(d, ignore_errors=True)
            return {"error": "rocprofv3 --pmc %s failed: %s" % (counter, (r.stderr or r.stdout)[-300:])}
        db = sqlite3.connect(dbs[0])
        rows = list(db.execute("select count(*), sum(value) from counters_collection where kernel_name like '%accumulate_chunks%' and counter_name = ?",
                               (counter,)))
        db.close()
        shutil.rmtree(d, ignore_errors=True)
        if not rows or not rows[0][0]:
            return {"error": "no %s rows for accumulate_chunks" % counter}
        out[counter] = (int(rows[0][0]), float(rows[0][1]) / rows[0][0])
    kib = out["FETCH_SIZE"][1] + out["WRITE_SIZE"][1]
    return {"hbm_bytes_per_launch": int(kib * 1024), "FETCH_SIZE_KiB_per_launch": round(out["FETCH_SIZE"][1], 1),
            "WRITE_SIZE_KiB_per_launch": round(out["WRITE_SIZE"][1], 1), "launches_averaged": out["FETCH_SIZE"][0]}


def hbm_reference():
    """on-box figures next to the 8 TB/s vendor peak `roofline.peak` uses: device-to-device copy and a
    triad-like a + b -> b over 1 GiB operands (torch, current device)"""
    import torch
    n = 1 << 28  # 1 GiB of float32
    a = torch.empty(n, dtype=torch.float32, device="cuda").normal_()
    b = torch.empty_like(a)

    def timeit(f, reps=8):
        f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps
    tc = timeit(lambda: b.copy_(a))
    tt = timeit(lambda: torch.add(a, b, out=b))
    del a, b
    torch.cuda.empty_cache()
    return {"d2d_copy_TBps": round(2 * 4 * n / tc / 1e12, 2), "triad_TBps": round(3 * 4 * n / tt / 1e12, 2), "vendor_peak_TBps": HBM_PEAK_GBPS / 1e3,
            "how": "torch copy_ / add(out=) over 1 GiB float32 operands, read + write bytes"}


def host_info():
    """CPU model / thread count of the box the CPU baselines run on, and whether the real reference could be timed
    here (it needs cargo plus an offline registry holding the ark-* 0.3 crates)."""
    model = None
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    cargo = shutil.which("cargo")
    reg = os.path.isdir(os.path.expanduser("~/.cargo/registry"))
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count()
    return {"cpu_model": model, "hardware_concurrency": os.cpu_count(), "cpus_in_affinity_mask": usable,
            "cargo": {"cargo_on_path": cargo, "cargo_registry_present": reg,
                      "reference_timed": False,
                      "note": "no Rust toolchain / offline ark-* registry on this box: the CPU baseline is the C restatement of "
                              "the arkworks 0.3 algorithms (oracle/), not `cargo bench -p manta-benchmark`" if not (cargo and reg)
                      else "cargo and a registry exist: `cargo bench -p manta-benchmark --bench private_transfer` could be run by hand"}}


def launch_plan(gpus, environ, argv):
    """How `python bench.py --gpus N` gets its N ranks. -> None when this process IS a rank (N = 1, or a
    launcher already set WORLD_SIZE: the driver's `python -m torch.distributed.run ... bench.py --gpus N`), else the command that
    re-executes this file as N ranks on this node, one per GPU, rendezvous on 127.0.0.1 (the container hostname may not resolve)
    with a free port of our own. Pure function of its arguments: tests/test_host.py checks the decision without a GPU."""
    if gpus <= 1 or "WORLD_SIZE" in environ:
        return None
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % gpus, "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def self_launch(cmd):
    """run the N-rank job; its rank 0 prints the one compact line on our stdout (inherited). -> exit code"""
    import subprocess
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MANTA_BENCH_LAUNCHER="self", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.setdefault("OMP_NUM_THREADS", "4")  # torchrun would set 1 with a warning; the host side of a rank is a few threads
    sys.stdout.flush()
    return subprocess.call(cmd, env=env, cwd=ROOT)


def parity_gate(env):
    """N > 1, BEFORE anything is timed: one PrivateTransfer-shape proof (BN254, same key / assignment / r, s on
    every rank) through (a) this rank's own single-device context and (b) the range-sharded prover with the exchange the timed
    legs use; the bytes of (b) must be identical on every rank, equal to (a), and verify. A failure ends the run before a number
    exists."""
    from manta_rs_amd import api, synth, keygen, distributed
    curve = synth.BN254
    p = synth.FR_MODULUS[curve]
    c = synth.make_shape(curve, "private_transfer", profile="W")
    rng = synth.XorShift(0x4D414E5441_0006)
    pk = keygen.generate(c, [rng.field(p) for _ in range(5)])
    rs = synth.to_mont([rng.field(p) for _ in range(2)], p, 4).reshape(2, 4)
    r1cs = api.R1CS.from_circuit(c)
    z = api.PinnedArray.like(c.z)
    t0 = time.perf_counter()
    ctx = api.ProvingContext(curve, pk, full_table_bytes=0)
    it = iter(rs)
    single = api.Groth16.prove(ctx, r1cs, lambda: next(it))
    ctx.close()
    sp = distributed.ShardedProver(curve, pk, max_batch=1)
    sp.set_r1cs(r1cs)
    sharded = sp.prove(z.array, rs[0], rs[1])
    on_gpu = bool(sp.exchange.on_gpu)
    sp.close()
    mine = (bytes(single).hex(), bytes(sharded).hex())
    alls = [None] * env.world
    env.dist.all_gather_object(alls, mine)
    if any(a != alls[0] for a in alls) or mine[0] != mine[1]:
        raise SystemExit("bench.py parity gate: sharded proof bytes differ (rank %d: single %s... sharded %s...; ranks agree: %s)"
                         % (env.rank, mine[0][:16], mine[1][:16], all(a == alls[0] for a in alls)))
    vctx = api.VerifyingContext(curve, pk)
    ok = api.groth16_verify(vctx, c.z[1:c.P], api.proof_decode(curve, sharded))
    vctx.close()
    if not ok:
        raise SystemExit("bench.py parity gate: the sharded proof does not verify")
    return {"sharded_proof_equals_single_device_on_all_ranks": True, "verified": True, "exchange_on_gpu": on_gpu,
            "seconds": round(time.perf_counter() - t0, 2)}


class Env:
    """Process-per-GPU plumbing: device, process group, barrier, max-over-ranks."""

    def __init__(self, args):
        import torch
        import torch.distributed as dist
        from manta_rs_amd import api
        self.torch, self.dist, self.api = torch, dist, api
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        if self.world != args.gpus:  # main() re-executes itself as N ranks when WORLD_SIZE is unset; a launcher that disagrees is an error
            raise SystemExit("bench.py: launched with WORLD_SIZE=%d but --gpus %d" % (self.world, args.gpus))
        # MANTA_BENCH_DEVICE pins every rank to one device (functional test of the multi-process path on a 1-GPU box); RCCL
        # refuses one device twice in a clique, so that layout exchanges over gloo unless MANTA_BENCH_BACKEND says otherwise
        pinned = os.environ.get("MANTA_BENCH_DEVICE")
        self.dev = int(pinned) if pinned is not None else self.local_rank
        self.backend = os.environ.get("MANTA_BENCH_BACKEND", "gloo" if pinned is not None and self.world > 1 else "nccl")
        ndev = torch.cuda.device_count()
        if self.dev >= ndev:
            raise SystemExit("bench.py: rank %d wants device %d but this node shows %d GPU(s) -- --gpus N needs N visible devices "
                             "(or MANTA_BENCH_DEVICE=<id> to stack the ranks on one device over gloo)" % (self.rank, self.dev, ndev))
        torch.cuda.set_device(self.dev)
        api.init(self.dev)
        self.collective = {"backend": "none", "ranks": 1, "devices": [self.device_id()]}
        if self.world > 1:
            if self.backend == "nccl":
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=torch.device("cuda", self.dev))
            else:
                dist.init_process_group(self.backend, rank=self.rank, world_size=self.world)
            ids = [None] * self.world
            dist.all_gather_object(ids, self.device_id())
            # what the collective actually saw: the backend torch reports, the group's size, every DISTINCT physical device
            self.collective = {"backend": dist.get_backend(), "ranks": dist.get_world_size(), "devices": sorted(set(ids)),
                               "launcher": os.environ.get("MANTA_BENCH_LAUNCHER", "external")}

    def device_id(self):
        """a name for the PHYSICAL device this rank computes on: index + PCI bus id (two ranks stacked on one GPU report one id)"""
        pr = self.torch.cuda.get_device_properties(self.dev)
        bus = getattr(pr, "pci_bus_id", None)
        dom, devn = getattr(pr, "pci_domain_id", None), getattr(pr, "pci_device_id", None)
        if bus is None:
            return "cuda:%d" % self.dev
        return "cuda:%d@%04x:%02x:%02x" % (self.dev, dom or 0, bus, devn or 0)

    def barrier(self):
        self.api.synchronize()
        self.torch.cuda.synchronize()
        if self.world > 1:
            self.dist.barrier()
            self.torch.cuda.synchronize()

    def max_over_ranks(self, x):
        if self.world == 1:
            return x
        t = self.torch.tensor([x], dtype=self.torch.float64, device="cuda" if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def sum_ints_mod(self, v, p):
        if self.world == 1:
            return v % p
        parts = [None] * self.world
        self.dist.all_gather_object(parts, v)
        return sum(parts) % p

    def close(self):
        if self.world > 1:
            self.dist.destroy_process_group()


class MsmInstance:
    """One range shard of an n_total-term BLS12-381 G1 MSM: bases P_i = [S0 + i S1]G for i in this rank's range (built
    on the GPU by the library's fixed-base multiply), uniform scalars, both resident in HBM. The closed form
    sum_i k_i (S0 + i S1) mod r gives the expected global point from one scalar multiplication."""

    def __init__(self, env, n_total, window_bits, seed, curve=CURVE):
        from manta_rs_amd import api, synth, distributed
        self.env, self.api = env, api
        CURVE = self.curve = curve  # noqa: N806 (shadows the module default on purpose)
        p, q = synth.FR_MODULUS[CURVE], synth.FQ_MODULUS[CURVE]
        self.p = p
        self.G = synth.to_mont(list(BLS_G1 if curve == 1 else (1, 2)), q, synth.FQ_LIMBS[curve]).reshape(-1)
        self.launch_kw = {}
        self.acc_mhz = []
        lo, hi = distributed.shard_range(n_total, env.rank, env.world)
        self.n = hi - lo
        self.ks = [(S0 + i * S1) % p for i in range(lo, hi)]
        d_ks = api.DeviceBuffer.from_numpy(synth.ints_to_limbs(self.ks, 4))
        self.d_pts = api.fixed_base_mul(CURVE, 1, self.G, d_ks, self.n)
        self.bases = api.Bases(CURVE, 1, (self.d_pts.ptr, self.n), precompute_window_bits=window_bits, on_device=True)
        self.scalars = synth.msm_scalars(CURVE, self.n, "U", seed=seed + env.rank)  # uniform: the h-query MSM's case
        self.d_sc = api.DeviceBuffer.from_numpy(self.scalars)
        self.msm = distributed.ShardedMSM(self.bases)
        self.synth = synth
        api.synchronize()

    def expected(self):
        part = sum(k * b for k, b in zip(self.synth.limbs_to_ints(self.scalars), self.ks))
        t = self.env.sum_ints_mod(part, self.p)
        d_one = self.api.DeviceBuffer.from_numpy(self.synth.ints_to_limbs([t], 4))
        return self.api.fixed_base_mul(self.curve, 1, self.G, d_one, 1).to_numpy()

    def run(self, steps, depth, acc_ms=None):
        """`depth` MSMs in flight (each on its own HIP stream + workspace): the serial tail of step i (bucket reduce,
        host fold, partial-point exchange) overlaps the accumulate kernel of step i+1. depth = 1: latency mode."""
        res, pending = None, []

        def finish_one():
            out = pending.pop(0).finish()  # local fold + all_gather of the partial points + N-term sum
            if acc_ms is not None:
                acc_ms.append(self.api.last_accumulate_ms())  # HIP events around the accumulate kernel, on its stream
                self.acc_mhz.append(self.api.last_accumulate_mhz())  # shader clock of the same launch (s_memtime / wall clock)
            return out
        for _ in range(steps):
            pending.append(self.msm.launch(self.d_sc, self.n, **self.launch_kw))
            if len(pending) == depth:
                res = finish_one()
        while pending:
            res = finish_one()
        return res

    def timed(self, steps, depth, warmup=2, kernel_timing=False):
        """-> (seconds for `steps` steps: max over ranks, list of accumulate-kernel durations in ms); the point of the last step
        is kept in `self.last`"""
        env = self.env
        self.run(warmup, depth)
        acc = []
        if kernel_timing:
            self.api.set_kernel_timing(True)
        env.barrier()
        t0 = time.perf_counter()
        self.last = self.run(steps, depth, acc if kernel_timing else None)
        env.barrier()
        dt = time.perf_counter() - t0
        if kernel_timing:
            self.api.set_kernel_timing(False)
        return env.max_over_ranks(dt), acc


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """--dump-outputs DIR: what the timed path handed its caller in its last step, as DIR/<name>.npy, so that two builds can be
    compared output for output (the inputs are seeded: the same arguments give the same inputs). Limbs and proof bytes are
    unsigned integers; they are written as float64, exactly (64-bit limbs split into their 32-bit halves, little-endian first)."""
    out = {}
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.uint32)
        assert a.dtype in (np.uint8, np.uint32), (name, a.dtype)
        out[name] = a.astype(np.float64)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_CAP_BYTES:
        raise SystemExit("bench.py --dump-outputs: %d bytes, more than the %d allowed" % (total, DUMP_CAP_BYTES))
    os.makedirs(d, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(d, name + ".npy"), a)


def msm_bench(args, env):
    """The headline (pipelined 2^20 MSM) and, with --full, every other MSM leg. -> (line, instance)"""
    n = 1 << LOG_N
    inst = MsmInstance(env, env.world * n, WINDOW_BITS, seed=0x4D414E54)
    result = None
    if args.full:
        # ---- correctness gate before any timing counts
        result = inst.run(1, 1)
        assert (result == inst.expected()).all(), "MSM result does not match the closed-form expectation"

    dt, acc_pipe = inst.timed(args.steps, DEPTH, warmup=args.warmup, kernel_timing=True)
    if args.dump_outputs and env.rank == 0:
        dump_outputs(args.dump_outputs, {"msm_result": inst.last})
    mhz_pipe = [v for v in inst.acc_mhz if v > 0]
    line = {
        "metric": "G1 MSM Mscalar/s at 2^%d" % LOG_N, "value": round(env.world * n * args.steps / dt / 1e6, 3),
        "unit": "Mscalar/s", "n_gpus": env.world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u32", "data": "synthetic",
        "config": {"workload": "2^%d BLS12-381 G1 variable-base MSM per GPU, uniform scalars resident in HBM" % LOG_N,
                   "curve": "BLS12-381", "log_n": LOG_N, "window_bits": WINDOW_BITS, "msms_in_flight": DEPTH},
    }
    if env.world > 1:
        line["config"]["sharding"] = ("contiguous base/scalar ranges; partial points folded on the GPU, all_gather from device memory (RCCL), "
                                      "N-term host sum" if inst.msm.device_path else
                                      "contiguous base/scalar ranges, all_gather of partial points from host memory + N-term host sum")
    else:
        line["config"]["sharding"] = "none"
    if not args.full:
        return line, inst
    # ---- latency mode (one MSM at a time: nothing hides the merge / reduce / host-fold tail) doubles as the
    # stand-alone measurement of the dominant kernel: with one MSM in flight the HIP-event span IS the kernel's duration
    lat_steps = max(5, min(args.steps, 10))
    inst.acc_mhz = []
    dt_lat, acc_alone = inst.timed(lat_steps, 1, warmup=2, kernel_timing=True)
    mhz_alone = [v for v in inst.acc_mhz if v > 0]
    # ---- plain bases: what `VariableBaseMSM::multi_scalar_mul(bases, scalars)` literally takes (no precomputed tables)
    plain = None
    if env.world == 1 and not args.quick:
        from manta_rs_amd import api, distributed
        pb = api.Bases(CURVE, 1, (inst.d_pts.ptr, inst.n), precompute_window_bits=0, on_device=True)
        keep = inst.bases, inst.msm
        inst.bases, inst.msm = pb, distributed.ShardedMSM(pb)
        assert (inst.run(1, 1) == result).all()
        # three repetitions of each leg, alternating (a single sample of these legs once read 195 three in flight
        # against 244 one at a time; the median of three has never put the pipelined rate below the other)
        p1, p3 = [], []
        for _ in range(3):
            p1.append(n * lat_steps / inst.timed(lat_steps, 1)[0] / 1e6)
            p3.append(n * lat_steps / inst.timed(lat_steps, DEPTH)[0] / 1e6)
        plain = {"latency_mode_Mscalar_s": round(float(np.median(p1)), 2), "pipelined_Mscalar_s": round(float(np.median(p3)), 2),
                 "repetitions": 3, "latency_mode_min_max": [round(min(p1), 2), round(max(p1), 2)],
                 "pipelined_min_max": [round(min(p3), 2), round(max(p3), 2)],
                 "bases_hbm_bytes": pb.device_bytes()}
        inst.bases, inst.msm = keep
        pb.close()
    # ---- SURVEY.md 8(d) config 2, the rest of it: witness-like scalars (40 % zeros, 25 % ones, 10 % < 2^64, 25 % uniform)
    # on the same bases through the zero-digit compaction path, and the BN254 instantiation at the same size
    other = None
    if env.world == 1 and not args.quick:
        from manta_rs_amd import api, synth
        keep = inst.scalars, inst.d_sc
        inst.scalars = synth.msm_scalars(CURVE, n, "W", seed=0x4D414E57)
        inst.d_sc, inst.launch_kw = api.DeviceBuffer.from_numpy(inst.scalars), {"sparse": True}
        assert (inst.run(1, 1) == inst.expected()).all(), "witness-like MSM does not match the closed form"
        dt_w1, _ = inst.timed(lat_steps, 1)
        dt_w3, _ = inst.timed(lat_steps, DEPTH)
        (inst.scalars, inst.d_sc), inst.launch_kw = keep, {}
        bn = MsmInstance(env, n, WINDOW_BITS, seed=0x4D414E42, curve=0)
        assert (bn.run(1, 1) == bn.expected()).all(), "BN254 MSM does not match the closed form"
        dt_b1, _ = bn.timed(lat_steps, 1)
        dt_b3, _ = bn.timed(lat_steps, DEPTH)
        other = {"witness_like_scalars": {"latency_mode_Mscalar_s": round(n * lat_steps / dt_w1 / 1e6, 2),
                                          "pipelined_Mscalar_s": round(n * lat_steps / dt_w3 / 1e6, 2)},
                 "bn254_g1_uniform": {"latency_mode_Mscalar_s": round(n * lat_steps / dt_b1 / 1e6, 2),
                                      "pipelined_Mscalar_s": round(n * lat_steps / dt_b3 / 1e6, 2), "algorithmic_bytes_per_scalar": 96}}
        bn.bases.close()
        del bn
    line["config"].update({
        "precomputed_base_multiples": True, "bases_hbm_bytes": inst.bases.device_bytes(),
        "windows": -(-255 // WINDOW_BITS),
        "note": "headline = pipelined (%d MSMs in flight) against bases with precomputed 2^(%dw) multiples (a full 2^20 "
                "BLS12-381 key needs 5 such tables, ~10 GB of the 288 GB)" % (DEPTH, WINDOW_BITS),
        "latency_mode": {"Mscalar_s": round(env.world * n * lat_steps / dt_lat / 1e6, 2), "ms_per_msm": round(dt_lat / lat_steps * 1e3, 4)},
        "plain_bases": plain,
        "other_inputs_same_size": other})

    roofline = cpu = None
    if env.rank == 0:
        k_alone = float(np.mean(acc_alone))
        k_pipe = float(np.mean(acc_pipe))
        algo = n * ALGO_BYTES_PER_SCALAR
        achieved = algo / (k_alone * 1e-3) / 1e9
        traffic = None
        pmc = os.path.join(ROOT, "profiles", "pmc_accumulate.json")
        if os.path.exists(pmc):
            try:
                traffic = json.load(open(pmc)).get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        mads = clock = None
        try:  # the issue peak of the multiplier and the clock under that load, measured now on this box (mg_clock_probe)
            mhz, mad_per_us, probe_ms = inst.api.clock_probe(150000)
            clock = {"probe_MHz": round(mhz, 1), "probe_wave_mads_per_simd_per_us": round(mad_per_us, 2), "probe_ms": round(probe_ms, 2),
                     "accumulate_kernel_MHz_latency_mode": round(float(np.mean(mhz_alone)), 1) if mhz_alone else None,
                     "accumulate_kernel_MHz_pipelined": round(float(np.mean(mhz_pipe)), 1) if mhz_pipe else None,
                     "how": "shader clock = s_memtime ticks per wall-clock second (s_memrealtime, constant rate). probe: mg_clock_probe, two "
                            "wavefronts per SIMD on every CU spinning on 8 independent v_mad_u64_u32 chains each; accumulate kernel: its first "
                            "wavefront brackets its own run (the launches of the timed loops above)"}
            peak_meas = mad_per_us * 1e6 * 1024 * 64 / 1e12
        except Exception as e:  # noqa: BLE001
            clock, peak_meas = {"error": str(e)}, None
        if LOG_N == 20 and WINDOW_BITS >= 15:
            # modelled low: 0.941 mixed additions per (scalar, window) -- the PMC count of wave-additions per scalar-lane is 1.0 per window
            windows = -(-255 // WINDOW_BITS)
            adds = 15.06 / 16 * windows
            m = n * adds * MADS_PER_MIXED_ADD
            ach = m / (k_alone * 1e-3) / 1e12
            mads = {"mads_per_launch_modelled": int(m), "model": "%.2f mixed additions per scalar (%d windows) x %d multiply-adds each (PMC: %d.0 wave-additions per scalar-lane)" % (adds, windows, MADS_PER_MIXED_ADD, windows),
                    "achieved_Tmad_s": round(ach, 2),
                    "note_round_4": "13 x 30-bit limbs: %d multiply-adds per mixed addition instead of the %d of rounds 2-3 (-13.5 %%) for -2.6 %% of "
                                    "kernel time on one box (profiles/r04_limbs_13x30_ab.txt): the columns that overflow are flushed, and the carry-free "
                                    "differences the 14 x 28 layout had room for are normalised again, so the multiply-add share of the instruction "
                                    "stream fell; at the old count the same launch would read %.2f Tmad/s" % (MADS_PER_MIXED_ADD, MADS_PER_MIXED_ADD_R3, n * adds * MADS_PER_MIXED_ADD_R3 / (k_alone * 1e-3) / 1e12),
                    "peak_Tmad_s": round(peak_meas, 2) if peak_meas else None, "frac": round(ach / peak_meas, 3) if peak_meas else None,
                    "peak_how": "issue rate measured in this run by mg_clock_probe (no clock assumed) x 1024 SIMDs x 64 lanes",
                    "peak_Tmad_s_assuming_2.4GHz": round(PEAK_TMAD_S_ASSUMED, 2), "frac_assuming_2.4GHz": round(ach / PEAK_TMAD_S_ASSUMED, 3)}
            if peak_meas and mhz_alone:
                # the probe's issue rate scaled to the clock the accumulate kernel itself ran at (same launches as kernel_ms)
                pk = peak_meas * float(np.mean(mhz_alone)) / mhz
                mads["peak_Tmad_s_at_the_kernels_own_clock"] = round(pk, 2)
                mads["frac_at_the_kernels_own_clock"] = round(ach / pk, 3)
        traffic_source = ("profiles/pmc_accumulate.json: FETCH_SIZE + WRITE_SIZE of this kernel from separate rocprofv3 --pmc passes of an earlier "
                          "run of this build (not re-measured by this run)")
        live = None
        if env.world == 1 and not args.quick and not os.environ.get("MANTA_BENCH_NO_PMC") and LOG_N == 20:
            try:
                live = pmc_traffic()
            except Exception as e:  # noqa: BLE001
                live = {"error": str(e)}
            if live and "hbm_bytes_per_launch" in live:
                traffic = live["hbm_bytes_per_launch"]
                traffic_source = ("measured by this run: two child runs under rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate "
                                  "passes), raw counters, average over %d launches of this kernel" % live["launches_averaged"])
        roofline = {"bound": "hbm", "kernel": "accumulate_chunks<FpR<Bls381Fq>>", "achieved": round(achieved, 2),
                    "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 5), "traffic": traffic,
                    "traffic_source": traffic_source, "traffic_pmc": live,
                    "clock": clock,
                    "kernel_ms": round(k_alone, 4),
                    "kernel_ms_how": "HIP events on the kernel's own stream, averaged over the %d latency-mode steps of this run "
                                     "(one MSM in flight, so the span is the launch duration; rocprofv3 --kernel-trace of "
                                     "MANTA_BENCH_DEPTH=1 runs agrees: profiles/)" % lat_steps,
                    "kernel_ms_pipelined_span": round(k_pipe, 4),
                    "kernel_ms_pipelined_note": "same events inside the timed region: with %d MSMs in flight the span also holds "
                                                "time queued behind / shared with the neighbours' kernels, so it exceeds ms_per_step" % DEPTH,
                    "algorithmic_bytes_per_launch": algo,
                    "note": "integer-multiply bound, not HBM bound (SURVEY.md F7); int_mad gives the bound that governs",
                    "int_mad": mads}
    if env.rank == 0 and env.world == 1 and not args.quick:
        try:
            line["hbm_reference"] = hbm_reference()
        except Exception as e:  # noqa: BLE001
            line["hbm_reference"] = {"error": str(e)}
    line["roofline"], line["cpu_baseline"] = roofline, cpu
    # the CPU baseline runs LAST (main): OpenMP worker threads of the oracle must not share the host with the timed GPU legs
    line["_cpu_todo"] = (inst, result, n) if (env.rank == 0 and not args.no_cpu_baseline and env.world == 1) else None
    return line, inst


def msm_cpu_baseline(inst, result, n):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O  # the checker, here only as the timed CPU baseline
    host_pts = inst.d_pts.to_numpy(shape=(n, 12))
    O.set_threads(1)
    t1, out = O.time_msm(CURVE, 1, host_pts, inst.scalars)  # one whole 2^20 MSM: ~12 s on one thread
    assert (np.asarray(out).reshape(-1) == np.asarray(result).reshape(-1)).all(), "CPU and GPU MSM results differ"
    cores = O.set_threads(O.usable_cpus())
    ta, out = O.time_msm(CURVE, 1, host_pts, inst.scalars)
    O.set_threads(1)
    assert (np.asarray(out).reshape(-1) == np.asarray(result).reshape(-1)).all()
    return {"value": round(n / t1 / 1e6, 5), "unit": "Mscalar/s", "cores": 1, "kind": "port",
            "sample": f"the same {n} bases/scalars as the GPU workload, arkworks-0.3 Pippenger restatement (window rule, "
                      f"bucket method, Horner), {t1:.1f} s on 1 thread (the reference ships arkworks without `parallel`); "
                      "result point equals the GPU's",
            "all_cores": {"value": round(n / ta / 1e6, 5), "cores": cores, "seconds": round(ta, 2),
                          "how": "one task per Pippenger window, the decomposition of arkworks' `parallel` feature (17 windows at "
                                 "2^20: at most 17-way)"},
            **host_info()}


def strong_scaling(args, env):
    """1/2/4/8-GPU times for a FIXED n = 2^20 and a fixed n = 35 174 (the PrivateTransfer witness MSM),
    split into N contiguous ranges -- expected near-linear at 2^20, flat or worse at 35 k (launch-latency-bound)."""
    out = {}
    for name, n_total, c in (("n_2^20", 1 << 20, WINDOW_BITS), ("n_35174", 35174, 8)):
        inst = MsmInstance(env, n_total, c, seed=0x5354524F)
        got = inst.run(1, 1)
        assert (got == inst.expected()).all(), "strong-scaling MSM does not match the closed form"
        steps = max(5, min(args.steps, 20))
        dt1, _ = inst.timed(steps, 1)
        dt3, _ = inst.timed(steps, DEPTH)
        out[name] = {"n_total": n_total, "n_per_gpu": inst.n, "window_bits": c,
                     "ms_per_msm_latency_mode": round(dt1 / steps * 1e3, 4), "ms_per_msm_pipelined": round(dt3 / steps * 1e3, 4),
                     "Mscalar_s_pipelined": round(n_total * steps / dt3 / 1e6, 3)}
        inst.bases.close()
    return out


def ntt_bench(env, log_n=20):
    """SURVEY.md 8(d) "NTT micro": 2^20 uniform BLS12-381 Fr elements resident in HBM, forward / inverse / coset transforms in
    place through mg_ntt_device (natural order in and out, arkworks format in and out). Algorithmic bytes = one read + one
    write of the vector = 64 B per element. Parity gate: inverse(forward(x)) == x before timing."""
    from manta_rs_amd import api, synth
    curve, D = 1, 1 << log_n
    p = synth.FR_MODULUS[curve]
    rng = np.random.RandomState(0x4E5454)
    x = rng.randint(0, 1 << 62, size=(D, 4), dtype=np.int64).astype(np.uint64)
    x[:, 3] &= np.uint64((1 << 60) - 1)  # < p: valid Montgomery residues
    d = api.DeviceBuffer.from_numpy(x)
    dom = api.Radix2EvaluationDomain(curve, D)
    dom.fft_device(d, False, False)
    dom.fft_device(d, True, False)
    assert (d.to_numpy(shape=(D, 4)) == x).all(), "ifft(fft(x)) != x"
    dom.fft_device(d, False, True)
    dom.fft_device(d, True, True)
    assert (d.to_numpy(shape=(D, 4)) == x).all(), "coset_ifft(coset_fft(x)) != x"
    out = {"curve": "BLS12-381", "log_n": log_n, "algorithmic_bytes": 64 * D, "data": "uniform Fr, resident in HBM, transformed in place"}
    api.set_kernel_timing(True)
    for name, inv, cos in (("fft", 0, 0), ("ifft", 1, 0), ("coset_fft", 0, 1), ("coset_ifft", 1, 1)):
        reps, dev, parts = 12, [], []
        for _ in range(2):
            dom.fft_device(d, inv, cos)
        t0 = time.perf_counter()
        for _ in range(reps):
            dom.fft_device(d, inv, cos)
            v = api.last_ntt_ms()
            dev.append(v[0])
            parts.append(v[1:])
        wall = (time.perf_counter() - t0) / reps
        ms = float(np.median(dev))
        pm = np.median(np.array(parts), axis=0)
        npass = -(-log_n // 10)
        out[name] = {"device_ms": round(ms, 4), "Melem_per_s": round(D / ms / 1e3, 1), "algorithmic_GBps": round(64 * D / ms / 1e6, 1),
                     "frac_of_hbm_peak": round(64 * D / ms / 1e6 / HBM_PEAK_GBPS, 4), "call_wall_ms": round(wall * 1e3, 4),
                     "conversion_in_us": round(float(pm[0]) * 1e3, 1), "butterfly_passes": npass,
                     "us_per_pass": round(float(pm[1]) * 1e3 / npass, 1), "conversion_out_us": round(float(pm[2]) * 1e3, 1)}
    api.set_kernel_timing(False)
    d.free()
    return out


def config2_bench(env, log_d=20):
    """BASELINE configs[2]: "2^20 Fr radix-2 NTT + 2^20 G1/G2 MSM -> single Groth16 proof, 1 MI355X" (SURVEY.md 8(d) config 3):
    BLS12-381, D = V = 2^20, P = 16, synthetic chain circuit, valid key generated on the GPU. Parity gate here: the proof
    verifies on the GPU (mg_groth16_verify, BLS12-381 pairing) and is reproduced bit for bit by a second run; the byte
    comparison with the CPU oracle at this size is tests/test_gpu_configs.py::test_config2_* (it takes minutes of CPU)."""
    from manta_rs_amd import api, synth, keygen
    curve, D, P = 1, 1 << log_d, 16
    p = synth.FR_MODULUS[curve]
    t0 = time.perf_counter()
    c = synth.make_circuit(curve, D - P, D, P, seed=0x4D414E5441_0301, profile="W")  # the witness-like 40 / 25 / 10 / 25 split
    rng = synth.XorShift(0x4D414E5441_0302)
    pk = keygen.generate(c, [rng.field(p) for _ in range(5)])
    ctx = api.ProvingContext(curve, pk)
    ctx.set_r1cs(api.R1CS.from_circuit(c))
    setup_s = time.perf_counter() - t0
    rs = synth.to_mont([rng.field(p), rng.field(p)], p, 4)
    z = api.PinnedArray.like(c.z)
    first = api.Groth16.prove_with_randomness(ctx, z.array, rs[0], rs[1])
    vctx = api.VerifyingContext(curve, pk)
    assert api.groth16_verify(vctx, c.z[1:c.P], api.proof_decode(curve, first)), "2^20 BLS12-381 proof does not verify"
    vctx.close()
    ts = []
    for _ in range(6):
        t = time.perf_counter()
        pr = api.Groth16.prove_with_randomness(ctx, z.array, rs[0], rs[1])
        ts.append(time.perf_counter() - t)
        assert pr == first
    api.set_kernel_timing(True)  # eager launches with events between the phases
    phases = None
    for _ in range(3):
        assert api.Groth16.prove_with_randomness(ctx, z.array, rs[0], rs[1]) == first
        phases = api.last_prove_phases_ms()
    api.set_kernel_timing(False)
    ctx.close()
    z.free()
    hist = synth.histogram(c.z_int)
    return {"_cpu_todo": (c, pk, rs, first),
            "workload": "one Groth16 proof, BLS12-381, D = V = 2^%d, P = 16: 3 SpMV + 7 NTT of 2^%d + 4 G1 MSM + 1 G2 MSM of ~2^%d terms" % (log_d, log_d, log_d),
            "witness_profile": "W", "z_histogram": {k: (round(v, 4) if k != "n" else v) for k, v in hist.items()},
            "prove_ms": round(min(ts) * 1e3, 3), "prove_ms_median": round(float(np.median(ts)) * 1e3, 3), "proofs_per_s": round(1 / min(ts), 2),
            "phases_ms": phases,
            "phases_note": "HIP events between the phases of one proof enqueued with plain launches (the timed runs above replay captured "
                           "graphs); the five MSMs run concurrently on their own streams, so the phases overlap and do not add up to prove_ms",
            "parity": "verified on the GPU (BLS12-381 pairing), identical bytes on every run; oracle byte comparison in tests/test_gpu_configs.py",
            "setup_s": round(setup_s, 1)}


def sharded_proof_bench(args, env):
    """BASELINE configs[3]: "PrivateTransfer full proof, MSM sharded across the GPUs via RCCL/xGMI" -- one process per GPU,
    every rank holds slice rank/N of the five queries (mg_ctx_create_shard), proves its five partial MSMs, ONE fused all_gather
    of the five partial points per proof (device memory -> RCCL, no host sync before the collective), every rank assembles.
    Proof bytes are checked against each other across ranks and verified on the GPU before timing."""
    from manta_rs_amd import api, synth, keygen, distributed
    curve = synth.BN254
    p = synth.FR_MODULUS[curve]
    c = synth.make_shape(curve, "private_transfer", profile="W")
    rng = synth.XorShift(0x4D414E5441_0002)
    pk = keygen.generate(c, [rng.field(p) for _ in range(5)])  # the same key on every rank (same seed)
    K = 32
    sp = distributed.ShardedProver(curve, pk, max_batch=K)
    sp.set_r1cs(api.R1CS.from_circuit(c))
    nrs = 64
    rs = synth.to_mont([rng.field(p) for _ in range(2 * nrs)], p, 4).reshape(nrs, 2, 4)
    z1 = api.PinnedArray.like(c.z)
    zK = api.PinnedArray.like(np.stack([c.z] * K))
    first = sp.prove(z1.array, rs[0][0], rs[0][1])
    theirs = [None] * env.world
    env.dist.all_gather_object(theirs, first)
    assert all(t == first for t in theirs), "ranks assembled different proofs"
    vctx = api.VerifyingContext(curve, pk)
    assert api.groth16_verify(vctx, c.z[1:c.P], api.proof_decode(curve, first)), "sharded proof does not verify"
    vctx.close()

    def run_single(n):
        for i in range(n):
            sp.prove(z1.array, rs[i % nrs][0], rs[i % nrs][1])

    def run_batched(n_passes, depth=3):
        pending = []
        for i in range(n_passes):
            sel = [(i * K + q) % nrs for q in range(K)]
            pending.append(sp.launch(zK.array, rs[sel, 0], rs[sel, 1]))
            if len(pending) == depth:
                pending.pop(0).finish()
        while pending:
            pending.pop(0).finish()
    run_single(8)
    env.barrier()
    t0 = time.perf_counter()
    n1 = 40
    run_single(n1)
    env.barrier()
    dt1 = env.max_over_ranks(time.perf_counter() - t0)
    run_batched(4)
    env.barrier()
    t0 = time.perf_counter()
    nb = 12
    run_batched(nb)
    env.barrier()
    dtb = env.max_over_ranks(time.perf_counter() - t0)
    out = {"workload": "PrivateTransfer-shape proof, every MSM range-sharded over %d ranks (one process per GPU)" % env.world,
           "exchange": ("one fused RCCL all_gather of 5 partial points per proof from device memory (%d B per rank and proof)"
                        % (5 * sp.slot * 8)) if sp.exchange.on_gpu else "gloo all_gather from host memory (functional run)",
           "sequential": {"ms_per_proof": round(dt1 / n1 * 1e3, 4), "proofs_per_s": round(n1 / dt1, 2)},
           "batched": {"proofs_per_pass": K, "passes_in_flight": 3, "proofs_per_s": round(nb * K / dtb, 2),
                       "ms_per_proof": round(dtb / (nb * K) * 1e3, 4)},
           "scaling": "strong (one proof's MSMs split N ways; the witness map is recomputed on every rank)"}
    sp.close()
    # the alternative placement of SURVEY.md 8(e): every MSM computed in full by one rank (at most five busy), same exchange
    tp = distributed.ShardedProver(curve, pk, max_batch=K, placement="task")
    tp.set_r1cs(api.R1CS.from_circuit(c))
    assert tp.prove(z1.array, rs[0][0], rs[0][1]) == first, "task-parallel proof differs from the range-sharded one"
    for i in range(8):
        tp.prove(z1.array, rs[i % nrs][0], rs[i % nrs][1])
    env.barrier()
    t0 = time.perf_counter()
    for i in range(n1):
        tp.prove(z1.array, rs[i % nrs][0], rs[i % nrs][1])
    env.barrier()
    dtt = env.max_over_ranks(time.perf_counter() - t0)
    out["task_parallel"] = {"placement": "MSM i computed in full by one rank: masks %s (bit 0 a, 1 b_g1, 2 b_g2, 3 l, 4 h)" % distributed.task_masks(env.world),
                            "sequential": {"ms_per_proof": round(dtt / n1 * 1e3, 4), "proofs_per_s": round(n1 / dtt, 2)}}
    tp.close()
    return out


# ---------------------------------------------------------------------------------------------------- proofs
_DISTINCT = {}  # shape -> (circuit, [K, V, 4] uint64 assignments); filled by main() BEFORE the process initialises HIP


def _assign_worker(seed):
    return _REASSIGNER.assign(seed).z


def precompute_assignments(shape, K, profile="W"):
    """K independent satisfying assignments of the shape's circuit (z_0 = the circuit's own, z_j from
    seed ...1000+j: fresh public inputs, fresh boolean witnesses, every gate output recomputed; the witness profile's density is
    kept, synth.Reassigner). ~0.1 s of Python each, so they are made by a fork pool -- before this process touches the GPU (a
    forked HIP context is not usable)."""
    global _REASSIGNER
    import multiprocessing as mp
    from manta_rs_amd import synth
    c = synth.make_shape(synth.BN254, shape, profile=profile)
    _REASSIGNER = synth.Reassigner(c)
    try:
        procs = max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        procs = 4
    seeds = [0x4D414E5441_1000 + j for j in range(1, K)]
    with mp.get_context("fork").Pool(procs) as pool:
        zs = pool.map(_assign_worker, seeds, chunksize=max(1, len(seeds) // (4 * procs)))
    _DISTINCT[shape] = (c, np.stack([c.z] + zs))


class ProveSetup:
    def __init__(self, shape, profile="W"):
        from manta_rs_amd import api, synth, keygen
        self.api, self.synth, self.shape, self.profile = api, synth, shape, profile
        curve = self.curve = synth.BN254
        p = self.p = synth.FR_MODULUS[curve]
        t0 = time.perf_counter()
        self.c, self.zs = _DISTINCT[shape] if shape in _DISTINCT else (synth.make_shape(curve, shape, profile=profile), None)
        assert self.c.profile == profile
        self.rng = synth.XorShift(0x4D414E5441_0002)
        toxic = [self.rng.field(p) for _ in range(5)]
        self.pk = keygen.generate(self.c, toxic)
        self.ctx = api.ProvingContext(curve, self.pk)
        self.ctx.set_r1cs(api.R1CS.from_circuit(self.c))
        self.setup_s = time.perf_counter() - t0
        self.nrs = 64
        self.rs = synth.to_mont([self.rng.field(p) for _ in range(2 * self.nrs)], p, 4).reshape(self.nrs, 2, 4)
        # the assignment lives in page-locked memory (mg_host_alloc), as a host integration would keep it: the library
        # then DMAs it from there instead of staging a copy first
        self.z1_pin = api.PinnedArray.like(self.c.z)
        self.zK = {}

    def release_gpu(self):
        """drop the proving context (device key, proof slots, their graphs) and the pinned assignments"""
        self.ctx.close()
        self.z1_pin.free()
        for v in self.zK.values():
            v.free()
        self.zK = {}
        self.api.synchronize()

    def zk(self, K):
        """K assignments back to back: distinct ones when they were prepared (K <= their number), else K copies"""
        if K not in self.zK:
            src = self.zs[:K] if self.zs is not None and len(self.zs) >= K else np.stack([self.c.z] * K)
            self.zK[K] = self.api.PinnedArray.like(src)
        return self.zK[K].array

    def distinct(self, K):
        return self.zs is not None and len(self.zs) >= K

    def run(self, steps, threads, K):
        """`steps` proofs, `threads` host threads sharing ONE ProvingContext (the reference's signer does the same,
        manta-pay/src/simulation/mod.rs:75-79), K proofs per call (K = 1: mg_groth16_prove)."""
        api, rs, nrs, ctx = self.api, self.rs, self.nrs, self.ctx
        z1 = self.z1_pin.array
        zK = self.zk(K) if K > 1 else None
        out = [None] * steps
        if K == 1:
            # single calls: the C entry point directly, pointers prepared once (a few microseconds of Python per call, the GIL
            # released inside the library) -- six signer threads must not be measured through a lock and numpy conversions
            import ctypes
            vp = ctypes.c_void_p
            zp = z1.ctypes.data_as(vp)
            rp = [(rs[j][0].ctypes.data_as(vp), rs[j][1].ctypes.data_as(vp)) for j in range(nrs)]
            nbytes, h, prove = api.PROOF_BYTES[ctx.curve], ctx.handle, api.LIB.mg_groth16_prove

            def worker(tid=0):
                for i in range(tid, steps, threads):
                    buf = ctypes.create_string_buffer(nbytes)
                    rc = prove(h, zp, rp[i % nrs][0], rp[i % nrs][1], buf)
                    if rc:
                        raise api.MantaGpuError(rc, "mg_groth16_prove")
                    out[i] = buf.raw
        else:
            idx = iter(range(0, steps, K))
            lock = threading.Lock()

            def worker(tid=0):
                while True:
                    with lock:
                        i = next(idx, None)
                    if i is None:
                        return
                    sel = [(i + q) % nrs for q in range(K)]  # one pass of the GPU pipeline for proofs i .. i+K-1
                    got = api.Groth16.prove_batch(ctx, zK, rs[sel, 0], rs[sel, 1])
                    for q in range(min(K, steps - i)):
                        out[i + q] = got[q]
        if threads == 1:
            worker()
        else:
            ts = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
            [t.start() for t in ts]
            [t.join() for t in ts]
        return out

    def timed(self, env, steps, threads, K, reps=1):
        """-> (seconds of the MEDIAN repetition of `steps` proofs, the proofs of the last one, [seconds of every repetition]).
        Thread legs vary by +-15 % from run to run (which calls a pass happens to coalesce), so they are repeated and the line
        carries median, min and max."""
        # slots capture their graphs on the 3rd call; coalesced single calls use one slot per pass size (2 .. threads)
        self.run(max(4 * K * threads, 8) if threads <= 2 else 60 * threads, threads, K)
        dts, proofs = [], None
        for _ in range(reps):
            env.barrier()
            t0 = time.perf_counter()
            proofs = self.run(steps, threads, K)
            env.barrier()
            dts.append(env.max_over_ranks(time.perf_counter() - t0))
        return float(np.median(dts)), proofs, dts


def _rate_stats(env, n, dts, extra=None):
    """proofs/s of the median repetition, with the spread"""
    rates = sorted(env.world * n / d for d in dts)
    out = {"proofs_per_s": round(float(np.median(rates)), 2), "repetitions": len(dts), "min": round(rates[0], 2), "max": round(rates[-1], 2)}
    if extra:
        out.update(extra)
    return out


BN254_MADS_G1_MIXED_ADD = 6 * 171 + 2 * 135 + 252   # 9 x 29-bit limbs: 2K^2+K per product, squarings K(K+1)/2+K^2+K, one fused a*b+c*d (3K^2+K)
BN254_MADS_G2_MIXED_ADD = (6 * 3 + 2 * 2) * 171 + 3 * 252  # over Fp2: 3 base products per product (Karatsuba), 2 per squaring, the fused one x 3


def proof_work_model(c, cw=None):
    """Mixed additions of ONE proof's five accumulate kernels on the wide bucket tables batched passes use (z queries c = cw
    signed windows, h query c = log2(D) - 2), counted on the assignment actually proved: non-zero signed digits of every
    scalar whose base is not the point at infinity (a variable absent from A / B has an infinity entry in the query and is
    dropped when the key is loaded). Merges and bucket reduces are left out: the figure is a LOWER bound on the work, the
    rate derived from it an UPPER bound."""
    from manta_rs_amd import synth
    r = synth.FR_MODULUS[c.curve]
    bits = synth.FR_BITS[c.curve]
    if cw is None:  # the library's rule (csrc/prover_key.h, round 6): 12-bit windows from 2^15 scalars on, else 11
        cw = 12 if c.V - 1 >= (1 << 15) else 11

    def nz_digits(v, cc):
        if v > r - v:
            v = r - v
        n, carry, half, mask = 0, 0, 1 << (cc - 1), (1 << cc) - 1
        for _ in range(-(-bits // cc)):
            d = (v & mask) + carry
            v >>= cc
            carry = 1 if d > half else 0
            n += 1 if (d != 0 and d != (1 << cc)) else 0
        return n
    V, P = c.V, c.P
    in_a = np.zeros(V, dtype=bool)
    in_a[np.asarray(c.A.col)] = True
    in_a[:P] = True  # input-consistency rows
    in_b = np.zeros(V, dtype=bool)
    in_b[np.asarray(c.B.col)] = True
    dig = [nz_digits(v, cw) if v else 0 for v in c.z_int]
    a = sum(dig[i] for i in range(1, V) if in_a[i])
    b = sum(dig[i] for i in range(1, V) if in_b[i])
    l = sum(dig[P:])
    ch = max(8, min(14, c.D.bit_length() - 1 - 2))
    h = int(c.D * (-(-bits // ch)) * (1 - 2.0 ** -ch))  # h is a dense vector of D coefficients
    g1, g2 = a + b + l + h, b
    return {"g1_mixed_additions": int(g1), "g2_mixed_additions": int(g2), "per_msm": {"a": int(a), "b_g1": int(b), "b_g2": int(b), "l": int(l), "h": h},
            "mads_per_proof": int(g1 * BN254_MADS_G1_MIXED_ADD + g2 * BN254_MADS_G2_MIXED_ADD),
            "model": "non-zero %d-bit signed digits of z over the non-infinity entries of a / b / l (h: %d-bit windows, dense) x %d multiply-adds per "
                     "G1 mixed addition, %d per G2 one; merges and bucket reduces not counted" % (cw, ch, BN254_MADS_G1_MIXED_ADD, BN254_MADS_G2_MIXED_ADD)}


def verify_bench(ps, proofs, zs=None):
    """mg_groth16_verify / mg_groth16_verify_batch on the proofs just produced (same circuit and inputs for all of them:
    the verifier's work does not depend on that). Proof decoding (decompression + subgroup checks, host) is outside the
    timed region, as a `Proof` arrives deserialised in the reference."""
    api = ps.api
    vctx = api.VerifyingContext(ps.curve, ps.pk)
    inputs = ps.c.z[1:ps.c.P]
    pts = [api.proof_decode(ps.curve, p) for p in proofs[:256]]
    assert api.groth16_verify(vctx, inputs, pts[0])
    if zs is not None:  # distinct assignments: every proof against ITS public inputs; one against a neighbour's must fail
        for i in (1, len(pts) // 2, len(pts) - 1):
            assert api.groth16_verify(vctx, zs[i][1:ps.c.P], pts[i]), "proof %d of the distinct batch does not verify" % i
        assert not api.groth16_verify(vctx, zs[2][1:ps.c.P], pts[1])
    bad = inputs.copy()
    bad[0] = ps.rs[0][0]
    assert not api.groth16_verify(vctx, bad, pts[0])
    n1 = 100
    for i in range(10):  # untimed: the device idled while the host decoded the proofs above, and a one-wavefront kernel runs at its clock
        api.groth16_verify(vctx, inputs, pts[i % len(pts)])
    t0 = time.perf_counter()
    for i in range(n1):
        api.groth16_verify(vctx, inputs, pts[i % len(pts)])
    t1 = (time.perf_counter() - t0) / n1
    k = len(pts)
    rnd = np.random.RandomState(7).randint(1, 1 << 62, size=(k, 2)).astype(np.uint64)
    allin = np.stack([inputs] * k) if zs is None else np.ascontiguousarray(zs[:k, 1:ps.c.P])
    assert api.groth16_verify_batch(vctx, allin, pts, rnd)
    t0 = time.perf_counter()
    nb = 3
    for _ in range(nb):
        api.groth16_verify_batch(vctx, allin, pts, rnd)
    tb = (time.perf_counter() - t0) / nb
    vctx.close()
    return {"single_ms": round(t1 * 1e3, 3), "single_proofs_per_s": round(1 / t1, 1), "batch": k, "batch_ms": round(tb * 1e3, 3),
            "batch_proofs_per_s": round(k / tb, 1),
            "how": "3 / k + 3 Miller loops (two wavefronts each: one makes the lines -- G2Prepared::from of the proof's B as it runs, or the stored table scaled by P -- the other multiplies them in, one Fq product per lane) + one wave-cooperative final exponentiation (cyclotomic squarings, width-4 NAF); 10 untimed + 100 timed single calls; accepted and a fuzzed input rejected before timing"}


def prove_cpu_baseline(ps, proofs, ncpu=8):
    ncpu = min(ncpu, len(proofs))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O  # checker, here as the timed CPU baseline (and a free byte-parity check)
    c, pk, rs, nrs = ps.c, ps.pk, ps.rs, ps.nrs
    O.set_threads(1)
    t1 = time.perf_counter()
    want = [O.groth16_prove(c, pk, rs[i % nrs][0], rs[i % nrs][1], msm_algo=1) for i in range(ncpu)]
    t1 = time.perf_counter() - t1
    for i in range(ncpu):
        assert want[i] == proofs[i], "GPU proof bytes differ from the CPU restatement"
    assert O.groth16_verify(ps.curve, pk, c.z[1:c.P], proofs[0]) == 1, "proof does not satisfy the pairing equation"
    cores = O.set_threads(O.usable_cpus())
    ta = time.perf_counter()
    again = [O.groth16_prove(c, pk, rs[i % nrs][0], rs[i % nrs][1], msm_algo=1) for i in range(ncpu)]
    ta = time.perf_counter() - ta
    O.set_threads(1)
    assert again == want
    return {"value": round(ncpu / t1, 4), "unit": "proofs/s", "cores": 1, "kind": "port",
            "sample": f"{ncpu} proofs of the same circuit/key/witness (the timed run's first {ncpu} (r, s) pairs), arkworks-0.3 "
                      f"algorithm restatement (7-FFT witness map, 5 Pippenger MSMs), {t1:.2f} s on 1 thread; bytes equal the GPU "
                      "proofs; proof pairing-verified",
            "all_cores": {"value": round(ncpu / ta, 4), "cores": cores, "seconds": round(ta, 2),
                          "how": "arkworks-`parallel` decomposition: one task per MSM window, chunk-parallel FFT stages and element loops"},
            **host_info()}


def prove_bench(args, env, shape="private_transfer", full=True, profile="W", lite=False):
    """The proofs/s half of the metric on one witness profile. full: sequential / 2 / 6 threads / batches of 256 (N = 1); lite: the
    same without the two-thread leg and verification (the profiles next to the headline one); else only the batched stream."""
    ps = ProveSetup(shape, profile)
    D, V, P = ps.synth.SHAPES[shape]
    first = ps.api.Groth16.prove_with_randomness(ps.ctx, ps.c.z, ps.rs[0][0], ps.rs[0][1])
    hist = ps.synth.histogram(ps.c.z_int)
    res = {"metric": f"Groth16 proofs/sec (manta-pay {shape} shape)", "unit": "proofs/s", "dtype": "u32", "data": "synthetic",
           "workload": f"Groth16 prove, shape-exact synthetic {shape} circuit (D={D}, V={V}, P={P}), BN254, valid key, witness profile "
                       f"'{profile}', assignment in page-locked memory; a step = one proof incl. H2D of z and the 128 proof bytes out",
           "witness_profile": profile,
           "z_histogram": {k: (round(v, 4) if k != "n" else v) for k, v in hist.items()},
           "z_histogram_note": "shares of the assignment PROVED (synth.histogram of the first of the distinct assignments; the others keep the "
                               "profile): 0 / 1 / other values below 2^64 / anything else. Zero scalars cost nothing, ones one addition, dense ones "
                               "a full set of windows -- arkworks and this library alike",
           "setup_s": round(ps.setup_s, 2)}
    try:
        tb = ps.ctx.table_bytes()
        res["key_tables_hbm_bytes"] = {"bucket_tables": tb[0], "full_tables": tb[1],
                                       "note": "full tables = every multiple of every window of the five queries; passes of ONE proof run on them "
                                               "(no sort, no bucket reduce), batched passes on the bucket tables; budget = mg_ctx_opts.full_table_bytes, "
                                               "default a tenth of the device's HBM per context"}
    except Exception as e:  # noqa: BLE001
        res["key_tables_hbm_bytes"] = {"error": str(e)}
    proofs = None
    if full or lite:
        n1 = max(20, min(100, args.steps * 5))
        dt, proofs, dts = ps.timed(env, n1, 1, 1, reps=3)
        assert proofs[0] == first
        res["sequential"] = _rate_stats(env, n1, dts, {"ms_per_proof": round(dt / n1 * 1e3, 4), "host_threads": 1, "proofs_per_call": 1})
        try:
            res["sequential"]["host_side_of_the_last_pass_ms"] = ps.api.last_pass_host_ms()
        except Exception:  # noqa: BLE001
            pass
        n2 = 3 * n1
        if full:
            dt, _, dts = ps.timed(env, n2, 2, 1, reps=3)
            res["two_threads"] = _rate_stats(env, n2, dts, {"host_threads": 2, "proofs_per_call": 1})
        dt, _, dts = ps.timed(env, 2 * n2, 6, 1, reps=3)  # the reference's simulation: six signer threads on one context (simulation.rs:36-38)
        res["six_threads"] = _rate_stats(env, 2 * n2, dts, {"host_threads": 6, "proofs_per_call": 1,
                                                             "note": "concurrent single calls are coalesced into batched passes by the library"})
    # configs[4]: batches of 256 proofs streamed through per-GPU pipelines -- one mg_groth16_prove_batch call per batch (the
    # library runs it as passes of ~29 proofs, three in flight); two host threads keep a second batch queued behind the first
    K = 256
    nb = K * (4 if full else 2)
    dt, pb, dts = ps.timed(env, nb, 2, K, reps=5 if full else (2 if lite else 1))  # (the headline: median of five repetitions)
    if args.dump_outputs and env.rank == 0:
        dump_outputs(args.dump_outputs, {"proofs": np.frombuffer(b"".join(pb), dtype=np.uint8).reshape(len(pb), -1)})
    assert pb[0] == first
    res["batched"] = _rate_stats(env, nb, dts, {"host_threads": 2, "proofs_per_call": K, "proofs": env.world * nb,
                      "ms_per_proof": round(dt / nb * 1e3, 4),
                      "assignments": ("%d distinct satisfying assignments per call (fresh public inputs and witnesses, synth.Reassigner), "
                                      "distinct (r, s) per proof" % K) if ps.distinct(K) else "one assignment repeated, distinct (r, s) per proof"})
    res["value"] = res["batched"]["proofs_per_s"]
    if full:  # SURVEY f-2: `Groth16::verify` on the GPU -- one proof at a time and 256 at once by random linear combination
        res["verify"] = verify_bench(ps, pb, ps.zs if ps.distinct(K) else None)
    res["n_gpus"] = env.world
    res["scaling"] = "weak (replicas: every GPU proves its own stream, no collective)"
    algo_bytes = 7 * 64 * D + 32 * V + 32 * D + 64 * (3 * V - P + D) + 128 * V
    nnz, m = int(len(ps.c.A.col) + len(ps.c.B.col) + len(ps.c.C.col)), int(ps.c.m)
    spmv_bytes = nnz * 36 + 3 * (m + 1) * 4 + 3 * m * 32  # SURVEY.md 8(d) SpMV term of THIS circuit (z is counted once above)
    with_spmv = algo_bytes + spmv_bytes
    res["roofline"] = {"bound": "hbm", "achieved": round(with_spmv * res["value"] / 1e9, 3), "peak": HBM_PEAK_GBPS * env.world, "unit": "GB/s",
                       "frac": round(with_spmv * res["value"] / 1e9 / (HBM_PEAK_GBPS * env.world), 6), "traffic": None,
                       "algorithmic_bytes_per_proof": with_spmv,
                       "algorithmic_bytes_per_proof_without_spmv": algo_bytes, "frac_without_spmv": round(algo_bytes * res["value"] / 1e9 / (HBM_PEAK_GBPS * env.world), 6),
                       "spmv_nnz": nnz,
                       "note": "whole-proof algorithmic bytes (SURVEY.md 8(d)) incl. the SpMV term of the synthetic circuit (%d non-zeros; the survey's "
                               "~68 MB assumed ~0.5 M of them); integer-multiply and latency bound: int_mad is the bound that governs" % nnz}
    if env.world == 1 and (full or lite):
        # the bound that governs: multiply-adds of the accumulate kernels of one proof against the issue peak measured NOW
        try:
            work = proof_work_model(ps.c)
            mhz, mad_per_us, _ = ps.api.clock_probe(60000)
            peak = mad_per_us * 1e6 * 1024 * 64 / 1e12
            bound = peak * 1e12 / work["mads_per_proof"]
            res["roofline"]["int_mad"] = dict(work, peak_Tmad_s=round(peak, 2), probe_MHz=round(mhz, 1),
                                              bound_proofs_per_s=round(bound, 1), batched_frac_of_bound=round(res["value"] / bound, 3),
                                              peak_how="issue rate measured in this run by mg_clock_probe x 1024 SIMDs x 64 lanes (no clock assumed)")
        except Exception as e:  # noqa: BLE001
            res["roofline"]["int_mad"] = {"error": str(e)}
    res["_cpu_todo"] = (ps, proofs if proofs else pb, 8 if profile != "dense" else 4) if (env.rank == 0 and env.world == 1 and not args.no_cpu_baseline) else None
    ps.release_gpu()  # the CPU baseline needs the host-side circuit / key / randomness only
    return res


def config2_cpu_baseline(c, pk, rs, first):
    """the same 2^20 proof on the host's cores (the arkworks-`parallel` decomposition of the restatement), once: a CPU number next to
    config2.ms and a byte comparison of the proof the GPU leg timed"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O  # the checker, here as the timed CPU baseline
    cores = O.set_threads(O.usable_cpus())
    t = time.perf_counter()
    want = O.groth16_prove(c, pk, rs[0], rs[1], msm_algo=1)
    t = time.perf_counter() - t
    O.set_threads(1)
    assert want == first, "config2: GPU proof bytes differ from the CPU restatement"
    return {"seconds": round(t, 2), "cores": cores, "kind": "port", "proofs_per_s": round(1 / t, 4), "bytes_equal_gpu": True}


def finish_cpu_baselines(line):
    """the timed CPU legs, after every GPU measurement of the run"""
    todo = line.pop("_cpu_todo", None)
    if todo:
        line["cpu_baseline"] = msm_cpu_baseline(*todo)
    c2 = line.get("config2")
    if isinstance(c2, dict):
        todo = c2.pop("_cpu_todo", None)
        if todo and line.get("cpu_baseline") is not None:  # (--no-cpu-baseline skips this one too)
            try:
                c2["cpu_all_cores"] = config2_cpu_baseline(*todo)
                c2["speedup_vs_cpu_all_cores"] = round(c2["cpu_all_cores"]["seconds"] * 1e3 / c2["prove_ms"], 1)
            except AssertionError:
                raise
            except Exception as e:  # noqa: BLE001
                c2["cpu_all_cores"] = {"error": str(e)}
    res = line.get("proofs")
    if res is not None:
        todo = res.pop("_cpu_todo", None)
        if todo:
            b = res["cpu_baseline"] = prove_cpu_baseline(*todo)
            ks = [k for k in ("sequential", "two_threads", "six_threads", "batched") if k in res]
            res["speedup_vs_cpu_1_thread"] = {k: round(res[k]["proofs_per_s"] / b["value"], 1) for k in ks}
            res["speedup_vs_cpu_all_cores"] = {k: round(res[k]["proofs_per_s"] / b["all_cores"]["value"], 1) for k in ks}


def prove_leg_in_child(args, env):
    """`python bench.py --workload prove --child` on this rank's GPU; ranks start their children together (barrier), every
    child times its own stream of proofs, the whole-job rate is the sum over ranks (replicas, no collective)."""
    import subprocess
    cenv = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MANTA_BENCH_DEVICE=str(env.dev))
    for k in ("MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID", "GROUP_RANK", "LOCAL_WORLD_SIZE", "ROLE_RANK"):
        cenv.pop(k, None)
    cmd = [sys.executable, os.path.abspath(__file__), "--full", "--workload", "prove", "--child", "--gpus", "1", "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    if args.no_cpu_baseline or env.world > 1 or env.rank != 0:
        cmd.append("--no-cpu-baseline")
    if env.world > 1:
        cmd.append("--batched-only")
        env.dist.barrier()
    out = subprocess.run(cmd, env=cenv, capture_output=True, text=True)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not lines:
        raise RuntimeError("proofs leg failed on rank %d:\n%s" % (env.rank, out.stdout[-2000:] + out.stderr[-2000:]))
    res = json.loads(lines[-1])
    if env.world == 1 and not args.quick:
        # the same legs on the other two witness profiles (their own circuits, keys and 256 distinct assignments
        # each, every one in a child process of its own like the headline profile); `proofs.value` is the W profile's batched rate
        def summary(r):
            keep = ("z_histogram", "sequential", "two_threads", "six_threads", "batched", "cpu_baseline", "speedup_vs_cpu_1_thread",
                    "speedup_vs_cpu_all_cores", "key_tables_hbm_bytes", "setup_s")
            out = {k: r[k] for k in keep if k in r}
            if "roofline" in r and "int_mad" in r["roofline"]:
                out["int_mad"] = r["roofline"]["int_mad"]
            return out
        res["witness_profiles"] = {"W": summary(res)}
        for prof in ("sparse", "dense"):
            c3 = cmd[:3] + ["--workload", "prove", "--child", "--profile", prof, "--lite", "--gpus", "1", "--steps", str(args.steps),
                            "--warmup", str(args.warmup)] + (["--no-cpu-baseline"] if args.no_cpu_baseline else [])
            o3 = subprocess.run(c3, env=cenv, capture_output=True, text=True)
            l3 = [ln for ln in o3.stdout.splitlines() if ln.startswith("{")]
            res["witness_profiles"][prof] = summary(json.loads(l3[-1])) if (o3.returncode == 0 and l3) else {"error": (o3.stdout[-500:] + o3.stderr[-800:])}
        res["witness_profiles"]["note"] = ("sparse = the generator of rounds 1-3 (multiplication gates cascade zeros: ~69 % zeros / 23 % ones -- a lower bound on "
                                           "the MSM work), W = SURVEY.md 8(d) config 2's 40 / 25 / 10 / 25 split enforced on the resulting z (the headline: "
                                           "proofs.value), dense = config 1's multiplication chain, no trivial scalar (the upper bound). No real "
                                           "`private_transfer::prove` witness can be captured in this image (rust/capture writes its histogram the day it runs)")
        # SURVEY a-11: the other two shapes of the reference's benches, batched stream only
        res["shapes"] = {}
        for shape in ("to_private", "to_public"):
            o2 = subprocess.run(cmd[:3] + ["--workload", "prove", "--child", "--shape", shape, "--batched-only", "--no-cpu-baseline", "--gpus", "1",
                                           "--steps", str(args.steps), "--warmup", str(args.warmup)], env=cenv, capture_output=True, text=True)
            l2 = [ln for ln in o2.stdout.splitlines() if ln.startswith("{")]
            if o2.returncode == 0 and l2:
                r2 = json.loads(l2[-1])
                res["shapes"][shape] = {"workload": r2["workload"], "batched": r2["batched"], "setup_s": r2["setup_s"]}
            else:
                res["shapes"][shape] = {"error": (o2.stdout[-500:] + o2.stderr[-500:])}
    if env.world > 1:
        parts = [None] * env.world
        env.dist.all_gather_object(parts, res["batched"])
        res["per_gpu_proofs_per_s"] = [round(p["proofs_per_s"], 2) for p in parts]
        res["batched"] = dict(res["batched"], proofs_per_s=round(sum(p["proofs_per_s"] for p in parts), 2),
                              proofs=sum(p["proofs"] for p in parts))
        res["value"] = res["batched"]["proofs_per_s"]
        res["n_gpus"] = env.world
        res["roofline"]["peak"] = HBM_PEAK_GBPS * env.world
        res["roofline"]["achieved"] = round(res["roofline"]["algorithmic_bytes_per_proof"] * res["value"] / 1e9, 3)
        res["roofline"]["frac"] = round(res["roofline"]["achieved"] / res["roofline"]["peak"], 6)
    return res


# ---------------------------------------------------------------------------------------------------- the printed line
LINE_HARD_CAP = 8192   # the driver keeps ~8 KB of stdout: round 4's 22 KB line came back `parsed: null`
LINE_TARGET = 4096


def _g(o, *path, default=None):
    """nested lookup that never raises: legs that did not run (quick, N > 1, an error object) give `default`"""
    for k in path:
        if not isinstance(o, dict) or k not in o or o[k] is None:
            return default
        o = o[k]
    return o


def _drop_none(o):
    if isinstance(o, dict):
        out = {k: _drop_none(v) for k, v in o.items() if v is not None}
        return {k: v for k, v in out.items() if v != {}}
    return o


def _three(leg):
    """the three numbers of a witness profile: sequential ms, six threads proofs/s, batched proofs/s"""
    return {"sequential_ms": _g(leg, "sequential", "ms_per_proof"), "six_threads": _g(leg, "six_threads", "proofs_per_s"),
            "batched": _g(leg, "batched", "proofs_per_s"), "cpu_1_thread": _g(leg, "cpu_baseline", "value"),
            "cpu_all_cores": _g(leg, "cpu_baseline", "all_cores", "value"),
            "batched_frac_of_int_mad_bound": _g(leg, "int_mad", "batched_frac_of_bound", default=_g(leg, "roofline", "int_mad", "batched_frac_of_bound"))}


def compact_line(full):
    """The ONE line the driver parses: numbers only, a few short strings, no notes. Everything else (how-strings, histograms,
    per-phase tables, min / max of the repetitions, the host probe) stays in the detail object, which main() writes to
    gpurun_out/bench_detail.json and, with --detail, to stderr -- never to stdout."""
    rl, cb, pr = full.get("roofline") or {}, full.get("cpu_baseline") or {}, full.get("proofs") or {}
    out = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                    "vs_baseline", "dtype", "data")}
    cfg = full.get("config") or {}
    out["config"] = {k: cfg[k] for k in ("workload", "curve", "log_n", "window_bits", "msms_in_flight", "sharding") if k in cfg}
    if "latency_mode" in cfg:
        out["config"]["one_at_a_time_Mscalar_s"] = _g(cfg, "latency_mode", "Mscalar_s")
    if cfg.get("plain_bases"):
        out["config"]["plain_bases_Mscalar_s"] = _g(cfg, "plain_bases", "pipelined_Mscalar_s")
    out["roofline"] = None if not rl else {
        "bound": rl.get("bound"), "kernel": rl.get("kernel"), "achieved": rl.get("achieved"), "peak": rl.get("peak"), "unit": rl.get("unit"),
        "frac": rl.get("frac"), "traffic": rl.get("traffic"), "kernel_ms": rl.get("kernel_ms"),
        "algorithmic_bytes_per_launch": rl.get("algorithmic_bytes_per_launch"),
        "int_mad": None if not rl.get("int_mad") else {
            "frac": _g(rl, "int_mad", "frac"), "peak_Tmad_s": _g(rl, "int_mad", "peak_Tmad_s"), "achieved_Tmad_s": _g(rl, "int_mad", "achieved_Tmad_s"),
            "frac_at_kernel_clock": _g(rl, "int_mad", "frac_at_the_kernels_own_clock")},
        "kernel_MHz": _g(rl, "clock", "accumulate_kernel_MHz_latency_mode")}
    out["cpu_baseline"] = None if not cb else {
        "value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
        "sample": "the same 2^%s bases/scalars, one whole MSM, arkworks-0.3 Pippenger restatement (oracle/)" % _g(cfg, "log_n", default="?"),
        "all_cores": {"value": _g(cb, "all_cores", "value"), "cores": _g(cb, "all_cores", "cores")}, "cpu_model": cb.get("cpu_model")}
    if pr:
        p = {"metric": pr.get("metric"), "value": pr.get("value"), "unit": "proofs/s", "profile": pr.get("witness_profile"),
             "sequential_ms": _g(pr, "sequential", "ms_per_proof"), "two_threads": _g(pr, "two_threads", "proofs_per_s"),
             "six_threads": _g(pr, "six_threads", "proofs_per_s"), "batched": _g(pr, "batched", "proofs_per_s"),
             "per_gpu": pr.get("per_gpu_proofs_per_s"),
             "int_mad": {"bound_proofs_per_s": _g(pr, "roofline", "int_mad", "bound_proofs_per_s"),
                         "batched_frac_of_bound": _g(pr, "roofline", "int_mad", "batched_frac_of_bound")},
             "cpu_baseline": None if not pr.get("cpu_baseline") else {
                 "value": _g(pr, "cpu_baseline", "value"), "unit": "proofs/s", "cores": 1, "kind": _g(pr, "cpu_baseline", "kind"),
                 "all_cores": {"value": _g(pr, "cpu_baseline", "all_cores", "value"), "cores": _g(pr, "cpu_baseline", "all_cores", "cores")}},
             "key_tables_hbm_bytes": (_g(pr, "key_tables_hbm_bytes", "bucket_tables", default=0) + _g(pr, "key_tables_hbm_bytes", "full_tables", default=0)) or None}
        wp = pr.get("witness_profiles")
        if wp:
            p["witness_profiles"] = {k: (_three(v) if "error" not in v else {"error": str(v["error"])[-120:]}) for k, v in wp.items() if isinstance(v, dict)}
        if pr.get("shapes"):
            p["shapes_batched"] = {k: _g(v, "batched", "proofs_per_s", default="error") for k, v in pr["shapes"].items()}
        out["proofs"] = p
        if pr.get("verify"):
            out["verify"] = {"single_ms": _g(pr, "verify", "single_ms"), "batch": _g(pr, "verify", "batch"),
                             "batch_per_s": _g(pr, "verify", "batch_proofs_per_s")}
    if full.get("ntt"):
        out["ntt"] = {"log_n": _g(full, "ntt", "log_n"), "ms": _g(full, "ntt", "fft", "device_ms"), "frac": _g(full, "ntt", "fft", "frac_of_hbm_peak"),
                      "ifft_ms": _g(full, "ntt", "ifft", "device_ms"), "coset_fft_ms": _g(full, "ntt", "coset_fft", "device_ms"),
                      "coset_ifft_ms": _g(full, "ntt", "coset_ifft", "device_ms")}
    if full.get("config2"):
        out["config2"] = {"ms": _g(full, "config2", "prove_ms"), "profile": _g(full, "config2", "witness_profile"),
                          "cpu_all_cores_s": _g(full, "config2", "cpu_all_cores", "seconds"), "cpu_cores": _g(full, "config2", "cpu_all_cores", "cores"),
                          "error": _g(full, "config2", "error")}
    if full.get("hbm_reference"):
        out["hbm_copy_TBps"] = _g(full, "hbm_reference", "d2d_copy_TBps")
    ss = full.get("strong_scaling")
    if ss:
        out["strong_scaling"] = {k: {"ms_per_msm": _g(v, "ms_per_msm_pipelined"), "Mscalar_s": _g(v, "Mscalar_s_pipelined")} for k, v in ss.items()
                                 if isinstance(v, dict)}
    sp = full.get("sharded_proof")
    if sp:
        out["sharded_proof"] = {"sequential_ms": _g(sp, "sequential", "ms_per_proof"), "batched": _g(sp, "batched", "proofs_per_s"),
                                "task_parallel_ms": _g(sp, "task_parallel", "sequential", "ms_per_proof"), "error": _g(sp, "error")}
    if full.get("errors"):
        out["errors"] = {k: str(v)[-160:] for k, v in full["errors"].items()}
    co = full.get("collective")
    if co:  # what the exchange actually ran on: torch's backend name, the group's size, the distinct physical devices
        out["collective"] = {"backend": co.get("backend"), "ranks": co.get("ranks"), "devices": co.get("devices"), "launcher": co.get("launcher"),
                             "parity_gate": None if not co.get("parity_gate") else "sharded proof == single-device proof on all ranks, verified"}
    out = _drop_none(out)
    for k in ("vs_baseline",):  # keys of the contract stay even when null
        out.setdefault(k, None)
    out["detail"] = full.get("_detail_path")
    s = json.dumps(out, separators=(",", ":"))
    if len(s) >= LINE_HARD_CAP:  # cannot happen with the fields above; if it ever does, shed the optional blocks rather than the headline
        for k in ("strong_scaling", "sharded_proof", "hbm_copy_TBps", "verify", "ntt", "config2", "errors", "proofs", "collective"):
            out.pop(k, None)
            s = json.dumps(out, separators=(",", ":"))
            if len(s) < LINE_HARD_CAP:
                break
    return s


def emit(full, args):
    """rank 0: detail object -> file (and stderr on --detail), compact line -> the LAST line of stdout"""
    full = dict(full)
    path = None
    blob = json.dumps(full, indent=1, default=str)
    for d in (os.path.join(ROOT, "gpurun_out"), "/tmp"):
        try:
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, "bench_detail_n%d.json" % full.get("n_gpus", 1))
            with open(path, "w") as f:
                f.write(blob)
            break
        except OSError:
            path = None
    full["_detail_path"] = os.path.relpath(path, ROOT) if path and path.startswith(ROOT) else path
    if getattr(args, "detail", False):
        sys.stderr.write("#detail " + json.dumps(full, default=str) + "\n")
        sys.stderr.flush()
    sys.stdout.flush()
    print(compact_line(full), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--quick", action="store_true", help="MSM headline only: skip plain-bases, strong-scaling and proofs legs")
    ap.add_argument("--workload", choices=["both", "msm", "prove"], default="both",
                    help="both (default) = the MSM line with the proofs half inside it; msm = configs[1] only; prove = a "
                         "proofs/s line of its own for --shape")
    ap.add_argument("--shape", default="private_transfer", choices=["to_private", "to_public", "private_transfer"])
    ap.add_argument("--profile", default="W", choices=["sparse", "W", "dense"],
                    help="witness profile of the proofs legs (manta_rs_amd/synth.py); the headline is W")
    ap.add_argument("--detail", action="store_true", help="also write the full detail object to stderr (it always goes to gpurun_out/bench_detail_n<N>.json)")
    ap.add_argument("--lite", action="store_true", help=argparse.SUPPRESS)          # internal: sequential / six threads / batched only
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)         # internal: print the proofs object only
    ap.add_argument("--batched-only", action="store_true", help=argparse.SUPPRESS)  # internal: skip the single-proof legs
    ap.add_argument("--full", action="store_true",
                    help="every leg besides the headline: correctness gates, latency mode, other inputs and sizes, the proofs half, NTT, the "
                         "2^20 proof, roofline and PMC traffic, strong scaling and the sharded proof (N > 1), CPU baselines. Without it a run "
                         "sets up, warms up, times --steps steps of the headline MSM and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    full_only = [name for name, given in (("--quick", args.quick), ("--workload", args.workload != "both"),
                                          ("--shape", args.shape != "private_transfer"), ("--profile", args.profile != "W"),
                                          ("--no-cpu-baseline", args.no_cpu_baseline), ("--detail", args.detail), ("--lite", args.lite),
                                          ("--child", args.child), ("--batched-only", args.batched_only)) if given]
    if full_only and not args.full:
        ap.error("%s: option(s) of the full run, add --full" % " ".join(full_only))
    if args.dump_outputs:
        args.dump_outputs = os.path.abspath(args.dump_outputs)  # the ranks below start in the repository root
    cmd = launch_plan(args.gpus, os.environ, sys.argv[1:] + (["--dump-outputs", args.dump_outputs] if args.dump_outputs else []))
    if cmd is not None:  # `python bench.py --gpus N` with no launcher around it: become the launcher
        sys.exit(self_launch(cmd))
    if args.workload == "prove" and not args.batched_only and os.environ.get("MANTA_BENCH_DISTINCT", "1") != "0":
        precompute_assignments(args.shape, 256, args.profile)  # before anything initialises HIP in this process
    env = Env(args)
    if not args.full:  # the plain run: the headline MSM and its line, nothing else
        line, _ = msm_bench(args, env)
        line["collective"] = env.collective
        if env.rank == 0:
            print(compact_line(line), flush=True)
        env.close()
        return
    if args.workload == "prove":
        res = prove_bench(args, env, args.shape, full=env.world == 1 and not args.batched_only and not args.lite, profile=args.profile,
                          lite=args.lite and env.world == 1)
        finish_cpu_baselines({"proofs": res})
        if args.child:
            print(json.dumps(res), flush=True)
            env.close()
            return
        if env.rank == 0:
            line = {"metric": res["metric"], "value": res["value"], "unit": "proofs/s", "n_gpus": env.world, "steps": args.steps,
                    "warmup": args.warmup, "ms_per_step": res["batched"]["ms_per_proof"], "higher_is_better": True, "scaling": "weak",
                    "vs_baseline": None, "dtype": "u32", "data": "synthetic", "config": {"workload": res["workload"]},
                    "roofline": res["roofline"], "cpu_baseline": res.get("cpu_baseline"), "proofs": res}
            emit(line, args)
        env.close()
        return
    # The proofs half runs in a CHILD PROCESS of its own (one per rank, same GPU, before this process touches the device):
    # both legs depend on how the HIP runtime maps their streams onto its 4 hardware queues, and whichever leg creates
    # its streams second in a shared process loses -- measured on MI355X: sequential proof 1.38 ms instead of 1.05 ms after
    # the MSM leg, pipelined MSM 320 instead of 345 Mscalar/s after the proofs leg. A deployment runs one or the other.
    proofs, errors = None, {}

    def leg(name, f, *a):
        """an optional leg must never cost the run its headline: its failure is recorded under `errors` (all ranks take the same
        branch only for failures that are deterministic; a rank-local failure in a collective leg still ends the run)"""
        try:
            return f(*a)
        except Exception as e:  # noqa: BLE001
            if env.world > 1:
                raise
            errors[name] = "%s: %s" % (type(e).__name__, e)
            return None
    gate = parity_gate(env) if env.world > 1 else None  # before anything is timed; any rank's failure ends the run
    if args.workload == "both" and not args.quick:
        proofs = leg("proofs", prove_leg_in_child, args, env)
    line, inst = msm_bench(args, env)
    line["collective"] = dict(env.collective, parity_gate=gate) if gate else env.collective
    if args.workload == "both" and not args.quick and env.world == 1:
        inst.bases.close()  # the 2 GiB window tables: the legs below allocate their own
        line["ntt"] = leg("ntt", ntt_bench, env)
        line["config2"] = leg("config2", config2_bench, env)
    if args.workload == "both" and not args.quick:
        if env.world > 1:
            line["strong_scaling"] = strong_scaling(args, env)
            line["sharded_proof"] = sharded_proof_bench(args, env)
        line["proofs"] = proofs
    finish_cpu_baselines(line)
    if errors:
        line["errors"] = errors
    if env.rank == 0:
        emit(line, args)
    env.close()


if __name__ == "__main__":
    main()
