"""The MSM inputs whose bucket sums and partials are NOT distinct random points: few distinct bases, so that the tail additions
behind the accumulate stage (XYZZ::add, CoopAdd; msm_reduce.h, accumulate_single) meet true doublings and cancellations. One
builder for tests/test_msm_tail_ref.py (the census of the plain-integer model, no GPU) and tests/test_gpu_msm_degenerate.py
(the same inputs on the GPU), so that a changed seed or vector cannot silently empty a class.

Every base is a small multiple m G of the generator (m = 0: infinity), so an input is (mults, scalars) and its MSM is
[sum_i k_i m_i mod r] G in closed form."""
import functools

import numpy as np

from manta_rs_amd import synth

CYCLE = (1, 1, -1, 2, 1, 0, -1, 1)          # the eight-point base cycle G, G, -G, 2G, G, infinity, -G, G
LANE_MIXED = (1, 1, -1, 2, 0, -2, 3, 1)     # all five addition classes between neighbouring lanes
# read from the TOP of a stretch of 8 buckets by serial_reduce (acc += X, sum += acc):
#   X     1      0      -2     -1     2      1      3   1
#   acc   1      1      -1     -2     0      1      4   5      (a_inf, o_inf, general, dbl, cancel, a_inf, ...)
#   sum   1      2       1     -1    -1      0      4   9      (a_inf, dbl, general, general, o_inf, cancel, ...)
FRONT_PATTERN = (1, 0, -2, -1, 2, 1, 3, 1)
WIDTHS = (7, 9, 13, 14)                     # T0 = 1 | 4 | 64 (front levels with MANTA_RED_MIN=128) | 128 (T1 = nP = 2)
SMALL_MULTIPLE = ((7, 512), (11, 4096), (13, 8192))  # (window_bits, n): uniform scalars on the base cycle, plain bases


def vectors(c):
    """{name: bucket vector v of 2^(c-1) small signed integers}: bucket j is to hold v_j G"""
    B = 1 << (c - 1)
    alt = [(-1) ** j for j in range(B)]
    out = {"ones": [1] * B, "alternating": alt, "lane_mixed": [LANE_MIXED[j % 8] for j in range(B)],
           "zero_total": alt[:B // 2] + [-x for x in alt[B // 2:]]}
    if B > 64:
        out["tile_alternating"] = [1 if (j // 64) % 2 == 0 else -1 for j in range(B)]
    if c == 13:
        out["front_pattern"] = [FRONT_PATTERN[7 - j % 8] for j in range(B)]
    return out


class Case:
    """One MSM: bases mults[i] G, scalars (Python integers), how the bases are built and launched.
    pre = precompute_window_bits, window_bits = the launch's window width for plain bases (0: the library's choice)."""

    def __init__(self, name, curve, mults, scalars, pre=0, window_bits=0, buckets=None):
        self.name, self.curve, self.pre, self.window_bits = name, curve, pre, window_bits
        self.mults, self.scalars, self.buckets = list(mults), list(scalars), buckets
        self.r = synth.FR_MODULUS[curve]
        assert len(self.mults) == len(self.scalars) <= 1 << 14
        self.k = sum(k * m for k, m in zip(self.scalars, self.mults)) % self.r  # the result is [k] G

    @property
    def c(self):
        return abs(self.pre) if self.pre else self.window_bits

    def limbs(self):
        return synth.ints_to_limbs([k % self.r for k in self.scalars], 4)


def _entries(v, scalar_of, copies):
    """one entry per bucket with the base v_j G (v_j = 0: an infinity base), or |v_j| copies of +-G"""
    mults, scalars = [], []
    for j, x in enumerate(v):
        for _ in range(abs(x) if copies else 1):
            mults.append((1 if x > 0 else -1) if copies else x)
            scalars.append(scalar_of(j))
    return mults, scalars


def dictated_cases(curve):
    """Window tables of width c with the scalars j + 1 <= 2^(c-1): only window 0 is non-zero and the entry lands in bucket j.
    Plain bases with window_bits = c and the scalars (j + 1)(1 + 2^(3c)): windows 0 and 3 hold the same content, every other
    window is empty."""
    out = []
    for c in WIDTHS:
        for name, v in vectors(c).items():
            for copies in (False, True):
                tag = "c%d.%s.%s" % (c, name, "copies" if copies else "bucket")
                m, k = _entries(v, lambda j: j + 1, copies)
                out.append(Case("tables." + tag, curve, m, k, pre=c, buckets=v))
                m, k = _entries(v, lambda j: (j + 1) * (1 + (1 << (3 * c))), copies)
                out.append(Case("plain." + tag, curve, m, k, window_bits=c, buckets=v))
    return out


def small_multiple_cases(curve):
    """uniform scalars on the eight-point base cycle, plain bases; and one input that cancels altogether: bases G, -G alternating
    under pairwise equal scalars"""
    out = []
    for c, n in SMALL_MULTIPLE:
        ks = synth.limbs_to_ints(synth.msm_scalars(curve, n, "U", seed=0xDE6E + c))
        out.append(Case("cycle.c%d.n%d" % (c, n), curve, [CYCLE[i % 8] for i in range(n)], ks, window_bits=c))
    ks = synth.limbs_to_ints(synth.msm_scalars(curve, 2048, "U", seed=0xDE6F))
    out.append(Case("cycle.cancels.c11", curve, [1, -1] * 2048, [k for k in ks for _ in (0, 1)], window_bits=11))
    return out


def merge_cases(curve):
    """One-point inputs for the merge levels and accumulate_single. Three distinct scalars over the bases G: the sorted pairs of
    a bucket all carry G, a lane's partial over L entries is L G, and the merge adds equal partials (with G, -G alternating under
    pairwise equal scalars: +-G partials for odd L, infinity for even L). Full tables and one digit s < 32: a single key, every
    lane of accumulate_single holds the same sum and its workgroup fold is doublings (G, -G alternating: cancellations)."""
    r = synth.FR_MODULUS[curve]
    rng = synth.XorShift(0xDE70 + curve)
    three = [rng.field(r) for _ in range(3)]
    n, out = 4096, []
    for pre in (0, 7):
        out.append(Case("merge.same.pre%d" % pre, curve, [1] * n, [three[i % 3] for i in range(n)], pre=pre))
        out.append(Case("merge.runs.pre%d" % pre, curve, [1] * n, [three[3 * i // n] for i in range(n)], pre=pre))
        out.append(Case("merge.negated.pre%d" % pre, curve, [1, -1] * (n // 2), [three[(i // 2) % 3] for i in range(n)], pre=pre))
    for s in (1, 21, 31):
        out.append(Case("full.same.s%d" % s, curve, [1] * 2048, [s] * 2048, pre=-6))
    out.append(Case("full.negated", curve, [1, -1] * 1024, [21] * 2048, pre=-6))
    return out


# the knob sets of the child processes (helpers.knob_env: any of them selects the diagnosis twin)
PLAIN = {"MANTA_COOP_TILES": "0", "MANTA_COOP_WAVES": "0"}
COOP = {"MANTA_COOP_TILES": "1073741824", "MANTA_COOP_WAVES": "1073741824"}
TAIL_KNOBS = {"plain": PLAIN, "coop": COOP, "plain.front": dict(PLAIN, MANTA_RED_MIN="128"),
              "coop.front": dict(COOP, MANTA_RED_MIN="128"), "coop.front.inline": dict(COOP, MANTA_RED_MIN="128", MANTA_RED_SIDE="0")}
MERGE_KNOBS = {"%s.L%d" % (name, L): dict(k, MANTA_MSM_L=str(L)) for name, k in (("plain", PLAIN), ("coop", COOP)) for L in (1, 2, 3)}
MERGE_KNOBS["coop.single_g2"] = dict(COOP, MANTA_ACC_SINGLE="3")  # G2 through accumulate_single too (the default: G1 only)


MULT_LO, MULT_HI = -4, 4  # every base is m G with MULT_LO <= m <= MULT_HI


def point_table(curve, group):
    """the affine points m G for m = MULT_LO .. MULT_HI (the oracle's fixed-base multiply; 0 -> infinity = zeros)"""
    import oracle_lib as O
    r = synth.FR_MODULUS[curve]
    tab = O.fixed_base_mul(curve, group, O.generator(curve, group), synth.ints_to_limbs([m % r for m in range(MULT_LO, MULT_HI + 1)], 4))
    tab[-MULT_LO] = 0
    return tab


def points(tab, mults):
    m = np.asarray(mults, dtype=np.int64)
    assert m.min() >= MULT_LO and m.max() <= MULT_HI
    return tab[m - MULT_LO]


def degenerate_key(curve):
    """(circuit, proving key) whose every query cycles through the eight points of CYCLE (G1 and G2): the key of a setup with
    the queries overwritten -- no valid key, but what the prover computes from it is defined, and the oracle computes it too"""
    import helpers as H
    import oracle_lib as O
    c = synth.make_circuit(curve, 1000, 700, 13)
    pk = O.groth16_setup(c, H.toxic(curve, seed=31))
    tabs = {g: point_table(curve, g) for g in (1, 2)}
    for f, g in (("a_query", 1), ("b_g1_query", 1), ("b_g2_query", 2), ("h_query", 1), ("l_query", 1)):
        q = getattr(pk, f)
        q[:] = points(tabs[g], [CYCLE[i % 8] for i in range(q.shape[0])])
    return c, pk


def prove_all(gpu, curve, c, pk):
    """three single proofs (eager, capture, replay), then prove_batch of three: [proof bytes], against fixed randomness"""
    import helpers as H
    rs = H.rand_fr_mont(curve, 6, seed=32)
    ctx = gpu.ProvingContext(curve, pk)
    ctx.set_r1cs(gpu.R1CS.from_circuit(c))
    out = [gpu.Groth16.prove_with_randomness(ctx, c.z, rs[i], rs[3 + i]) for i in range(3)]
    return out + gpu.Groth16.prove_batch(ctx, np.stack([c.z] * 3), rs[:3], rs[3:])


def expected(curve, group, case):
    """[k] G by one scalar multiplication, all-zero limbs for k = 0"""
    import oracle_lib as O
    G = O.generator(curve, group)
    return np.zeros_like(G) if case.k == 0 else O.g_mul(curve, group, G, synth.ints_to_limbs([case.k], 4)[0])


def pack(curve, group, cases):
    """the arrays of np.savez for a child process: the point table, and per case its multiples, scalars and expected result"""
    data = {"names": np.array([c.name for c in cases]), "pre": np.array([c.pre for c in cases]),
            "window_bits": np.array([c.window_bits for c in cases]), "table": point_table(curve, group)}
    for i, c in enumerate(cases):
        data["m%d" % i], data["sc%d" % i], data["want%d" % i] = np.array(c.mults, dtype=np.int8), c.limbs(), expected(curve, group, c)
    return data


@functools.lru_cache(maxsize=None)
def inputs(curve, group, kind):
    """(cases, packed arrays) of kind "tails" (dictated buckets + small multiples) or "merge" -- built once per process, shared by
    the host test, the in-process GPU run and the children, never changed"""
    cases = merge_cases(curve) if kind == "merge" else dictated_cases(curve) + small_multiple_cases(curve)
    return cases, pack(curve, group, cases)


def run(gpu, curve, group, data):
    """Every case of `data` through every entry point of the MSM on the GPU; -> one line per case, "<name> ok" or
    "<name> FAIL <entry points>". launch() and launch(sparse=True) take the case's window width, so for plain bases they see
    the dictated buckets; multi_scalar_mul has no such argument and runs plain bases at the library's own width (other buckets,
    the same few points); with tables every entry point, result_to_device included, sees the dictated buckets."""
    lines, tab = [], data["table"]
    for i, name in enumerate(data["names"]):
        pts, sc, want = points(tab, data["m%d" % i]), data["sc%d" % i], data["want%d" % i]
        pre, wb, n = int(data["pre"][i]), int(data["window_bits"][i]), sc.shape[0]
        b = gpu.Bases(curve, group, pts, precompute_window_bits=pre)
        d = gpu.DeviceBuffer.from_numpy(sc)
        got = {"multi_scalar_mul": gpu.VariableBaseMSM.multi_scalar_mul(b, sc),
               "launch": gpu.VariableBaseMSM.launch(b, d, n, window_bits=wb).finish(),
               "sparse": gpu.VariableBaseMSM.launch(b, d, n, window_bits=wb, sparse=True).finish()}
        if pre:  # fold_windows: the fold of the window sums on the device
            out = gpu.DeviceBuffer(gpu.xyzz_limbs(curve, group) * 8)
            job = gpu.VariableBaseMSM.launch(b, d, n, sparse=True)
            job.result_to_device(out.ptr)
            job.release()
            got["fold_windows"] = gpu.xyzz_sum(curve, group, out.to_numpy(shape=(1, gpu.xyzz_limbs(curve, group))))
        bad = [k for k, g in got.items() if not (g == want).all()]
        lines.append("%s %s" % (name, "FAIL " + ",".join(bad) if bad else "ok"))
        b.close()
    return lines
