// Bulk group operations beside the MSM -- key generation (fixed-base multiplication), the trusted-setup ceremony (element-wise
// operations, group NTT, differences) and batch verification (the GLV multiply) -- and the type-erased host-point helpers:
// kernels and host code, GroupOpsT. Part of msm_impl.h. Nothing here knows the MSM: no base set, no plan, and of a workspace only
// `scratch` and `stream`; msm_engine.h includes this header ahead of everything of its own and GroupEngineT derives from GroupOpsT.
#pragma once
#include "../../include/mantagpu.h"
#include "msm_common.h"
#include "staging.h"
#include "msm_tables.h"

namespace mg {

// acc = [k] of a 256-bit scalar k, most significant bit first: one doubling per bit, then step(acc) where the bit is set. k is
// eight u32 words in memory, least significant first, or an Fp<C> in registers, whose limb is read with selects (a run-time index
// into the limb array would put it in scratch). In place: over Fp2 the group operations are calls on objects in scratch, and a
// ladder that returned its accumulator would cost the caller another point there.
static __device__ __forceinline__ u32 scalar_word(const u32 *k, int limb) { return k[limb]; }
template <class C> static __device__ __forceinline__ u32 scalar_word(const Fp<C> &k, int limb) {
    u32 w = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) w = (q == limb) ? k.v[q] : w;
    return w;
}
template <class F, class K, class Step> static __device__ __forceinline__ void double_and_add(XYZZ<F> &acc, const K &k, Step step) {
    acc = XYZZ<F>::inf();
    for (int limb = 7; limb >= 0; --limb) {
        const u32 w = scalar_word(k, limb);
        for (int bit = 31; bit >= 0; --bit) {
            acc = XYZZ<F>::dbl(acc);
            if ((w >> bit) & 1) step(acc);
        }
    }
}

// [k_i] * base, k canonical; output XYZZ (converted by xyzz_to_affine_batch)
template <class F>
__global__ __launch_bounds__(256) void fixed_base_mul_kernel(const u32 *__restrict__ base_aff,
                                                             const u32 *__restrict__ scalars, size_t n,
                                                             u32 *__restrict__ out_xyzz) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> b = Affine<F>::load(base_aff);
    XYZZ<F> acc;
    double_and_add(acc, scalars + i * 8, [&](XYZZ<F> &p) { p.madd(b, false); });
    acc.store(out_xyzz + i * XYZZ<F>::WORDS);
}

// Windowed fixed-base multiplication (key generation: every element of a Groth16 key is a multiple of a generator;
// ark-groth16 generate_parameters uses FixedBaseMSM the same way). Table T[w][d-1] = d * 2^(8w) * B for 32 windows of 8
// bits, d = 1..255 (8160 affine points, ~0.5 / 0.8 MB in G1: L2-resident); [k]B = at most 32 mixed additions, no doubling.
template <class F>
__global__ __launch_bounds__(256) void fixed_base_table_kernel(const u32 *__restrict__ base_aff, u32 *__restrict__ out_xyzz) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 32 * 255) return;
    const u32 w = t / 255, d = t % 255 + 1;
    const Affine<F> b = Affine<F>::load(base_aff);
    XYZZ<F> acc = XYZZ<F>::inf();
    for (int bit = 7; bit >= 0; --bit) { // d * B
        acc = XYZZ<F>::dbl(acc);
        if ((d >> bit) & 1) acc.madd(b, false);
    }
    for (u32 k = 0; k < 8 * w; ++k) acc = XYZZ<F>::dbl(acc); // * 2^(8w)
    acc.store(out_xyzz + (size_t)t * XYZZ<F>::WORDS);
}
template <class F>
__global__ __launch_bounds__(256) void fixed_base_mul_table_kernel(const u32 *__restrict__ table_aff, const u32 *__restrict__ scalars,
                                                                   size_t n, u32 *__restrict__ out_xyzz) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XYZZ<F> acc = XYZZ<F>::inf();
    for (int limb = 0; limb < 8; ++limb) {
        const u32 s = scalars[i * 8 + limb];
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const u32 d = (s >> (8 * k)) & 255u;
            if (d) acc.madd(Affine<F>::load(table_aff + ((size_t)(limb * 4 + k) * 255 + d - 1) * Affine<F>::WORDS), false);
        }
    }
    acc.store(out_xyzz + i * XYZZ<F>::WORDS);
}

// Radix-2 NTT over GROUP elements (`Radix2EvaluationDomain::{fft, ifft}` applied to a vector of points:
// manta-trusted-setup/src/groth16/mpc.rs:378-381 turns powers of tau into the Lagrange basis this way). One butterfly
// per lane and stage on XYZZ points in HBM: t = [w] b (double-and-add, w canonical from the Fr twiddle table),
// a' = a + t, b' = a - t. Input in bit-reversed order, output natural (decimation in time).
template <class F, class FrC>
__global__ __launch_bounds__(256) void group_ntt_stage_kernel(u32 *__restrict__ pts, const u32 *__restrict__ tw_mont, unsigned lg,
                                                              unsigned s) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1u << (lg - 1))) return;
    const u32 half = 1u << (s - 1), j = k & (half - 1), g = k >> (s - 1);
    const size_t i0 = ((size_t)g << s) | j, i1 = i0 + half;
    constexpr size_t XW = XYZZ<F>::WORDS;
    XYZZ<F> a = XYZZ<F>::load(pts + i0 * XW);
    const XYZZ<F> b = XYZZ<F>::load(pts + i1 * XW);
    XYZZ<F> t = b;
    if (s > 1) { // twiddle w_n^(j * n / 2^s); stage 1 has w = 1
        const Fp<FrC> wc = Fp<FrC>::from_mont(Fp<FrC>::load(tw_mont + ((size_t)j << (lg - s)) * 8));
        double_and_add(t, wc, [&](XYZZ<F> &p) { p.add(b); });
    }
    XYZZ<F> d = a;
    a.add(t);
    if (!t.is_inf()) {
        t.y = b_neg(bv<XYZZ<F>::BY>(t.y)).v;
        d.add(t);
    }
    a.store(pts + i0 * XW);
    d.store(pts + i1 * XW);
}
// affine (arkworks format) -> XYZZ internal at the bit-reversed position; and XYZZ internal -> scaled by a scalar -> std XYZZ
template <class F>
__global__ __launch_bounds__(256) void group_ntt_load_kernel(const u32 *__restrict__ in_aff, unsigned lg, u32 *__restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << lg)) return;
    const u32 j = lg ? (__brev(i) >> (32 - lg)) : 0;
    XYZZ<F>::from_affine(load_affine_std<F>(in_aff + (size_t)j * Affine<typename F::Std>::WORDS)).store(out + (size_t)i * XYZZ<F>::WORDS);
}
template <class F>
__global__ __launch_bounds__(256) void group_scale_store_kernel(const u32 *__restrict__ pts, const u32 *__restrict__ scalar_canon,
                                                                size_t n, u32 *__restrict__ out_xyzz_std) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef typename F::Std S;
    XYZZ<F> p = XYZZ<F>::load(pts + i * XYZZ<F>::WORDS);
    if (scalar_canon) { // ifft: times n^-1
        const XYZZ<F> b = p;
        double_and_add(p, scalar_canon, [&](XYZZ<F> &q) { q.add(b); });
    }
    p.store_std(out_xyzz_std + i * XYZZ<S>::WORDS);
}

// Element-wise group operations on arrays of affine points (arkworks format in, XYZZ in arkworks format out,
// normalised by xyzz_to_affine_batch) computed with the MSM kernels' own device functions in their internal
// field representation -- the primitive menu of manta-benchmark/src/ecc.rs:30-128 (mixed add :69-74, projective
// add :78-83, scalar multiplication :87-101, batch normalisation :114-119) as a parity-test surface. The first six are the
// MG_EC_* codes of the C ABI.
enum EcOp : int {
    EC_ADD_MIXED = 0, // P + Q via madd (projective += affine)
    EC_ADD = 1,       // P + Q via the general add (projective += projective)
    EC_DOUBLE = 2,    // 2P
    EC_MUL = 3,       // [k]P, k = 4 x u64 canonical (double-and-add over madd)
    EC_SUB_MIXED = 4, // P - Q via madd with the negate flag
    EC_MUL_FIXED = 5, // [k]P with ONE scalar k for all points (`batch_mul_fixed_scalar`, manta-trusted-setup/src/util.rs:440-445)
    EC_MUL_GLV = 6,   // internal (ec_mul_xyzz_begin): [k1 + lambda k2]P, 64-bit k1 and k2, through the endomorphism (G1 only)
};
static_assert(EC_ADD_MIXED == MG_EC_ADD_MIXED && EC_ADD == MG_EC_ADD && EC_DOUBLE == MG_EC_DOUBLE && EC_MUL == MG_EC_MUL &&
                  EC_SUB_MIXED == MG_EC_SUB_MIXED && EC_MUL_FIXED == MG_EC_MUL_FIXED,
              "EcOp is the C ABI's numbering");
template <class F>
__global__ __launch_bounds__(256) void ec_elementwise_kernel(EcOp op, const u32 *__restrict__ a, const u32 *__restrict__ b,
                                                             size_t n, u32 *__restrict__ out_xyzz_std) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef typename F::Std S;
    const Affine<F> pa = load_affine_std<F>(a + i * Affine<S>::WORDS);
    XYZZ<F> acc = XYZZ<F>::from_affine(pa);
    if (op == EC_ADD_MIXED || op == EC_SUB_MIXED) {
        acc.madd(load_affine_std<F>(b + i * Affine<S>::WORDS), op == EC_SUB_MIXED);
    } else if (op == EC_ADD) {
        acc.add(XYZZ<F>::from_affine(load_affine_std<F>(b + i * Affine<S>::WORDS)));
    } else if (op == EC_DOUBLE) {
        acc = XYZZ<F>::dbl(acc);
    } else if (op == EC_MUL_GLV) {
        // [k1 + lambda k2] P with 64-bit k1, k2 (the low two u64 of the lane's scalar) through the curve's endomorphism
        // phi(x, y) = (beta x, y) = lambda (x, y): ONE chain of 64 doublings with additions of P, phi(P) or P + phi(P) --
        // the general addition on a table entry picked by selects, so that every lane runs the same instruction stream
        // (128 doublings + 64 mixed additions for a 128-bit multiplier otherwise). beta: arkworks-format words behind the
        // n scalars in b. The batch verifier's random coefficients (verify.cpp).
        const S beta_std = S::load(b + n * 8);
        const F beta = F::from_std(beta_std);
        const XYZZ<F> t1 = acc;
        XYZZ<F> t2 = acc;
        if (!t1.is_inf()) t2.x = (bv<F::BM>(pa.x) * bv<F::BM>(beta)).v;
        XYZZ<F> t3 = t1;
        t3.add(t2);
        const u64 k1 = (u64)b[i * 8] | ((u64)b[i * 8 + 1] << 32), k2 = (u64)b[i * 8 + 2] | ((u64)b[i * 8 + 3] << 32);
        acc = XYZZ<F>::inf();
        for (int bit = 63; bit >= 0; --bit) {
            acc = XYZZ<F>::dbl(acc);
            const int sel = (int)((k1 >> bit) & 1) | ((int)((k2 >> bit) & 1) << 1);
            XYZZ<F> o;
            o.x = F::select(sel == 3, t3.x, F::select(sel == 2, t2.x, t1.x));
            o.y = F::select(sel == 3, t3.y, t1.y); // (phi keeps y)
            o.zz = F::select(sel == 3, t3.zz, t1.zz);
            o.zzz = F::select(sel == 3, t3.zzz, t1.zzz);
            if (sel) acc.add(o);
        }
    } else { // EC_MUL, EC_MUL_FIXED: every lane reads the same scalar there (uniform control flow)
        double_and_add(acc, b + (op == EC_MUL_FIXED ? 0 : i) * 8, [&](XYZZ<F> &p) { p.madd(pa, false); });
    }
    acc.store_std(out_xyzz_std + i * XYZZ<S>::WORDS);
}

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
template <class Curve, int GROUP> struct GT;
template <class Curve> struct GT<Curve, 1> {
#ifdef MG_G1_SATURATED
    typedef Fp<typename Curve::Fq> F; // 32-bit saturated limbs everywhere (A/B reference build)
#else
    typedef FpR<typename Curve::Fq> F; // internal: reduced radix, lazily reduced
#endif
    typedef Fp<typename Curve::Fq> FIO; // arkworks memory format at the ABI
    typedef host::HFp<typename Curve::Fq> HF;
};
template <class Curve> struct GT<Curve, 2> {
    // G2 on the lazily-reduced Fp2R as well, its base products inlined (13 limbs over BLS12-381; the calls that 14 limbs needed
    // are recorded in profiles/history/code_comment_measurements.md). MG_G2_SATURATED keeps the canonical 32-bit Fp2 path for A/B.
#ifdef MG_G2_SATURATED
    typedef Fp2<typename Curve::Fq> F;
#else
    typedef Fp2R<typename Curve::Fq> F;
#endif
    typedef Fp2<typename Curve::Fq> FIO;
    typedef host::HFp2<typename Curve::Fq> HF;
};

// fixed_base_mul builds its table from this many scalars on (A/B knob, tuning.h ab_knob)
static size_t fixed_base_table_min() {
    static const size_t v = (size_t)ab_knob("MANTA_FIXED_BASE_TABLE_MIN", 16384);
    return v;
}

template <class Curve, int CURVE_ID, int GROUP> class GroupOpsT : public GroupEngine {
  public:
    typedef typename GT<Curve, GROUP>::F F;
    typedef typename GT<Curve, GROUP>::FIO FIO;
    typedef typename GT<Curve, GROUP>::HF HF;
    typedef host::HPoint<HF> HP;
    typedef typename Curve::Fr FrC;
    static constexpr int AW = Affine<F>::WORDS, XW = XYZZ<F>::WORDS;           // internal formats
    static constexpr int AW_IO = Affine<FIO>::WORDS, XW_IO = XYZZ<FIO>::WORDS; // arkworks formats (ABI, staging)
    static_assert(sizeof(HP) <= sizeof(HostPoint), "HostPoint too small");

    int curve() const override { return CURVE_ID; }
    int group() const override { return GROUP; }
    int affine_words() const override { return AW_IO; }
    int xyzz_words() const override { return XW_IO; }
    int scalar_bits() const override { return FrC::BITS; }
    int point_bytes(bool compressed) const override { return compressed ? HF::BYTES : 2 * HF::BYTES; }

    static HP &hp(HostPoint *p) { return *reinterpret_cast<HP *>(p); }
    static const HP &hp(const HostPoint *p) { return *reinterpret_cast<const HP *>(p); }
    void hp_set_inf(HostPoint *p) const override { hp(p) = HP::inf(); }
    void hp_from_affine(HostPoint *p, const u32 *w) const override { hp(p) = HP::from_affine_words(w); }
    void hp_from_xyzz(HostPoint *p, const u32 *w) const override { hp(p) = HP::from_xyzz_words(w); }
    void hp_add(HostPoint *a, const HostPoint *o) const override { hp(a) = HP::add(hp(a), hp(o)); }
    void hp_neg(HostPoint *p) const override { hp(p) = hp(p).neg(); }
    void hp_mul(HostPoint *p, const u64 *k4) const override { hp(p) = HP::mul(hp(p), k4, 4); }
    void hp_mul2(const HostPoint *p, const u64 *k1, const HostPoint *q, const u64 *k2, HostPoint *out) const override {
        hp(out) = HP::mul2(hp(p), k1, hp(q), k2, 4);
    }
    void *hp_table_create(const HostPoint *base) const override {
        auto *t = new host::FixedBaseTable<HP>();
        t->build(hp(base));
        return t;
    }
    void hp_table_mul(const void *table, const u64 *k4, HostPoint *out) const override {
        hp(out) = static_cast<const host::FixedBaseTable<HP> *>(table)->mul(k4);
    }
    void hp_table_free(void *table) const override { delete static_cast<host::FixedBaseTable<HP> *>(table); }
    void hp_to_affine(const HostPoint *p, u32 *w) const override { hp(p).to_affine_words(w); }
    void hp_serialize(const HostPoint *p, unsigned char *out, bool compressed) const override {
        hp(p).serialize(out, compressed);
    }

    // ---------------------------------------------------------------- fixed-base batch mul
    int fixed_base_mul(const u32 *base_affine_host, const u32 *d_scalars, size_t n, u32 *d_out_affine,
                       hipStream_t s) override {
        DevBlock table; // the 32 x 255 multiples of the base as XYZZ | affine
        DevCall m;      // base | XYZZ results; on the caller's stream, or the setup stream (never the NULL stream: engine.h)
        if (const int rc = m.begin({AW_IO * 4, n * XW_IO * 4}, "fixed_base_mul", false, s)) return rc;
        s = m.stream();
        u32 *d_base = m.dev<u32>(0), *tmp = m.dev<u32>(1);
        m.up(0, base_affine_host, AW_IO * 4);
        m.run([&] {
            constexpr size_t TN = 32 * 255;
            // many multiples of one base: 32 table additions each instead of ~380 group operations -- when the table's memory can be had
            if (n >= fixed_base_table_min() && table.try_alloc({TN * XW_IO * 4, TN * AW_IO * 4})) {
                u32 *t_xyzz = table.dev<u32>(0), *t_aff = table.dev<u32>(1);
                hipLaunchKernelGGL((fixed_base_table_kernel<FIO>), dim3(cdiv(TN, 256)), dim3(256), 0, s, d_base, t_xyzz);
                xyzz_to_affine_launch<FIO>(s, t_xyzz, TN, t_aff, AW_IO);
                hipLaunchKernelGGL((fixed_base_mul_table_kernel<FIO>), dim3(cdiv(n, 256)), dim3(256), 0, s, t_aff, d_scalars, n, tmp);
            } else {
                hipLaunchKernelGGL((fixed_base_mul_kernel<FIO>), dim3(cdiv(n, 256)), dim3(256), 0, s, d_base, d_scalars, n, tmp);
            }
            xyzz_to_affine_launch<FIO>(s, tmp, n, d_out_affine, AW_IO);
        });
        return m.finish();
    }

    // ---------------------------------------------------------------- element-wise operations
    int ec_elementwise(int op, const u32 *a_host, const u32 *b_host, size_t n, u32 *out_affine_host) override {
        if (op < EC_ADD_MIXED || op > EC_MUL_FIXED || !a_host || !out_affine_host || n == 0 || (op != EC_DOUBLE && !b_host))
            return MG_ERR_ARG;
        const size_t ab = n * AW_IO * 4, bb = op == EC_MUL ? n * 32 : (op == EC_MUL_FIXED ? 32 : ab);
        // a stream of its own (not stream 0: a synchronous copy anywhere else in the process -- another thread creating a base
        // set, say -- would wait for this kernel, a millisecond of one-lane latency for 128-bit multipliers)
        hipStream_t st = stream_pool_get_normal(); // (pooled: the library destroys no stream, streams.cpp)
        if (!st) return hip_status(hipErrorOutOfMemory, "ec_elementwise");
        DevCall m; // a | b | XYZZ results | affine results
        int rc = m.begin({ab, bb, n * XW_IO * 4, ab}, "ec_elementwise", false, st);
        if (!rc) {
            m.up(0, a_host, ab);
            if (op != EC_DOUBLE) m.up(1, b_host, bb);
            m.launch(ec_elementwise_kernel<F>, dim3(cdiv(n, 256)), dim3(256), 0, (EcOp)op, m.dev<u32>(0), m.dev<u32>(1), n, m.dev<u32>(2));
            m.run([&] { xyzz_to_affine_launch<FIO>(st, m.dev<u32>(2), n, m.dev<u32>(3), AW_IO); });
            m.down(out_affine_host, 3, ab);
            rc = m.finish();
        }
        stream_pool_put_normal(st); // (finished: nothing of the call is in flight on it)
        return rc;
    }

    // The multiplication k_i P_i (EC_MUL, or EC_MUL_GLV when beta is given) ahead of other work: uploads into the workspace's
    // grow-only scratch buffer and launches on the workspace's stream (no hipMalloc / hipFree / stream 0: nothing else on the
    // device waits for it and it waits for nothing). ec_mul_xyzz_device says where the kernel leaves the n XYZZ results.
    struct MulScratch { // byte offsets in ws->scratch: points at 0 | scalars | beta (GLV only) | results | end
        size_t k, beta, out, end;
        MulScratch(size_t n, bool glv)
            : k(n * AW_IO * 4), beta(k + n * 32), out(beta + (glv ? (size_t)AW_IO / 2 * 4 : 0)), end(out + n * XW_IO * 4) {}
    };
    int ec_mul_xyzz_begin(const u32 *a_host, const u32 *k_host, size_t n, MsmWorkspace *ws, const u32 *glv_beta_std) override {
        if (!a_host || !k_host || !n || !ws) return MG_ERR_ARG;
        const MulScratch at(n, glv_beta_std != nullptr);
        if (const int rc = ws->scratch.reserve(at.end)) return rc;
        unsigned char *d = (unsigned char *)ws->scratch.p;
        hipError_t e = hipMemcpyAsync(d, a_host, at.k, hipMemcpyHostToDevice, ws->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d + at.k, k_host, n * 32, hipMemcpyHostToDevice, ws->stream);
        if (e == hipSuccess && glv_beta_std)
            e = hipMemcpyAsync(d + at.beta, glv_beta_std, at.out - at.beta, hipMemcpyHostToDevice, ws->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL((ec_elementwise_kernel<F>), dim3(cdiv(n, 256)), dim3(256), 0, ws->stream,
                               glv_beta_std ? EC_MUL_GLV : EC_MUL, (const u32 *)d, (const u32 *)(d + at.k), n, (u32 *)(d + at.out));
            e = hipGetLastError();
        }
        return e == hipSuccess ? MG_OK : sync_status(ws->stream, e, "ec_mul_xyzz"); // (a failure waits for what was enqueued)
    }
    const u32 *ec_mul_xyzz_device(MsmWorkspace *ws, size_t n, bool glv) const override {
        return ws && ws->scratch.p ? (const u32 *)((unsigned char *)ws->scratch.p + MulScratch(n, glv).out) : nullptr;
    }

    // ---------------------------------------------------------------- group NTT, differences
    // NTT over group elements: host affine in, host affine out (natural order both); tw = the Fr domain's device twiddle
    // table (omega^k, k < n/2, Montgomery), n_inv_canonical = n^-1 for the inverse transform (nullptr: forward)
    int group_ntt(const u32 *in_affine_host, unsigned lg, const u32 *d_twiddles_mont, const u32 *n_inv_canonical,
                  u32 *out_affine_host) override {
        if (!in_affine_host || !out_affine_host || lg > 26 || (lg > 0 && !d_twiddles_mont)) return MG_ERR_ARG;
        const size_t n = (size_t)1 << lg, ab = n * AW_IO * 4;
        DevCall m; // affine in | affine out
        if (const int rc = m.begin({ab, ab}, "group_ntt")) return rc;
        m.up(0, in_affine_host, ab);
        m.run([&] { return group_ntt_device(m.dev<u32>(0), lg, d_twiddles_mont, n_inv_canonical, m.dev<u32>(1)); });
        m.down(out_affine_host, 1, ab);
        return m.finish();
    }
    // the transform itself, device array to device array (`mpc::initialize`: the Lagrange bases never leave HBM)
    int group_ntt_device(const u32 *d_in, unsigned lg, const u32 *d_twiddles_mont, const u32 *n_inv_canonical, u32 *d_out) override {
        if (!d_in || !d_out || lg > 26 || (lg > 0 && !d_twiddles_mont)) return MG_ERR_ARG;
        const size_t n = (size_t)1 << lg;
        DevCall m; // working XYZZ | arkworks-format XYZZ | n^-1 (inverse transform only)
        if (const int rc = m.begin({n * XW * 4, n * XW_IO * 4, n_inv_canonical ? 32u : 0u}, "group_ntt")) return rc;
        hipStream_t st = m.stream();
        u32 *d_pts = m.dev<u32>(0), *d_std = m.dev<u32>(1), *d_sc = m.dev<u32>(2);
        m.up(2, n_inv_canonical, 32);
        m.run([&] {
            hipLaunchKernelGGL((group_ntt_load_kernel<F>), dim3(cdiv(n, 256)), dim3(256), 0, st, d_in, lg, d_pts);
            for (unsigned s = 1; s <= lg; ++s)
                hipLaunchKernelGGL((group_ntt_stage_kernel<F, FrC>), dim3(cdiv(n / 2, 256)), dim3(256), 0, st, d_pts, d_twiddles_mont, lg, s);
            hipLaunchKernelGGL((group_scale_store_kernel<F>), dim3(cdiv(n, 256)), dim3(256), 0, st, d_pts, (const u32 *)d_sc, n, d_std);
            xyzz_to_affine_launch<FIO>(st, d_std, n, d_out, AW_IO);
        });
        return m.finish();
    }
    int sub_device(const u32 *d_a, const u32 *d_b, size_t n, u32 *d_out) override {
        if (!d_a || !d_b || !d_out || n == 0) return MG_ERR_ARG;
        DevCall m; // XYZZ results
        if (const int rc = m.begin({n * XW_IO * 4}, "sub_device")) return rc;
        m.launch(ec_elementwise_kernel<F>, dim3(cdiv(n, 256)), dim3(256), 0, EC_SUB_MIXED, d_a, d_b, n, m.dev<u32>(0));
        m.run([&] { xyzz_to_affine_launch<FIO>(m.stream(), m.dev<u32>(0), n, d_out, AW_IO); });
        return m.finish();
    }
};

} // namespace mg
