// Element-wise prime-field arithmetic on the GPU through the kernels' own device functions -- the direct parity
// surface of SURVEY.md row a-10 (ark-ff 0.3 Fp256 / Fp384 Montgomery arithmetic, reached from
// manta-crypto/src/arkworks/groth16.rs:597): `mg_field_op` runs one operation over arrays of field elements in
// either of the two device representations,
//   repr 0: Fp<C>   saturated 32-bit limbs, R = 2^(32 N), always fully reduced (the ABI / arkworks memory format;
//                   NTT, SpMV, conversions)
//   repr 1: FpR<C>  reduced radix, lazily reduced (fpr_dev.h; the MSM kernels' internal format). Operands enter in
//                   the ABI format, are converted with from_std, then `lazy_a` / `lazy_b` times p is added limb-wise so
//                   that the operation sees a NON-canonical representative a + k p (what the kernels' intermediates
//                   look like), and the result is brought back with to_std (canonical).
// so that every function the Montgomery / lazy-reduction scheme consists of is compared with the CPU oracle (and with
// the reference-held BLS12-381 Fr Poseidon known answers) on edge values, not only through whole MSMs.
#include "fpr_dev.h"
#include "staging.h"
#include "params_gen.h"

namespace mg {

// the ABI's field ids -> f(an object of the field's configuration struct)
template <class F> static int with_field(int field, F f) {
    switch (field) {
    case 0: return f(Bn254FrCfg{});
    case 1: return f(Bn254FqCfg{});
    case 2: return f(Bls381FrCfg{});
    case 3: return f(Bls381FqCfg{});
    }
    return MG_ERR_ARG;
}

enum { FOP_ADD = 0, FOP_SUB = 1, FOP_MUL = 2, FOP_SQR = 3, FOP_NEG = 4, FOP_FROM_CANONICAL = 5, FOP_TO_CANONICAL = 6, FOP_INV = 7 };

template <class C> __device__ FpR<C> lazy_rep(const Fp<C> &s, int k) { // from_std(s) + k p, limbs renormalised
    typedef FpR<C> R;
    R r = R::from_std(s);
    if (k > 0) {
        R kp;
#pragma unroll
        for (int i = 0; i < R::K; ++i) {
            u32 v = 0;
#pragma unroll
            for (int m = 0; m <= C::RR_MAXM; ++m) v = (m == k) ? C::RR_MULT[m][i] : v;
            kp.v[i] = v;
        }
        r = R::add(r, kp);
    }
    return r;
}

template <class C>
__global__ __launch_bounds__(256) void field_op_kernel(int op, int repr, int lazy_a, int lazy_b, const u32 *__restrict__ a,
                                                       const u32 *__restrict__ b, u32 *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef Fp<C> S;
    typedef FpR<C> R;
    const S x = S::load(a + i * S::N);
    S y = S::zero();
    if (b) y = S::load(b + i * S::N);
    S r = S::zero();
    if (repr == 0) {
        switch (op) {
        case FOP_ADD: r = S::add(x, y); break;
        case FOP_SUB: r = S::sub(x, y); break;
        case FOP_MUL: r = S::mul(x, y); break;
        case FOP_SQR: r = S::sqr(x); break;
        case FOP_NEG: r = S::neg(x); break;
        case FOP_FROM_CANONICAL: r = S::to_mont(x); break;
        case FOP_TO_CANONICAL: r = S::from_mont(x); break;
        case FOP_INV: r = S::inv(x); break;
        }
    } else {
        // bounds: the representatives are < (lazy + 1) p <= 4 p, so products see operand bounds <= 4 x 4 = 16 <= RR_LIM
        // for all four fields (70 .. 2520), sums < 8 p, and sub<4> / neg<4> add a multiple that covers the subtrahend
        const R xr = lazy_rep<C>(x, lazy_a), yr = lazy_rep<C>(y, lazy_b);
        R t = R::zero();
        switch (op) {
        case FOP_ADD: t = R::add(xr, yr); break;                 // < 8 p
        case FOP_SUB: t = R::template sub<4>(xr, yr); break;     // a + 4p - b < 8 p
        case FOP_MUL: t = R::mul(xr, yr); break;                 // < 2 p
        case FOP_SQR: t = R::sqr(xr); break;
        case FOP_NEG: t = R::template neg<4>(xr); break;         // 4p - a
        case FOP_INV: t = R::inv(R::template reduce<4>(xr)); break;
        default: t = xr; break;                                  // 5 / 6: the conversion round trip itself
        }
        // every result above is < 8 p: reduce<8> brings it below 2 p (exercising the quotient estimate), to_std is the
        // final almost-Montgomery product with one conditional subtraction
        r = R::template reduce<8>(t).to_std();
        if (op == FOP_FROM_CANONICAL) r = S::to_mont(r);
        if (op == FOP_TO_CANONICAL) r = S::from_mont(r);
    }
    r.store(out + i * S::N);
}

template <class C> static int run(int op, int repr, int lazy_a, int lazy_b, const u32 *a, const u32 *b, size_t n, u32 *out) {
    const size_t bytes = n * Fp<C>::N * 4;
    DevCall m; // a | out | b (binary operations only)
    if (const int rc = m.begin({bytes, bytes, b ? bytes : 0}, "mg_field_op")) return rc;
    m.up(0, a, bytes);
    m.up(2, b, bytes);
    m.launch(field_op_kernel<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, op, repr, lazy_a, lazy_b, m.dev<u32>(0), m.dev<u32>(2),
             m.dev<u32>(1), n);
    m.down(out, 1, bytes);
    return m.finish();
}

int field_op(int field, int op, int repr, int lazy_a, int lazy_b, const u32 *a, const u32 *b, size_t n, u32 *out) {
    if (!a || !out || n == 0 || op < 0 || op > 7 || repr < 0 || repr > 1) return MG_ERR_ARG;
    if (lazy_a < 0 || lazy_a > 3 || lazy_b < 0 || lazy_b > 3 || (repr == 0 && (lazy_a || lazy_b))) return MG_ERR_ARG;
    const bool binary = op == FOP_ADD || op == FOP_SUB || op == FOP_MUL;
    if (binary && !b) return MG_ERR_ARG;
    if (!binary) b = nullptr;
    return with_field(field, [&](auto cfg) { return run<decltype(cfg)>(op, repr, lazy_a, lazy_b, a, b, n, out); });
}

// ---- the reduced-radix routines on RAW limb vectors (`mg_fpr_raw_op`): operands and result are K words of LB-bit limbs as the
// MSM kernels hold them, with no from_std / to_std around the operation -- mg_field_op above only ever feeds canonical values
// plus k p, which never puts a large value into every limb, the case the column accumulators of the products are sized for.
// coding 0 = FpR::mul / sqr / mul_add (the column walker FpR::product for BLS12-381 Fq, the interleaved bodies for the 29-bit fields)
// / sub2, 1 = the accumulate kernel's mul_t<true> / sqr_t<true> / mul_add_t<true> (the walker as a single chain for BLS12-381 Fq,
// the asm chains for the 29-bit fields) / sub2n.
enum { ROP_MUL = 0, ROP_SQR = 1, ROP_MUL_ADD = 2, ROP_SUB2_6 = 3, ROP_SUB2_12 = 4 };

template <class C>
__global__ __launch_bounds__(256) void fpr_raw_op_kernel(int op, int coding, const u32 *__restrict__ a, const u32 *__restrict__ b,
                                                         const u32 *__restrict__ c, const u32 *__restrict__ d, u32 *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef FpR<C> R;
    const R x = R::load(a + i * R::K);
    const R y = b ? R::load(b + i * R::K) : R::zero(), z = c ? R::load(c + i * R::K) : R::zero(), w = d ? R::load(d + i * R::K) : R::zero();
    R r = R::zero();
    switch (op) {
    case ROP_MUL: r = coding ? R::template mul_t<true>(x, y) : R::mul(x, y); break;
    case ROP_SQR: r = coding ? R::template sqr_t<true>(x) : R::sqr(x); break;
    case ROP_MUL_ADD: r = coding ? R::template mul_add_t<true>(x, y, z, w) : R::mul_add(x, y, z, w); break;
    case ROP_SUB2_6: r = coding ? R::template sub2n<6>(x, y, z) : R::template sub2<6>(x, y, z); break;
    case ROP_SUB2_12: r = coding ? R::template sub2n<12>(x, y, z) : R::template sub2<12>(x, y, z); break; // (the Fp2 additions' multiple)
    }
    r.store(out + i * R::K);
}

template <class C> static int run_raw(int op, int coding, const u32 *const (&in)[4], size_t n, u32 *out) {
    const size_t bytes = n * FpR<C>::K * 4;
    DevCall m; // out | a | b | c | d (absent operands take no room, and the kernel gets nullptr for them)
    if (const int rc = m.begin({bytes, bytes, in[1] ? bytes : 0, in[2] ? bytes : 0, in[3] ? bytes : 0}, "mg_fpr_raw_op")) return rc;
    for (int k = 0; k < 4; ++k) m.up(k + 1, in[k], bytes);
    m.launch(fpr_raw_op_kernel<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, op, coding, m.dev<u32>(1), m.dev<u32>(2), m.dev<u32>(3),
             m.dev<u32>(4), m.dev<u32>(0), n);
    m.down(out, 0, bytes);
    return m.finish();
}

int fpr_raw_op(int field, int op, int coding, const u32 *a, const u32 *b, const u32 *c, const u32 *d, size_t n, u32 *out) {
    if (!a || !out || n == 0 || n > ((size_t)1 << 24) || op < 0 || op > ROP_SUB2_12 || coding < 0 || coding > 1) return MG_ERR_ARG;
    const int operands = op == ROP_SQR ? 1 : (op == ROP_MUL ? 2 : (op == ROP_SUB2_6 || op == ROP_SUB2_12 ? 3 : 4));
    const u32 *const given[4] = {a, b, c, d};
    for (int k = 1; k < operands; ++k)
        if (!given[k]) return MG_ERR_ARG;
    const u32 *const in[4] = {a, operands > 1 ? b : nullptr, operands > 2 ? c : nullptr, operands > 3 ? d : nullptr};
    return with_field(field, [&](auto cfg) { return run_raw<decltype(cfg)>(op, coding, in, n, out); });
}

// the column plan of a field's products (fpr_dev.h), host side: flush[k] = FPR_FLUSH_* bits of column k, peak[k] = the
// planner's worst-case accumulator value of the column; returns the number of columns (2 K - 1) through *cols
template <class C> static int plan_out(int kind, u32 *flush, u64 *peak, int *cols, int *limb_bits, int *flushed_routines) {
    typedef FpR<C> R;
    // the tables the column walker indexes (flush_before), not a second run of the planner
    const typename R::Plan &pl = kind == FPR_KIND_MUL ? R::PLAN_MUL : (kind == FPR_KIND_SQR ? R::PLAN_SQR : R::PLAN_MUL_ADD);
    for (int k = 0; k < R::COLS; ++k) {
        if (flush) flush[k] = pl.flush[k];
        if (peak) peak[k] = pl.peak[k];
    }
    if (cols) *cols = R::COLS;
    if (limb_bits) *limb_bits = R::LB;
    if (flushed_routines) *flushed_routines = R::FLUSHES;
    return pl.fits ? MG_OK : MG_ERR_ARG;
}
int fpr_column_plan_host(int field, int kind, u32 *flush, u64 *peak, int *cols, int *limb_bits, int *flushed_routines) {
    if (kind < FPR_KIND_MUL || kind > FPR_KIND_MUL_ADD) return MG_ERR_ARG;
    return with_field(field, [&](auto cfg) { return plan_out<decltype(cfg)>(kind, flush, peak, cols, limb_bits, flushed_routines); });
}

} // namespace mg

// ---- clock probe (bench.py): what does the chip clock at under the accumulate kernel's kind of load? Every SIMD gets two
// wavefronts spinning on eight independent v_mad_u64_u32 chains each (the multiplier the MSM is bound by); each wavefront reads the
// shader-clock counter (s_memtime) and the constant-rate wall clock (s_memrealtime) before and after. ticks(s_memtime) per
// wall-clock second = the frequency s_memtime counts at during the load.
namespace mg {
__global__ __launch_bounds__(256) void clock_probe_kernel(u32 iters, u32 seed, unsigned long long *__restrict__ out) {
    unsigned long long acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = seed + threadIdx.x + 977u * k;
    const u32 m = 0x9e3779b9u ^ blockIdx.x;
    const long long c0 = clock64();
    const unsigned long long w0 = wall_clock64();
    for (u32 i = 0; i < iters; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = (unsigned long long)(u32)acc[k] * m + acc[k]; // v_mad_u64_u32, eight independent chains
    }
    const long long c1 = clock64();
    const unsigned long long w1 = wall_clock64();
    unsigned long long a = 0, b = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) a ^= acc[k];
    if ((threadIdx.x & 63) == 0) {
        const size_t w = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        out[3 * w] = (unsigned long long)(c1 - c0);
        out[3 * w + 1] = w1 - w0;
        out[3 * w + 2] = a ^ b; // keeps the chain alive
    }
}
// -> MHz of the s_memtime counter and of v_mad_u64_u32 issue (mads per SIMD-microsecond), duration of the probe in ms
int clock_probe(u32 iters, double *memtime_mhz, double *mad_issue_per_us_per_simd, double *ms) {
    int dev = 0, cus = 0, wall_khz = 0;
    MG_HIP(hipGetDevice(&dev));
    MG_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    MG_HIP(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, dev));
    const u32 blocks = (u32)cus * 2; // 256 threads = 4 wavefronts per block, two blocks per CU: two wavefronts per SIMD
    const size_t waves = (size_t)blocks * 4;
    struct Events { // destroyed on every path
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) hipEventDestroy(e0);
            if (e1) hipEventDestroy(e1);
        }
    } ev;
    MG_HIP(hipEventCreate(&ev.e0));
    MG_HIP(hipEventCreate(&ev.e1));
    std::vector<unsigned long long> h(waves * 3);
    DevCall m;
    if (const int rc = m.begin({h.size() * sizeof(unsigned long long)}, "clock probe")) return rc;
    unsigned long long *d = m.dev<unsigned long long>(0);
    m.launch(clock_probe_kernel, dim3(blocks), dim3(256), 0, 64u, 1u, d); // warm-up
    m.run([&] { return hipEventRecord(ev.e0, m.stream()); });
    m.launch(clock_probe_kernel, dim3(blocks), dim3(256), 0, iters, 2u, d);
    m.run([&] { return hipEventRecord(ev.e1, m.stream()); });
    m.down(h.data(), 0, h.size() * sizeof(unsigned long long));
    if (const int rc = m.finish()) return rc;
    float t = 0.f;
    hipEventElapsedTime(&t, ev.e0, ev.e1);
    double ratio = 0;
    for (size_t w = 0; w < waves; ++w) ratio += (double)h[3 * w] / (double)(h[3 * w + 1] ? h[3 * w + 1] : 1);
    ratio /= (double)waves;
    if (memtime_mhz) *memtime_mhz = ratio * (double)wall_khz / 1e3;
    // 32 multiply-adds per iteration and lane-wavefront, two wavefronts per SIMD
    if (mad_issue_per_us_per_simd) *mad_issue_per_us_per_simd = t > 0 ? 2.0 * 32.0 * (double)iters / ((double)t * 1e3) : 0;
    if (ms) *ms = t;
    return MG_OK;
}
} // namespace mg
