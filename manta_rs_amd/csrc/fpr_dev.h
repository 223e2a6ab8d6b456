// Reduced-radix ("carry-free") prime-field arithmetic for gfx950 -- the internal representation of
// the MSM, tail, table, QAP and group-NTT kernels.
//
// Why: CDNA4 has no multiply-with-carry-in. With saturated 32-bit limbs every 32x32 product costs one
// v_mad_u64_u32 (4.2 cycles/wave) PLUS one v_addc_co_u32 (4.3 cycles, serialised through VCC) -- half of
// Fp::mul's cycles are carries (measured: tools/ubench3.hip, profiles/r01_ubench3_reduced_radix_mul.txt).
// With K limbs of LB < 32 bits a column of products fits a 64-bit accumulator, so a product is
// exactly one v_mad_u64_u32 and a column costs one shift + mask: 1.55x faster at the accumulate kernel's
// occupancy, although it needs (K/N)^2 ~ 1.3x more multiplies.
//
//   BN254 Fq, BN254 Fr, BLS12-381 Fr: K = 9 limbs x 29 bits (R' = 2^261);  BLS12-381 Fq: K = 13 x 30 bits (R' = 2^390).
//
// A column of 29-bit limbs never comes near 2^64. With 30-bit limbs sixteen products do, so the column plan below says where
// such a column moves its accumulator's upper part aside ("flush"). ONE routine, FpR::product, walks the columns of a*b, a^2
// and a*b + c*d by that plan, group by group; it is the product of the field that flushes, in both of its C codings. A plan
// without flushes would make it the plain product of the 29-bit fields as well, but there the interleaved bodies (mul, sqr,
// mul_add below) are kept: grouped, the BN254 kernels cost the dense single proof 1.5 % (profiles/fpr_product_walker.txt).
//
// Values are kept LAZILY reduced: limbs are always normalised (< 2^LB), the integer value may be any
// representative below a small multiple of p (bounds are tracked per call site in ec_dev.h). Because
// R' >= 2^6 p, an "almost Montgomery" product of inputs a < Ba*p, b < Bb*p is < 2p whenever
// Ba*Bb <= RR_LIM = floor(R'/p) (70 .. 630 over the four fields), with no final subtraction. Subtractions add a multiple M*p
// chosen from the subtrahend's bound. Exact tests (is_zero_mod) compare against the multiples of p.
//
// Memory format: K u32 words per element. Conversion to/from the arkworks format (32-bit limbs,
// R = 2^(32N)) happens once, when bases are registered and when the few result points are staged.
//
// Compile-time switches of this header, all for A/B builds (tools/build_variant.sh); the defaults are the measured choices:
//   MG_CHAIN_FLUSHED   (default 1) single-chain coding of mul_t / sqr_t / mul_add_t<true> for the 30-bit field too: the column
//                      walker with every multiply-add pinned in C (mad_link), no asm; 0 = the compiler's two chains per column.
//                      Measurements in profiles/fpr_chain_padding_ab.txt
//   MG_SUB2_64         the mixed addition's sub2n of the 30-bit field with 64-bit carries (= sub2) instead of signed 32-bit limbs
//   MG_PACK_AFFINE     memory format of affine base coordinates (0 / 1 / 2, see load_aff)
// (Retired switches and what they measured: profiles/history/code_comment_measurements.md.)
#pragma once
#include "fp_dev.h"

#ifndef MG_CHAIN_FLUSHED
#define MG_CHAIN_FLUSHED 1
#endif

namespace mg {

// acc += a*b as ONE v_mad_u64_u32 the compiler may not re-associate: all multiply-adds of a column then form a single
// dependent chain (the C expression is split into an a*b chain and an m*p chain joined by a v_lshl_add_u64 per column:
// 28 more instructions per 14-limb product). Faster by 3.5-5.4 % at >= 2 wavefronts per SIMD, 35 % slower at one
// (profiles/r02_ubench4_fma_vs_int.txt) -- so only the throughput-bound accumulate kernel asks for it (CH = true), and
// there it pays only with SEVERAL links per asm block (below): -3 % kernel time on both curves.
MG_DEV void mad_chain_vv(u64 &acc, u32 a, u32 b) { asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b) : "vcc"); }
MG_DEV void mad_chain_vs(u64 &acc, u32 a, u32 k) { asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(a), "s"(k) : "vcc"); }
// Several links of the chain in ONE asm block: the compiler puts an s_nop after every asm statement (it cannot see inside),
// which at one statement per multiply-add cost more than the single chain saved (~3 400 per loop body).
MG_DEV void mad_chain_pair(u64 &acc, u32 a, u32 b, u32 m, u32 k) { // a*b + m*k
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\tv_mad_u64_u32 %0, vcc, %3, %4, %0" : "+v"(acc) : "v"(a), "v"(b), "v"(m), "s"(k) : "vcc");
}
MG_DEV void mad_chain_pair2(u64 &acc, u32 a0, u32 b0, u32 m0, u32 k0, u32 a1, u32 b1, u32 m1, u32 k1) {
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\tv_mad_u64_u32 %0, vcc, %3, %4, %0\n\t"
        "v_mad_u64_u32 %0, vcc, %5, %6, %0\n\tv_mad_u64_u32 %0, vcc, %7, %8, %0"
        : "+v"(acc)
        : "v"(a0), "v"(b0), "v"(m0), "s"(k0), "v"(a1), "v"(b1), "v"(m1), "s"(k1)
        : "vcc");
}
MG_DEV void mad_chain_vv2(u64 &acc, u32 a0, u32 b0, u32 a1, u32 b1) {
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\tv_mad_u64_u32 %0, vcc, %3, %4, %0" : "+v"(acc) : "v"(a0), "v"(b0), "v"(a1), "v"(b1) : "vcc");
}
MG_DEV void mad_chain_vs2(u64 &acc, u32 m0, u32 k0, u32 m1, u32 k1) {
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\tv_mad_u64_u32 %0, vcc, %3, %4, %0" : "+v"(acc) : "v"(m0), "s"(k0), "v"(m1), "s"(k1) : "vcc");
}
MG_DEV void mad_chain_triple(u64 &acc, u32 a, u32 b, u32 c, u32 d, u32 m, u32 k) { // a*b + c*d + m*k
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\tv_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_mad_u64_u32 %0, vcc, %5, %6, %0"
        : "+v"(acc)
        : "v"(a), "v"(b), "v"(c), "v"(d), "v"(m), "s"(k)
        : "vcc");
}
MG_DEV void mad_chain_triple2(u64 &acc, u32 a0, u32 b0, u32 c0, u32 d0, u32 m0, u32 k0, u32 a1, u32 b1, u32 c1, u32 d1, u32 m1, u32 k1) {
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\tv_mad_u64_u32 %0, vcc, %3, %4, %0\n\tv_mad_u64_u32 %0, vcc, %5, %6, %0\n\t"
        "v_mad_u64_u32 %0, vcc, %7, %8, %0\n\tv_mad_u64_u32 %0, vcc, %9, %10, %0\n\tv_mad_u64_u32 %0, vcc, %11, %12, %0"
        : "+v"(acc)
        : "v"(a0), "v"(b0), "v"(c0), "v"(d0), "v"(m0), "s"(k0), "v"(a1), "v"(b1), "v"(c1), "v"(d1), "v"(m1), "s"(k1)
        : "vcc");
}

// ---- compile-time column plan of the products (it holds a flush only for limbs wide enough that a column of a product can pass
// 2^64: LB = 30). A column k adds its products group by group -- a*b, then c*d (the fused product), then m*p -- into one 64-bit
// accumulator; before a group that could carry the accumulator to 2^64 the accumulator's upper part is moved aside ("flush").
// The planner walks the columns in the order the code adds them and keeps the EXACT worst case of every partial sum:
//   carry-in  = floor(worst total of the previous column / 2^LB)   (a flush moves value aside, it does not change the total)
//   a*b, c*d  = n * limb^2        (n products of the column; `limb` bounds every operand limb, 2^LB - 1 when normalised; the doubled
//                                  operand of a squaring makes a cross product count twice, which is the same n * limb^2)
//   m*p       = (2^LB - 1) * sum of the limbs p_j the column touches  (m_i is masked; p's limbs are the constants themselves)
// After a flush the accumulator holds at most 2^LB - 1. The plan is built ONCE per field and kind (static constexpr members of
// FpR below); the product routines only index it.
enum { FPR_KIND_MUL = 0, FPR_KIND_SQR = 1, FPR_KIND_MUL_ADD = 2 };
enum { FPR_FLUSH_AB = 1, FPR_FLUSH_CD = 2, FPR_FLUSH_MP = 4 }; // flush BEFORE the a*b / c*d / m*p group of the column
template <int COLS> struct FprColumnPlan {
    unsigned char flush[COLS]; // FPR_FLUSH_* bits per column
    u64 peak[COLS];            // worst-case accumulator value of the column under this plan
    u64 spill_peak;            // worst-case value of the spill word
    int flushes;               // flushes in the whole product
    bool fits;                 // no group alone reaches 2^64 (else there is no plan)
};
template <class C> constexpr FprColumnPlan<2 * C::RR_K - 1> fpr_column_plan(int kind, u64 limb) {
    constexpr int K = C::RR_K, LB = C::RR_LB;
    constexpr u64 MASK = ((u64)1 << LB) - 1, TOP = ~(u64)0;
    FprColumnPlan<2 * K - 1> pl{};
    pl.fits = limb <= 0xffffffffull;
    u64 carry = 0;
    for (int k = 0; k < 2 * K - 1 && pl.fits; ++k) {
        const int lo = k < K ? 0 : k - K + 1, hi = k < K ? k : K - 1, n = hi - lo + 1;
        u64 psum = 0;
        for (int i = lo; i <= hi; ++i) psum += C::RR_P[k - i];
        u64 group[3] = {0, 0, MASK * psum}; // (psum < K * 2^LB: no overflow for any LB <= 30)
        const bool use[3] = {true, kind == FPR_KIND_MUL_ADD, true};
        if (limb * limb > TOP / (u64)n) pl.fits = false; // n * limb^2 alone does not fit
        else group[0] = group[1] = (u64)n * limb * limb;
        u64 acc = carry, hi_part = carry >> LB, lo_part = carry & MASK, spill = 0; // column total = hi_part * 2^LB + lo_part
        for (int g = 0; g < 3 && pl.fits; ++g) {
            if (!use[g]) continue;
            if (group[g] > TOP - acc) { // adding the group could reach 2^64
                pl.flush[k] |= (unsigned char)(1 << g);
                ++pl.flushes;
                spill += acc >> LB;
                acc = MASK;
                if (group[g] > TOP - acc) pl.fits = false;
            }
            acc += group[g];
            if (acc > pl.peak[k]) pl.peak[k] = acc;
            lo_part += group[g] & MASK;
            hi_part += (group[g] >> LB) + (lo_part >> LB);
            lo_part &= MASK;
        }
        if (spill > pl.spill_peak) pl.spill_peak = spill;
        carry = hi_part;
    }
    return pl;
}

template <class C> struct FpR {
    static constexpr int K = C::RR_K, LB = C::RR_LB;
    static constexpr int N = K; // words per element in memory
    static constexpr bool EXT = false;
    static constexpr bool LAZY = true;
    static constexpr u32 MASK = (1u << LB) - 1;
    // A 64-bit column accumulator holds a carry-in (< 2^36) and the column's products of two LB-bit limbs. 29-bit limbs never
    // come near its end (a fused column has 3 K = 27 products); with 30-bit limbs -- BLS12-381 Fq as 13 x 30 bits, 2 K^2 + K =
    // 351 multiply-adds per product instead of the 406 of 14 x 28 -- sixteen 60-bit products overflow, so such a column is
    // FLUSHED between its product groups: the accumulator's upper part is moved aside (one 64-bit shift, one mask) and joined
    // again when the column is done (tools/ubench_limbs.hip, profiles/r04_ubench_limbs.txt: 1960 against 2183 cycles, -10 %).
    // Where a product flushes is the exact plan (fpr_column_plan above) and nothing else: for 13 x 30 bits a plain product or
    // squaring flushes in columns 10..14 only, the fused product 18 times; the 29-bit fields' plans hold no flush at all.
    // The plans are for NORMALISED limbs (< 2^LB). Wider ("lazy") limbs reach a product in one place today, and only where nothing
    // flushes: the register DIT butterfly of the Fr NTT (fr_impl.h ntt_butterfly) multiplies a subl<3> / limb-wise sum (limbs
    // < 2^31) by a normalised twiddle, a plain product of a 9 x 29 field: K 2^31 2^LB + K 2^(2 LB) = 9 2^60 + 9 2^58 < 2^64 in any
    // order of the groups. (LAZY_LIMBS below, the switch of the group law's carry-free subtractions, is false for all four fields.)
    static constexpr int COLS = 2 * K - 1;
    typedef FprColumnPlan<COLS> Plan;
    static constexpr Plan PLAN_MUL = fpr_column_plan<C>(FPR_KIND_MUL, MASK);
    static constexpr Plan PLAN_SQR = fpr_column_plan<C>(FPR_KIND_SQR, MASK);
    static constexpr Plan PLAN_MUL_ADD = fpr_column_plan<C>(FPR_KIND_MUL_ADD, MASK);
    // a plan exists, so by its construction no column passes 2^64 - 1; the spill word collects at most two accumulators' upper parts
    static_assert(PLAN_MUL.fits && PLAN_SQR.fits && PLAN_MUL_ADD.fits, "a product group alone overflows the column accumulator");
    static_assert(PLAN_MUL.spill_peak < ((u64)1 << 40) && PLAN_SQR.spill_peak < ((u64)1 << 40) && PLAN_MUL_ADD.spill_peak < ((u64)1 << 40),
                  "spill word overflow");
    // "this field's products flush": the one rule that sends mul / sqr / mul_add and their single-chain codings (mul_t below) to
    // the column walker, and what mg_fpr_column_plan reports. A field that does not flush keeps the interleaved bodies.
    static constexpr bool FLUSHES = PLAN_MUL.flushes != 0;
    static_assert((PLAN_SQR.flushes != 0) == FLUSHES && (PLAN_MUL_ADD.flushes != 0) == FLUSHES, "the three plans of a field must flush together");
    // bound bookkeeping consumed by ec_dev.h's Bv<> wrapper (values are "< B*p")
    static constexpr int BM = 2;            // a product is < 2p ...
    static constexpr int LIM = C::RR_LIM;   // ... whenever the operand bounds multiply to <= LIM
    static constexpr int MULK = 1;
    static constexpr int MAXM = C::RR_MAXM; // largest tabulated multiple of p
    static constexpr int BX = 8, BY = 4;    // invariants of stored XYZZ X and Y coordinates
    static constexpr int BRED = 2;          // reduce<>() output bound
    typedef Fp<C> Std;
    u32 v[K];

    static MG_DEV FpR zero() {
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = 0;
        return r;
    }
    static MG_DEV FpR one() {
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = C::RR_ONE[i];
        return r;
    }
    MG_DEV bool is_zero_exact() const { // the all-zero representative (used as the infinity marker)
        u32 x = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) x |= v[i];
        return x == 0;
    }
    // value == 0 (mod p), given value < B*p : value is one of 0, p, ..., (B-1)p
    template <int B> MG_DEV bool is_zero_mod() const {
        static_assert(B - 1 <= C::RR_MAXM, "multiple table too short");
        bool hit = false;
#pragma unroll
        for (int k = 0; k < B; ++k) {
            if (v[0] == C::RR_MULT[k][0]) { // cheap pre-filter on the low limb; the full compare is rare
                u32 d = 0;
#pragma unroll
                for (int i = 1; i < K; ++i) d |= v[i] ^ C::RR_MULT[k][i];
                hit |= (d == 0);
            }
        }
        return hit;
    }

    // ---- linear operations: limb-wise in signed 32-bit, then one carry-normalisation pass
    static MG_DEV FpR normalize(const int (&t)[K]) {
        FpR r;
        int c = 0;
#pragma unroll
        for (int i = 0; i < K - 1; ++i) {
            const int s = t[i] + c;
            c = s >> LB; // arithmetic shift: borrows propagate as -1
            r.v[i] = (u32)s & MASK;
        }
        r.v[K - 1] = (u32)(t[K - 1] + c); // value >= 0 and < 2^(LB*K): top limb needs no mask
        return r;
    }
    static MG_DEV FpR add(const FpR &a, const FpR &b) {
        int t[K];
#pragma unroll
        for (int i = 0; i < K; ++i) t[i] = (int)(a.v[i] + b.v[i]);
        return normalize(t);
    }
    static MG_DEV FpR dbl(const FpR &a) { return add(a, a); }
    // a + M*p - b   (requires b < M*p)
    template <int M> static MG_DEV FpR sub(const FpR &a, const FpR &b) {
        static_assert(M <= C::RR_MAXM, "multiple table too short");
        int t[K];
#pragma unroll
        for (int i = 0; i < K; ++i) t[i] = (int)a.v[i] + (int)C::RR_MULT[M][i] - (int)b.v[i];
        return normalize(t);
    }
    // a + M*p - b - 2c   (requires b + 2c < M*p)
    template <int M> static MG_DEV FpR sub2(const FpR &a, const FpR &b, const FpR &c) {
        static_assert(M <= C::RR_MAXM, "multiple table too short");
        if constexpr (LB >= 30) { // a + Mp - b - 2c leaves the 32-bit range limb-wise (-3 * 2^30): carry every limb in 64 bits
            FpR r;
            long long cy = 0;
#pragma unroll
            for (int i = 0; i < K - 1; ++i) {
                const long long sv = (long long)a.v[i] + (long long)C::RR_MULT[M][i] - (long long)b.v[i] - 2 * (long long)c.v[i] + cy;
                cy = sv >> LB;
                r.v[i] = (u32)sv & MASK;
            }
            r.v[K - 1] = (u32)((long long)a.v[K - 1] + (long long)C::RR_MULT[M][K - 1] - (long long)b.v[K - 1] - 2 * (long long)c.v[K - 1] + cy);
            return r;
        } else {
            int t[K];
#pragma unroll
            for (int i = 0; i < K; ++i) t[i] = (int)a.v[i] + (int)C::RR_MULT[M][i] - (int)b.v[i] - 2 * (int)c.v[i];
            return normalize(t);
        }
    }
    // sub2 with every limb in signed 32 bits at LB = 30 too. REQUIRES normalised limbs (< 2^LB) in a, b and c.
    // The plain t_i = a_i + (Mp)_i - b_i - 2 c_i of the narrower fields reaches -3 (2^30 - 1) < -2^31 at LB = 30; what is too wide
    // is the 31-bit term 2 c_i, so bit LB-1 of c_i -- worth 2^LB once doubled -- is subtracted one limb higher:
    //   t_i = a_i + (Mp)_i - b_i - 2 (c_i mod 2^(LB-1)) - (c_(i-1) >> (LB-1))   in [-2^31 + 2, 2^31 - 2],
    // normalize()'s carry in [-2, 1] (floor((-2^31 + 2 - 2) / 2^30) = -2, floor((2^31 - 2 + 1) / 2^30) = 1), and t_i + carry in
    // [-2^31, 2^31 - 1]: exact in int32. The top limb is neither split nor masked (arithmetic mod 2^32, as everywhere).
    // Called by the G1 mixed addition alone (ec_dev.h madd_finish: X3 = R^2 + 6p - PPP - 2Q, three product outputs). The generic
    // group operations keep sub2: inside the Fp2 operations of BLS12-381 G2 this form gave wrong column sums
    // (tests/test_gpu_qap_columns.py) for a reason that is not established -- an open question recorded in
    // profiles/fpr_column_plan_ab.txt; do not widen its use before that is answered. MG_SUB2_64 makes it sub2 again (A/B builds).
    template <int M> static MG_DEV FpR sub2n(const FpR &a, const FpR &b, const FpR &c) {
        static_assert(M <= C::RR_MAXM, "multiple table too short");
        static_assert(LB <= 30, "sub2n: the limb-wise differences must fit signed 32 bits");
#ifdef MG_SUB2_64
        return sub2<M>(a, b, c);
#else
        if constexpr (LB >= 30) {
            int t[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const u32 low = i < K - 1 ? (c.v[i] & (MASK >> 1)) : c.v[i];
                const u32 high = i > 0 ? (c.v[i - 1] >> (LB - 1)) : 0u;
                t[i] = (int)a.v[i] + (int)C::RR_MULT[M][i] - (int)b.v[i] - (int)(2 * low + high);
            }
            return normalize(t);
        } else {
            return sub2<M>(a, b, c);
        }
#endif
    }
    template <int M> static MG_DEV FpR neg(const FpR &a) { return sub<M>(zero(), a); }

    // ---- carry-free subtraction: a + M*p - b with NO normalisation pass. M*p is taken in the redundant limb form
    //   q_0 = m_0 + 2^LB,  q_i = m_i + 2^LB - 1 (0 < i < K-1),  q_{K-1} = m_{K-1} - 1      (same value: each limb lends one
    // unit of 2^LB to the limb below), so that q_i - b_i >= 0 for every NORMALISED b (limbs < 2^LB, and b < (M-1)*p keeps
    // the top limb non-negative: m_{K-1}(M) - 1 >= m_{K-1}(M-1) + p_top - 2 >= b_top). The result's limbs are < 3 * 2^LB
    // ("lazy limbs"); it is a legal multiplication operand wherever the column accumulators have the room, which saves the
    // 3-instructions-per-limb carry pass of `sub`. Two users with two bounds: the NTT butterfly (ONE lazy operand of a plain
    // product, see the plans above) and the mixed addition of ec_dev.h, which wants lazy operands on both sides of a fused
    // product and asks LAZY_LIMBS first.
    static constexpr u32 multb(int M, int i) {
        return i == 0 ? C::RR_MULT[M][0] + (1u << LB) : (i < K - 1 ? C::RR_MULT[M][i] + MASK : C::RR_MULT[M][K - 1] - 1u);
    }
    // worst column of a fused product with lazy operands: K * (3*3 + 3*1 + 1) * 2^(2 LB) must stay below 2^64
    // (true for 14 x 28, FALSE for 9 x 29 -- 117 * 2^58 -- and 13 x 30: no shipped field takes the group law's lazy path, and the
    // static_assert below binds only a future layout that does)
    static constexpr bool LAZY_LIMBS = (double)K * 13.0 * (double)(1ull << LB) * (double)(1ull << LB) < 18446744073709551616.0;
    // checked, not only stated: with limbs < 3 * 2^LB the plan of a fused product must exist and hold no flush
    static_assert(!LAZY_LIMBS || (fpr_column_plan<C>(FPR_KIND_MUL_ADD, 3 * ((u64)1 << LB)).fits &&
                                  fpr_column_plan<C>(FPR_KIND_MUL_ADD, 3 * ((u64)1 << LB)).flushes == 0),
                  "lazy limbs need columns that never flush");
    template <int M> static MG_DEV FpR subl(const FpR &a, const FpR &b) { // a may itself have lazy limbs only if a is normalised: see call sites
        static_assert(M <= C::RR_MAXM, "multiple table too short");
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = a.v[i] + multb(M, i) - b.v[i];
        return r;
    }
    template <int M> static MG_DEV FpR negl(const FpR &b) { return subl<M>(zero(), b); }
    static MG_DEV FpR normalize_u(const FpR &a) { // lazy limbs (non-negative) -> normalised
        FpR r;
        u32 c = 0;
#pragma unroll
        for (int i = 0; i < K - 1; ++i) {
            const u32 t = a.v[i] + c;
            c = t >> LB;
            r.v[i] = t & MASK;
        }
        r.v[K - 1] = a.v[K - 1] + c;
        return r;
    }
    // ---- fused almost-Montgomery product (a*b + c*d) * R'^-1 with ONE reduction: two double-width products share the
    // column accumulators and the m*p pass -- 3 K^2 + K multiply-adds instead of 4 K^2 + 2 K. Value < 2p whenever
    // Ba*Bb + Bc*Bd <= LIM; limbs of the operands may be lazy when LAZY_LIMBS (column bound above).
    static MG_DEV FpR mul_add(const FpR &a, const FpR &b, const FpR &c, const FpR &d) {
        if constexpr (FLUSHES) return product<FPR_KIND_MUL_ADD, false>(a, b, c, d);
        u64 acc = 0;
        u32 m[K];
        FpR t;
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int i = 0; i < k; ++i) {
                acc += (u64)a.v[i] * b.v[k - i];
                acc += (u64)c.v[i] * d.v[k - i];
                acc += (u64)m[i] * C::RR_P[k - i];
            }
            acc += (u64)a.v[k] * b.v[0];
            acc += (u64)c.v[k] * d.v[0];
            m[k] = ((u32)acc * C::RR_INV) & MASK;
            acc += (u64)m[k] * C::RR_P[0];
            acc >>= LB;
        }
#pragma unroll
        for (int k = K; k < 2 * K - 1; ++k) {
#pragma unroll
            for (int i = k - K + 1; i < K; ++i) {
                acc += (u64)a.v[i] * b.v[k - i];
                acc += (u64)c.v[i] * d.v[k - i];
                acc += (u64)m[i] * C::RR_P[k - i];
            }
            t.v[k - K] = (u32)acc & MASK;
            acc >>= LB;
        }
        t.v[K - 1] = (u32)acc;
        return t;
    }
    // ---- the column walker, the one body of all three products of a field that flushes (its plain and its single-chain coding):
    // the products of a column are added group by group -- a*b, then c*d, then m*p -- and the accumulator is flushed before a
    // group exactly where the plan says it would not fit. It is written for any plan; with none of the flushes it is the grouped
    // twin of the interleaved bodies, which the raw-limb tests could compare it with the day the 29-bit fields take it.
    // (the first group of a column never needs one: carry-in + n * limb^2 < 2^64 for every plan that exists, asserted here)
    static constexpr bool plan_flushes_first_group(const Plan &p) {
        for (int k = 0; k < COLS; ++k)
            if (p.flush[k] & FPR_FLUSH_AB) return true;
        return false;
    }
    static_assert(!plan_flushes_first_group(PLAN_MUL) && !plan_flushes_first_group(PLAN_SQR) && !plan_flushes_first_group(PLAN_MUL_ADD),
                  "flush before the first group of a column");
    static constexpr bool flush_before(int kind, int k, int group) {
        return ((kind == FPR_KIND_MUL ? PLAN_MUL : (kind == FPR_KIND_SQR ? PLAN_SQR : PLAN_MUL_ADD)).flush[k] & group) != 0;
    }
    static MG_DEV void flush(u64 &acc, u64 &spill) {
        spill += acc >> LB;
        acc &= (u64)MASK;
    }
    // One multiply-add of a column. CH = true keeps the column's multiply-adds in ONE dependent chain, in plain C. Left alone the
    // compiler's reassociation orders the terms of a sum by depth; the running accumulator is the deepest, so the a*b products of
    // a column are summed from zero and joined to it by a v_lshl_add_u64 (4.97 issue cycles, more than a multiply). The annotation
    // is an identity the optimiser does not look through and the code generator drops: every partial sum stays where it is
    // written, and no instruction is spent on it. (An assumption about the sum does the same only until the optimiser can prove
    // it from the operands' ranges -- the first four or so terms behind a flush -- and then goes, the reordering with it.)
    // The asm links of the narrower fields (mad_chain_*) buy the same chain with an s_nop behind every statement: the compiler
    // takes every register an asm statement writes, vcc included, for a destination whose next reader or writer must wait one
    // state, so neither a scalar-pair output in place of the vcc clobber nor longer blocks per column get rid of it
    // (profiles/fpr_chain_padding_ab.txt).
    template <bool CH> static MG_DEV void mad_link(u64 &acc, u32 x, u32 y) {
        const u64 prod = (u64)x * y;
        acc += prod;
        if constexpr (CH) acc = __builtin_annotation(acc, "chain");
    }
    // KIND = FPR_KIND_MUL: a*b (c, d unused), FPR_KIND_SQR: a^2 (b, c, d unused), FPR_KIND_MUL_ADD: a*b + c*d; all times R'^-1 mod p.
    // A squaring's a*b group is its cross products a_i a_j (i < j) once, against the doubled operand, and the squares a_i^2.
    template <int KIND, bool CH> static MG_DEV FpR product(const FpR &a, const FpR &b, const FpR &c, const FpR &d) {
        u64 acc = 0;
        u32 m[K], a2[K];
        FpR t;
        if constexpr (KIND == FPR_KIND_SQR) {
#pragma unroll
            for (int i = 0; i < K; ++i) a2[i] = a.v[i] << 1; // (< 2^31: a doubled cross product counts as two)
        }
#pragma unroll
        for (int k = 0; k < COLS; ++k) {
            const int lo = k < K ? 0 : k - K + 1, hi = k < K ? k : K - 1;
            u64 spill = 0;
#pragma unroll
            for (int i = lo; i <= hi; ++i) {
                const int j = k - i;
                if constexpr (KIND == FPR_KIND_SQR) {
                    if (i < j) mad_link<CH>(acc, a2[i], a.v[j]);
                    if (i == j) mad_link<CH>(acc, a.v[i], a.v[i]);
                } else {
                    mad_link<CH>(acc, a.v[i], b.v[j]);
                }
            }
            if constexpr (KIND == FPR_KIND_MUL_ADD) {
                if (flush_before(KIND, k, FPR_FLUSH_CD)) flush(acc, spill);
#pragma unroll
                for (int i = lo; i <= hi; ++i) mad_link<CH>(acc, c.v[i], d.v[k - i]);
            }
            if (flush_before(KIND, k, FPR_FLUSH_MP)) flush(acc, spill);
#pragma unroll
            for (int i = lo; i <= hi; ++i)
                if (!(k < K && i == k)) mad_link<CH>(acc, m[i], C::RR_P[k - i]);
            if (k < K) {
                m[k] = ((u32)acc * C::RR_INV) & MASK;
                mad_link<CH>(acc, m[k], C::RR_P[0]);
            } else {
                t.v[k - K] = (u32)acc & MASK;
            }
            acc >>= LB;
            acc += spill;
        }
        t.v[K - 1] = (u32)acc;
        return t;
    }
    // value < A*p (A <= 16)  ->  same residue, < 2p: subtract floor-estimate(value / p) * p, the
    // quotient estimated from the top limb (never too large, at most one too small)
    // (valid for any A with A*p < 2^(LB*K): with T the top limb and D = p_top + 1, the estimate q' = floor(T*RECIP/2^32) is
    // never above value/p and lies less than 1/8 + (A + 1)/p_top < 1 below T/D <= value/p, p_top >= 2^16 for all four fields)
    template <int A> static MG_DEV FpR reduce(const FpR &a) {
        static_assert(A <= 64 && A <= C::RR_LIM, "reduce: A*p must fit the representation");
        const u32 q = (u32)(((u64)a.v[K - 1] * C::RR_RECIP) >> 32);
        FpR r;
        long long c = 0;
#pragma unroll
        for (int i = 0; i < K - 1; ++i) {
            const long long s = (long long)a.v[i] - (long long)((u64)q * C::RR_P[i]) + c;
            c = s >> LB;
            r.v[i] = (u32)s & MASK;
        }
        r.v[K - 1] = (u32)((long long)a.v[K - 1] - (long long)((u64)q * C::RR_P[K - 1]) + c);
        return r;
    }

    template <int A, int B> static MG_DEV FpR mulb(const FpR &a, const FpR &b) { return mul(a, b); }
    // ---- almost-Montgomery product: a*b*R'^-1 mod p, result < 2p (see header for the input bounds)
    static MG_DEV FpR mul(const FpR &a, const FpR &b) {
        if constexpr (FLUSHES) return product<FPR_KIND_MUL, false>(a, b, a, b);
        u64 acc = 0;
        u32 m[K];
        FpR t;
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int i = 0; i < k; ++i) {
                acc += (u64)a.v[i] * b.v[k - i];
                acc += (u64)m[i] * C::RR_P[k - i];
            }
            acc += (u64)a.v[k] * b.v[0];
            m[k] = ((u32)acc * C::RR_INV) & MASK;
            acc += (u64)m[k] * C::RR_P[0];
            acc >>= LB;
        }
#pragma unroll
        for (int k = K; k < 2 * K - 1; ++k) {
#pragma unroll
            for (int i = k - K + 1; i < K; ++i) {
                acc += (u64)a.v[i] * b.v[k - i];
                acc += (u64)m[i] * C::RR_P[k - i];
            }
            t.v[k - K] = (u32)acc & MASK;
            acc >>= LB;
        }
        t.v[K - 1] = (u32)acc;
        return t;
    }
    // single-chain codings of mul / sqr / mul_add, for the accumulate kernel (CH = true). The field that flushes (13 x 30 bits)
    // has the column walker itself with its multiply-adds pinned in C (mad_link<true>): no asm statement, so no padding;
    // MG_CHAIN_FLUSHED=0 gives it the compiler's two-chain coding again (A/B builds). The 29-bit fields code the chain as asm links
    // (mad_chain_*, several links per statement): the three bodies below, with the a*b, c*d and m*p terms interleaved.
    static constexpr bool CHAIN_FLUSHED = MG_CHAIN_FLUSHED != 0;
    template <bool CH> static MG_DEV FpR mul_t(const FpR &a, const FpR &b) {
        if constexpr (!CH) return mul(a, b);
        if constexpr (FLUSHES) return product<FPR_KIND_MUL, CHAIN_FLUSHED>(a, b, a, b);
        u64 acc = 0;
        u32 m[K];
        FpR t;
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int i = 0; i + 1 < k; i += 2)
                mad_chain_pair2(acc, a.v[i], b.v[k - i], m[i], C::RR_P[k - i], a.v[i + 1], b.v[k - i - 1], m[i + 1], C::RR_P[k - i - 1]);
            if (k & 1) mad_chain_pair(acc, a.v[k - 1], b.v[1], m[k - 1], C::RR_P[1]);
            mad_chain_vv(acc, a.v[k], b.v[0]);
            m[k] = ((u32)acc * C::RR_INV) & MASK;
            mad_chain_vs(acc, m[k], C::RR_P[0]);
            acc >>= LB;
        }
#pragma unroll
        for (int k = K; k < 2 * K - 1; ++k) {
            const int lo = k - K + 1, n = K - lo; // pairs i = lo .. K-1
#pragma unroll
            for (int q = 0; q + 1 < n; q += 2) {
                const int i = lo + q;
                mad_chain_pair2(acc, a.v[i], b.v[k - i], m[i], C::RR_P[k - i], a.v[i + 1], b.v[k - i - 1], m[i + 1], C::RR_P[k - i - 1]);
            }
            if (n & 1) mad_chain_pair(acc, a.v[K - 1], b.v[k - K + 1], m[K - 1], C::RR_P[k - K + 1]);
            t.v[k - K] = (u32)acc & MASK;
            acc >>= LB;
        }
        t.v[K - 1] = (u32)acc;
        return t;
    }
    template <bool CH> static MG_DEV FpR sqr_t(const FpR &a) {
        if constexpr (!CH) return sqr(a);
        if constexpr (FLUSHES) return product<FPR_KIND_SQR, CHAIN_FLUSHED>(a, a, a, a);
        u64 acc = 0;
        u32 m[K], a2[K];
        FpR t;
#pragma unroll
        for (int i = 0; i < K; ++i) a2[i] = a.v[i] << 1;
#pragma unroll
        for (int k = 0; k < 2 * K - 1; ++k) {
            // cross products a_i a_j (i < j, i + j = k) against the doubled operand, two per asm block
            const int ilo = k < K ? 0 : k - K + 1, ihi = (k - 1) / 2; // i = ilo .. ihi with i < k - i
#pragma unroll
            for (int i = ilo; i + 1 <= ihi; i += 2) mad_chain_vv2(acc, a2[i], a.v[k - i], a2[i + 1], a.v[k - i - 1]);
            if (k >= 1 && ((ihi - ilo + 1) & 1) && ihi >= ilo) mad_chain_vv(acc, a2[ihi], a.v[k - ihi]);
            if (!(k & 1)) mad_chain_vv(acc, a.v[k / 2], a.v[k / 2]);
            // the m_i p_{k-i} terms already known, two per block
            const int mlo = k < K ? 0 : k - K + 1, mhi = k < K ? k - 1 : K - 1;
#pragma unroll
            for (int i = mlo; i + 1 <= mhi; i += 2) mad_chain_vs2(acc, m[i], C::RR_P[k - i], m[i + 1], C::RR_P[k - i - 1]);
            if (mhi >= mlo && ((mhi - mlo + 1) & 1)) mad_chain_vs(acc, m[mhi], C::RR_P[k - mhi]);
            if (k < K) {
                m[k] = ((u32)acc * C::RR_INV) & MASK;
                mad_chain_vs(acc, m[k], C::RR_P[0]);
            } else {
                t.v[k - K] = (u32)acc & MASK;
            }
            acc >>= LB;
        }
        t.v[K - 1] = (u32)acc;
        return t;
    }
    template <bool CH> static MG_DEV FpR mul_add_t(const FpR &a, const FpR &b, const FpR &c, const FpR &d) {
        if constexpr (!CH) return mul_add(a, b, c, d);
        if constexpr (FLUSHES) return product<FPR_KIND_MUL_ADD, CHAIN_FLUSHED>(a, b, c, d);
        u64 acc = 0;
        u32 m[K];
        FpR t;
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int i = 0; i + 1 < k; i += 2)
                mad_chain_triple2(acc, a.v[i], b.v[k - i], c.v[i], d.v[k - i], m[i], C::RR_P[k - i], a.v[i + 1], b.v[k - i - 1],
                                  c.v[i + 1], d.v[k - i - 1], m[i + 1], C::RR_P[k - i - 1]);
            if (k & 1) mad_chain_triple(acc, a.v[k - 1], b.v[1], c.v[k - 1], d.v[1], m[k - 1], C::RR_P[1]);
            mad_chain_vv(acc, a.v[k], b.v[0]);
            mad_chain_vv(acc, c.v[k], d.v[0]);
            m[k] = ((u32)acc * C::RR_INV) & MASK;
            mad_chain_vs(acc, m[k], C::RR_P[0]);
            acc >>= LB;
        }
#pragma unroll
        for (int k = K; k < 2 * K - 1; ++k) {
            const int lo = k - K + 1, n = K - lo;
#pragma unroll
            for (int q = 0; q + 1 < n; q += 2) {
                const int i = lo + q;
                mad_chain_triple2(acc, a.v[i], b.v[k - i], c.v[i], d.v[k - i], m[i], C::RR_P[k - i], a.v[i + 1], b.v[k - i - 1],
                                  c.v[i + 1], d.v[k - i - 1], m[i + 1], C::RR_P[k - i - 1]);
            }
            if (n & 1) mad_chain_triple(acc, a.v[K - 1], b.v[k - K + 1], c.v[K - 1], d.v[k - K + 1], m[K - 1], C::RR_P[k - K + 1]);
            t.v[k - K] = (u32)acc & MASK;
            acc >>= LB;
        }
        t.v[K - 1] = (u32)acc;
        return t;
    }
    template <int A> static MG_DEV FpR sqrb(const FpR &a) { return sqr(a); }
    static MG_DEV FpR sqr(const FpR &a) {
        if constexpr (FLUSHES) return product<FPR_KIND_SQR, false>(a, a, a, a);
        u64 acc = 0;
        u32 m[K], a2[K];
        FpR t;
#pragma unroll
        for (int i = 0; i < K; ++i) a2[i] = a.v[i] << 1;
#pragma unroll
        for (int k = 0; k < 2 * K - 1; ++k) {
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int j = k - i;
                if (j < 0 || j >= K) continue;
                if (i < j) acc += (u64)a2[i] * a.v[j];
                if (i == j) acc += (u64)a.v[i] * a.v[i];
                if (k < K) {
                    if (i < k) acc += (u64)m[i] * C::RR_P[k - i];
                } else {
                    acc += (u64)m[i] * C::RR_P[k - i];
                }
            }
            if (k < K) {
                m[k] = ((u32)acc * C::RR_INV) & MASK;
                acc += (u64)m[k] * C::RR_P[0];
            } else {
                t.v[k - K] = (u32)acc & MASK;
            }
            acc >>= LB;
        }
        t.v[K - 1] = (u32)acc;
        return t;
    }
    static __device__ __noinline__ FpR inv(const FpR &a) { // a^(p-2); slow, one-off use only
        FpR acc = one();
        for (int i = 32 * C::N - 1; i >= 0; --i) {
            acc = sqr(acc);
            u32 w = 0;
#pragma unroll
            for (int j = 0; j < C::N; ++j)
                if (j == (i >> 5)) w = C::PM2[j];
            if ((w >> (i & 31)) & 1) acc = mul(acc, a);
        }
        return acc;
    }

    // ---- the K limbs of LB bits repacked as N words of 32 bits and back, no arithmetic: a NORMALISED value below 2^(32 N)
    MG_DEV Std to_words() const {
        Std r;
#pragma unroll
        for (int w = 0; w < C::N; ++w) {
            u64 x = 0;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const int lo = i * LB - w * 32; // position of limb i relative to word w
                if (lo > -LB && lo < 32) x |= lo >= 0 ? ((u64)v[i] << lo) : ((u64)v[i] >> (-lo));
            }
            r.v[w] = (u32)x;
        }
        return r;
    }
    // limb i = bits [i LB - SH, (i + 1) LB - SH) of the N words: the limbs of (value << SH), which must stay below 2^(LB K)
    template <int SH = 0> static MG_DEV FpR from_words(const u32 (&t)[C::N]) {
        static_assert(SH >= 0 && SH < LB, "only limb 0 may start below bit 0");
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int bit = i * LB - SH;
            if (bit < 0) { // limb 0: its low SH bits are zero
                r.v[i] = (t[0] << (-bit)) & MASK;
            } else {
                const int w = bit >> 5, o = bit & 31;
                u64 x = w < C::N ? t[w] : 0;
                if (w + 1 < C::N) x |= (u64)t[w + 1] << 32;
                r.v[i] = (u32)(x >> o) & MASK;
            }
        }
        return r;
    }
    // a value < 2p with normalised limbs -> fully reduced: one conditional subtraction of p
    MG_DEV FpR sub_p_if_ge() const {
        int t[K];
#pragma unroll
        for (int i = 0; i < K; ++i) t[i] = (int)v[i] - (int)C::RR_P[i];
        int cy = 0;
        u32 d[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int s = t[i] + cy;
            cy = s >> LB;
            d[i] = (u32)s & MASK;
        }
        const bool ge = cy == 0; // no final borrow: value >= p
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = ge ? d[i] : v[i];
        return r;
    }
    // ---- cheap conversions for fields with R'/R = 2^(LB*K - 32N) small (Fr: 2^261 / 2^256 = 2^5): the arkworks Montgomery
    // form a*R is turned into a*R' by SHIFTING the integer left while repacking its limbs (value < 2^5 p) and one reduce --
    // no multiplication; and a*R' becomes the canonical integer a by one almost-Montgomery product with the integer 1.
    static MG_DEV FpR from_std_shift(const Std &s) {
        constexpr int SH = LB * K - 32 * C::N; // R' = 2^SH * R
        static_assert(SH >= 0 && SH < 8 && (1 << SH) <= 64 && (1 << SH) <= C::RR_LIM, "shift conversion needs a small R'/R");
        return reduce<(1 << SH)>(from_words<SH>(s.v));
    }
    // value (< 4p, any representative) -> the canonical integer a, as 32-bit words (ark-ff into_repr)
    MG_DEV Std to_canonical() const {
        FpR one_plain = zero();
        one_plain.v[0] = 1;
        return mul(*this, one_plain).canonical_words();
    }
    // a value < 2p with normalised limbs -> fully reduced, repacked into 32-bit words
    MG_DEV Std canonical_words() const { return sub_p_if_ge().to_words(); }
    // ---- conversions to / from the arkworks (32-bit limb, R = 2^(32N)) Montgomery form
    static MG_DEV FpR from_std(const Std &s) {
        Std c;
#pragma unroll
        for (int i = 0; i < C::N; ++i) c.v[i] = C::RR_TO[i];
        const Std t = Std::mul(s, c); // a*R * R' * R^-1 = a*R' mod p, canonical
        return from_words(t.v);
    }
    MG_DEV Std to_std() const {
        FpR c;
#pragma unroll
        for (int i = 0; i < K; ++i) c.v[i] = C::RR_FROM[i];
        return mul(*this, c).canonical_words(); // a*R' * R * R'^-1 = a*R mod p, in [0, 2p)
    }

    static MG_DEV FpR load(const u32 *p) {
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = p[i];
        return r;
    }
    MG_DEV void store(u32 *p) const {
#pragma unroll
        for (int i = 0; i < K; ++i) p[i] = v[i];
    }
    // 32 N-bit form of a NORMALISED value below 2^(32 N) (any lazily reduced value < 2p): the LB-bit limbs repacked into N
    // words, no arithmetic. What an NTT pass leaves in HBM for the next one: 32 B instead of 36 per element, and two adjacent
    // elements are one aligned 64 B sector where the 72 B of the limb form straddle two.
    MG_DEV void store_packed(u32 *p) const { to_words().store(p); }
    static MG_DEV FpR load_packed(const u32 *p) {
        u32 t[C::N];
#pragma unroll
        for (int w = 0; w < C::N; ++w) t[w] = p[w];
        return from_words(t);
    }
    // ---- memory format of AFFINE base coordinates (the records the accumulate kernels gather). A coordinate is < 2p with
    // normalised limbs, so it fits the 32 N-bit packed form: BN254 G1 = 2 x 32 B = ONE aligned 64 B sector per gathered point
    // where the 72 B limb form (96 B stride) touched two; the 18 v_alignbit/v_and of the unpacking are
    // 0.6 % of a mixed addition's instructions. MG_PACK_AFFINE: 0 = limb form everywhere (the round-1..5 layout), 1 (default) =
    // packed where the packed record is a whole number of 64 B sectors and smaller in sectors than the padded limb record
    // (BN254: 64 against 96 B, G2 128 against 160 B), 2 = BLS12-381 too (96 against 128 B: fewer bytes, the same two sectors).
#ifndef MG_PACK_AFFINE
#define MG_PACK_AFFINE 1
#endif
    static constexpr bool PACK_AFF = MG_PACK_AFFINE == 2 || (MG_PACK_AFFINE == 1 && C::N == 8);
    static constexpr int AFF_N = PACK_AFF ? C::N : K; // words per affine coordinate in memory
    static MG_DEV FpR load_aff(const u32 *p) {
        if constexpr (PACK_AFF) return load_packed(p);
        else return load(p);
    }
    MG_DEV void store_aff(u32 *p) const {
        if constexpr (PACK_AFF) store_packed(p);
        else store(p);
    }
    // limb i at p[i * stride]: LDS exchange areas keep one limb of all 64 lanes together (no bank conflicts)
    static MG_DEV FpR load_strided(const u32 *p, int stride) {
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = p[i * stride];
        return r;
    }
    MG_DEV void store_strided(u32 *p, int stride) const {
#pragma unroll
        for (int i = 0; i < K; ++i) p[i * stride] = v[i];
    }
    // LDS exchange format of the cooperative addition: quads of limbs, one 16-byte access per lane and quad
    // (quad q of lane l at word (q*64 + l)*4): a 9-limb element is 3 ds_*_b128 instead of 9 ds_*_b32
    static constexpr int XQ = (K + 3) / 4;         // quads per element
    static constexpr int XWORDS = XQ * 64 * 4;     // words of one exchange slot (64 lanes)
    MG_DEV void store_x(u32 *slot, int lane) const {
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            uint4 t;
            t.x = v[4 * q];
            t.y = 4 * q + 1 < K ? v[4 * q + 1] : 0u;
            t.z = 4 * q + 2 < K ? v[4 * q + 2] : 0u;
            t.w = 4 * q + 3 < K ? v[4 * q + 3] : 0u;
            *reinterpret_cast<uint4 *>(slot + ((size_t)q * 64 + lane) * 4) = t;
        }
    }
    static MG_DEV FpR load_x(const u32 *slot, int lane) {
        FpR r;
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const uint4 t = *reinterpret_cast<const uint4 *>(slot + ((size_t)q * 64 + lane) * 4);
            r.v[4 * q] = t.x;
            if (4 * q + 1 < K) r.v[4 * q + 1] = t.y;
            if (4 * q + 2 < K) r.v[4 * q + 2] = t.z;
            if (4 * q + 3 < K) r.v[4 * q + 3] = t.w;
        }
        return r;
    }
    static MG_DEV FpR select(bool c, const FpR &a, const FpR &b) {
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = c ? a.v[i] : b.v[i];
        return r;
    }
    static MG_DEV FpR shfl(const FpR &a, int src_lane) {
        FpR r;
#pragma unroll
        for (int i = 0; i < K; ++i) r.v[i] = __shfl(a.v[i], src_lane, 64);
        return r;
    }
};

// Fp2 = FpR[u]/(u^2+1), components lazily reduced. Products are schoolbook (4 base products): the sum
// a0+a1 a Karatsuba product needs would double the operand bounds and overrun BN254's 7 bits of
// Montgomery headroom. Component bounds: product < 4p (c0 = a0 b0 + 2p - a1 b1, c1 = a0 b1 + a1 b0).
template <class C> struct Fp2R {
    typedef FpR<C> B;
    static constexpr int N = 2 * B::N;
    static constexpr bool EXT = true;
    static constexpr bool LAZY = true;
    static constexpr int BM = 4, LIM = B::LIM, MULK = 1, MAXM = B::MAXM, BX = 4, BY = 4, BRED = 2;
    typedef Fp2<C> Std;
    B c0, c1;
    static MG_DEV Fp2R zero() { return Fp2R{B::zero(), B::zero()}; }
    static MG_DEV Fp2R one() { return Fp2R{B::one(), B::zero()}; }
    MG_DEV bool is_zero_exact() const { return c0.is_zero_exact() && c1.is_zero_exact(); }
    template <int A> MG_DEV bool is_zero_mod() const { return c0.template is_zero_mod<A>() && c1.template is_zero_mod<A>(); }
    static MG_DEV Fp2R add(const Fp2R &a, const Fp2R &b) { return Fp2R{B::add(a.c0, b.c0), B::add(a.c1, b.c1)}; }
    static MG_DEV Fp2R dbl(const Fp2R &a) { return add(a, a); }
    template <int M> static MG_DEV Fp2R sub(const Fp2R &a, const Fp2R &b) {
        return Fp2R{B::template sub<M>(a.c0, b.c0), B::template sub<M>(a.c1, b.c1)};
    }
    template <int M> static MG_DEV Fp2R sub2(const Fp2R &a, const Fp2R &b, const Fp2R &c) {
        return Fp2R{B::template sub2<M>(a.c0, b.c0, c.c0), B::template sub2<M>(a.c1, b.c1, c.c1)};
    }
    template <int M> static MG_DEV Fp2R neg(const Fp2R &a) { return Fp2R{B::template neg<M>(a.c0), B::template neg<M>(a.c1)}; }
    template <int A> static MG_DEV Fp2R reduce(const Fp2R &a) {
        return Fp2R{B::template reduce<A>(a.c0), B::template reduce<A>(a.c1)};
    }
    // (the base products are inlined for every field: profiles/history/code_comment_measurements.md has the calls they once were)
    static MG_DEV Fp2R mul(const Fp2R &a, const Fp2R &b) {
        const B v0 = B::mul(a.c0, b.c0), v1 = B::mul(a.c1, b.c1);
        const B x = B::mul(a.c0, b.c1), y = B::mul(a.c1, b.c0);
        return Fp2R{B::template sub<2>(v0, v1), B::add(x, y)};
    }
    // product of operands with component bounds A, Bb: c0 = a0 b0 + a1 (M p - b1) and c1 = a0 b1 + a1 b0 as TWO FUSED products
    // (FpR::mul_add: both double-width products of a component share the column accumulators and ONE Montgomery reduction) --
    // 6 K^2 + 2 K multiply-adds, the same as Karatsuba's three products (3 (2 K^2 + K)), but none of Karatsuba's linear work:
    // two operand sums, the sum v0 + v1, two subtractions and a reduce<6> (about 200 VALU instructions per product at K = 9)
    // become ONE negation. The G2 accumulate kernel issued 63 % non-multiply instructions with Karatsuba (34 % of the
    // multiply-add issue peak against 67 % for G1). Components of the result are < 2p. Needs (A Bb + A Bb) <= LIM; where the
    // bounds do not allow it, mulb_karatsuba below.
    template <int A, int Bb> static MG_DEV Fp2R mulb(const Fp2R &a, const Fp2R &b) {
        if constexpr (2L * A * Bb <= LIM && (A <= MAXM || Bb <= MAXM)) {
            if constexpr (Bb <= A || A > MAXM) { // negate the component with the smaller bound (the smaller multiple of p)
                const B nb1 = B::template neg<Bb>(b.c1);
                return Fp2R{B::mul_add(a.c0, b.c0, a.c1, nb1), B::mul_add(a.c0, b.c1, a.c1, b.c0)};
            } else {
                const B na1 = B::template neg<A>(a.c1);
                return Fp2R{B::mul_add(a.c0, b.c0, na1, b.c1), B::mul_add(a.c0, b.c1, a.c1, b.c0)};
            }
        } else {
            return mulb_karatsuba<A, Bb>(a, b);
        }
    }
    // (a0 + a1)(a0 - a1) and 2 a0 a1: two products where the operand sums fit the headroom (4 A^2 <= LIM), else a0^2 - a1^2 as
    // one fused product; either way one reduction per component and a result < 2p
    template <int A> static MG_DEV Fp2R sqrb(const Fp2R &a) {
        if constexpr (4L * A * A <= LIM && A <= MAXM) {
            const B s = B::add(a.c0, a.c1), d = B::template sub<A>(a.c0, a.c1);
            return Fp2R{B::mul(s, d), B::mul(B::dbl(a.c0), a.c1)};
        } else if constexpr (2L * A * A <= LIM && A <= MAXM) {
            return Fp2R{B::mul_add(a.c0, a.c0, a.c1, B::template neg<A>(a.c1)), B::mul(B::dbl(a.c0), a.c1)};
        } else {
            return sqr(a);
        }
    }
    // Where the headroom allows the operand sums (4 A Bb <= R'/p) Karatsuba -- 3 base products + one cheap reduction of c1 back
    // below 2p -- else the 4-product schoolbook form above. Either way the components of the result are < 4p.
    template <int A, int Bb> static MG_DEV Fp2R mulb_karatsuba(const Fp2R &a, const Fp2R &b) {
        if constexpr (4L * A * Bb <= LIM && 2 * A <= 16 && 2 * Bb <= 16) {
            const B v0 = B::mul(a.c0, b.c0), v1 = B::mul(a.c1, b.c1);
            const B s = B::mul(B::add(a.c0, a.c1), B::add(b.c0, b.c1));
            const B c1 = B::template reduce<6>(B::template sub<4>(s, B::add(v0, v1))); // s + 4p - v0 - v1 < 6p
            return Fp2R{B::template sub<2>(v0, v1), c1};
        } else {
            return mul(a, b);
        }
    }
    static MG_DEV Fp2R sqr(const Fp2R &a) {
        const B v0 = B::sqr(a.c0), v1 = B::sqr(a.c1), x = B::mul(a.c0, a.c1);
        return Fp2R{B::template sub<2>(v0, v1), B::dbl(x)};
    }
    static __device__ __noinline__ Fp2R inv(const Fp2R &a) { // one-off use only
        const B n = B::inv(B::add(B::sqr(a.c0), B::sqr(a.c1)));
        return Fp2R{B::mul(a.c0, n), B::template neg<2>(B::mul(a.c1, n))};
    }
    static MG_DEV Fp2R from_std(const Std &s) { return Fp2R{B::from_std(s.c0), B::from_std(s.c1)}; }
    MG_DEV Std to_std() const { return Std{c0.to_std(), c1.to_std()}; }
    static constexpr int XWORDS = 2 * B::XWORDS;
    MG_DEV void store_x(u32 *slot, int lane) const {
        c0.store_x(slot, lane);
        c1.store_x(slot + B::XWORDS, lane);
    }
    static MG_DEV Fp2R load_x(const u32 *slot, int lane) { return Fp2R{B::load_x(slot, lane), B::load_x(slot + B::XWORDS, lane)}; }
    static MG_DEV Fp2R load_strided(const u32 *p, int stride) {
        return Fp2R{B::load_strided(p, stride), B::load_strided(p + B::N * stride, stride)};
    }
    MG_DEV void store_strided(u32 *p, int stride) const {
        c0.store_strided(p, stride);
        c1.store_strided(p + B::N * stride, stride);
    }
    static constexpr int AFF_N = 2 * B::AFF_N;
    static MG_DEV Fp2R load_aff(const u32 *p) { return Fp2R{B::load_aff(p), B::load_aff(p + B::AFF_N)}; }
    MG_DEV void store_aff(u32 *p) const {
        c0.store_aff(p);
        c1.store_aff(p + B::AFF_N);
    }
    static MG_DEV Fp2R load(const u32 *p) { return Fp2R{B::load(p), B::load(p + B::N)}; }
    MG_DEV void store(u32 *p) const {
        c0.store(p);
        c1.store(p + B::N);
    }
    static MG_DEV Fp2R select(bool c, const Fp2R &a, const Fp2R &b) {
        return Fp2R{B::select(c, a.c0, b.c0), B::select(c, a.c1, b.c1)};
    }
    static MG_DEV Fp2R shfl(const Fp2R &a, int src_lane) { return Fp2R{B::shfl(a.c0, src_lane), B::shfl(a.c1, src_lane)}; }
};

} // namespace mg
