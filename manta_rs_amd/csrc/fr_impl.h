// Scalar-field kernels on gfx950: radix-2 NTT, CSR SpMV, QAP pointwise step. Templated on the Fr
// parameters; instantiated in fr_bn254.hip / fr_bls381.hip.
//
// Replaces: ark-poly ^0.3.0 Radix2EvaluationDomain::{fft,ifft,coset_fft,
// coset_ifft}_in_place and ark-groth16 ^0.3.0 R1CStoQAP::witness_map's evaluate_constraint /
// mul_polynomials_in_evaluation_domain / divide_by_vanishing_poly_on_coset (reached from
// manta-crypto/src/arkworks/groth16.rs:597). Conventions restated from SURVEY.md App. A.1/B.3:
// omega_D = omega_{2^s}^(2^(s - log D)); ifft scales by D^-1; coset shift g = Fr multiplicative
// generator; natural order in and out.
#pragma once
#include "fp_dev.h"
#include "tuning.h"
#include "fpr_dev.h"
#include "fr_host.h"
#include "params_gen.h"
#include <algorithm>
#include <type_traits>
#include <map>
#include <memory>
#include <mutex>

namespace mg {

// ---------------------------------------------------------------------------------------------------
// Reduced-radix scalar field (round 2). Inside the NTT / witness-map pipeline an Fr element is FpR<FrC>: 9 limbs of
// 29 bits, Montgomery radix R' = 2^261 = 2^5 R, lazily reduced (fpr_dev.h) -- the butterfly's product is 171 carry-free
// v_mad_u64_u32 instead of 136 multiply-adds + 136 carry additions, additions are limb-wise with one normalisation
// pass. Elements are 9 words (36 B) in HBM and in LDS. Conversions at the ends cost no multiplication going in (the
// arkworks form a*R becomes a*R' by a 5-bit shift folded into the limb repacking + one reduce, from_std_shift) and
// one product coming out (to_std / to_canonical). Tables (twiddles, scale tables) hold canonical values (< p).
//
// LDS-fused NTT pass: `ns` consecutive butterfly stages (global stages s0 .. s0+ns-1) of up to three
// vectors (blockIdx.y) in one launch. A workgroup owns the 2^ns elements that differ only in index bits
// [s0-1, s0-1+ns), for 2^cb adjacent values of the low bits; the tile lives in LDS as limb-major SoA
// (conflict-free ds_read_b32) and is read from / written to HBM exactly once per pass.
//   DIT (DIF = false): stages ascending, input bit-reversed -> output natural (Cooley-Tukey)
//   DIF (DIF = true) : stages descending, input natural -> output bit-reversed (Gentleman-Sande)
// Bounds (multiples of p; uniform per stage, tracked in `B`): tile values enter < 4p. DIT: t = b w < 2p, a' = a + t,
// b' = a + 2p - t, so B grows by 2 per stage (<= 4 + 5 + 2*9 = 27 over ten stages, within LIM = 70 / 169 for the only
// product, b w) and one reduce at the end of the pass brings everything below 2p. DIF: x = a + b doubles B, so x is
// reduced whenever 2B would exceed 8; y = (a + 9p - b) w < 2p. `post` (optional, last pass) multiplies element i by
// post[i] on the way out (n^-1 and coset powers, tabulated in the order the pass leaves the data in).
// The public transform (mg_ntt / mg_ntt_device: arkworks format in and out) folds its format conversions into its first and
// last pass instead of running them as kernels of their own (27 + 17 us of a 218 us 2^20 transform): with `in_std` the tile
// is gathered from the arkworks-format input at the bit-reversed index and converted on the way into LDS (times pre[j] for
// the forward coset transform); with `out_std` the finished tile is scaled (n^-1 of the plain inverse transform), converted
// back and written in the arkworks format. Both null inside the witness map, which stays in the work form throughout.
// the butterfly's product: the single-chain coding of fpr_dev.h (mad_chain_*: every multiply-add of a column in one dependent
// chain, no 64-bit joins) -- 112 instead of 131 VGPRs in the register kernel (four wavefronts per SIMD) and -10 % on the 2^20
// transform (profiles/r04_ntt_register_stages.txt; the stage-per-round-trip kernel: 82 -> 64 VGPRs, DIF passes -4 %);
// MG_NTT_TWO_CHAINS restores the compiler's coding for re-measurement
#ifdef MG_NTT_TWO_CHAINS
#define MG_NTT_MUL(x, y) R::mul(x, y)
#else
#define MG_NTT_MUL(x, y) R::template mul_t<true>(x, y)
#endif
// The witness map is the head of the chain that bounds a single proof (witness map -> h MSM) and runs beside the accumulate kernels
// of the other MSMs: its wavefronts ask for issue priority 2 -- above the accumulate kernels (0), below the MSMs' tail kernels (3).
// Sequential PrivateTransfer proofs, sparse / W / dense, library variants alternating on one box (profiles/r05_single_proof_ab.txt):
// level 0: 0.728 / 0.872 / 1.290 ms, 1: 0.714 / 0.867 / 1.253, 2: 0.707 / 0.864 / 1.249, 3: 0.716 / 0.925 / 1.245 (level 3 takes issue
// slots from the a | b_g1 | l and G2 chains' own tails: W +6 % -- what round 3 saw when it tried level 3 and dropped it);
// batched passes do not move. MG_WM_PRIO = the s_setprio level at build time (0: off).
#ifndef MG_WM_PRIO
#define MG_WM_PRIO 2
#endif
#if MG_WM_PRIO
#define MG_PRIO_WM() __builtin_amdgcn_s_setprio(MG_WM_PRIO)
#else
#define MG_PRIO_WM() ((void)0)
#endif
struct NttIo {
    const u32 *in_std, *pre_rr;
    u32 *out_std;
    const u32 *scale_rr;
    // the work vector between two passes of the public transform (a scratch vector, not the caller's) in the packed 32 B form
    // (FpR::store_packed): bit 0 = this pass reads it, bit 1 = this pass writes it. A strided pass moves two adjacent elements
    // per butterfly column: 64 B = one aligned sector instead of 72 B across two (2^20: passes 77.6 + 101 -> 75 + 97 us)
    // bit 2 = the tile's twiddles are staged in LDS behind it (ntt_stage_twiddles)
    u32 packed;
};

// the 48-byte record at index i of a twiddle table: 12 words per entry (three 16-byte loads), nine limbs of them used
template <class FrC> MG_DEV FpR<FrC> ntt_load_tw(const u32 *__restrict__ tw, size_t i) {
    static_assert(FpR<FrC>::K == 9, "a twiddle record holds nine limbs");
    const uint4 *q = reinterpret_cast<const uint4 *>(tw + i * 12);
    const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
    FpR<FrC> w;
    w.v[0] = q0.x, w.v[1] = q0.y, w.v[2] = q0.z, w.v[3] = q0.w, w.v[4] = q1.x, w.v[5] = q1.y, w.v[6] = q1.z, w.v[7] = q1.w, w.v[8] = q2.x;
    return w;
}
// Round 5, single-column tiles (cb = 0: the passes of ONE proof's witness map, a chain of six launches with ~1.5 wavefronts per
// SIMD): the tile's 2^ns - 1 twiddles -- entry 2^(tl-1) - 1 + jl for local stage tl -- are fetched ONCE, next to the tile, into
// LDS behind it (limb-major, stride E). Before, every stage waited for its own 48 B gather from a table that the accumulate kernels'
// GB of table traffic keep out of the L2: eight dependent memory latencies per pass (io.packed bit 2; MANTA_NTT_TWL=0 turns it off).
template <class FrC>
MG_DEV void ntt_stage_twiddles(u32 *__restrict__ stw, u32 E, const u32 *__restrict__ tw, unsigned lg, unsigned s0, u32 lo_bits,
                               u32 lo_base) {
    for (u32 x = threadIdx.x + 1; x < E; x += blockDim.x) {
        const unsigned tl = 32u - (unsigned)__clz(x);
        const unsigned s = s0 + tl - 1;
        if (s > 1) {
            const size_t j = ((size_t)(x - (1u << (tl - 1))) << lo_bits) | lo_base;
            ntt_load_tw<FrC>(tw, j << (lg - s)).store_strided(stw + (x - 1), (int)E);
        }
    }
}
// One radix-2 butterfly on (a, b) in place, and what a stage of them does to the bound B of the header comment (every value of the
// tile < B p): the only copy of either, for the LDS stage loop and the register kernel alike. DIT adds 2 (the first stage, w = 1:
// b < 4p, b' = a + 5p - b: adds 5); DIF doubles B and reduces the sum below 2p whenever 2B would exceed 8 (`red`, uniform per stage).
// The overflow argument of the header comment rests on these two functions agreeing, which is why there is one of each.
// lazy (DIT, the register kernel only): the sums a + t and a + 3p - t are left with unnormalised limbs (< 2^31) -- legal wherever
// they only feed the next stage's product and its normalising additions: 9 x 2^31 x 2^29 + 9 x 2^58 < 2^64 -- which saves the two
// carry passes (54 of ~330 VALU instructions per butterfly); the subtraction then adds 3p (fpr_dev.h `subl`), one p more than the
// normalised form: B + 3.
// (a and b are updated in place, the difference first: returned as a pair of values the compiler merges the w = 1 branch into the
// general one with selected constants, and ntt_pass_reg<DIT, 2> goes from 116 to 131 VGPRs -- three waves per SIMD instead of four)
template <bool DIF> MG_DEV bool ntt_stage_reduces(int B) { return DIF && 2 * B > 8; }
template <bool DIF> MG_DEV int ntt_bound_step(int B, bool has_w, bool lazy) {
    if (DIF) return ntt_stage_reduces<DIF>(B) ? 2 : 2 * B;
    return has_w ? B + (lazy ? 3 : 2) : B + 5;
}
template <class FrC, bool DIF> MG_DEV void ntt_butterfly(FpR<FrC> &a, FpR<FrC> &b, const FpR<FrC> &w, bool has_w, bool red, bool lazy) {
    typedef FpR<FrC> R;
    static_assert(R::LIM >= 64, "bound analysis above: any B <= 27 in the only product");
    if (DIF) {
        R x = R::add(a, b);                  // < 2B p
        R y = R::template sub<9>(a, b);      // a + 9p - b (b < 8p) < (B + 9) p
        if (has_w) y = MG_NTT_MUL(y, w);     // < 2p
        else y = R::template reduce<17>(y);  // last DIF stage (w = 1)
        if (red) x = R::template reduce<16>(x);
        a = x, b = y;
    } else if (has_w) {
        const R t = MG_NTT_MUL(b, w); // < 2p
        if (lazy) {
            b = R::template subl<3>(a, t);
#pragma unroll
            for (int l = 0; l < R::K; ++l) a.v[l] += t.v[l];
        } else {
            b = R::template sub<2>(a, t);
            a = R::add(a, t);
        }
    } else { // first DIT stage (w = 1): b < 4p
        const R t = b;
        b = R::template sub<5>(a, t);
        a = R::add(a, t);
    }
}

// ---------------------------------------------------------------------------------------------------
// The tile of a pass kernel's workgroup: the E = 2^ns elements that differ only in index bits [lo_bits, lo_bits + ns) for 2^cb
// adjacent values of the low bits, TOT = E 2^cb elements; element t of the tile is element gi(t) of the vector.
struct NttTile {
    u32 E, TOT, lo_bits, lo_base;
    unsigned cb;
    size_t base;
    MG_DEV NttTile(unsigned s0, unsigned ns, unsigned cb_) : E(1u << ns), TOT(E << cb_), lo_bits(s0 - 1), cb(cb_) {
        const u32 nlo = (1u << lo_bits) >> cb;
        lo_base = (blockIdx.x % nlo) << cb;
        base = ((size_t)(blockIdx.x / nlo) << (lo_bits + ns)) + lo_base;
    }
    MG_DEV size_t gi(u32 t) const { return base + ((size_t)(t >> cb) << lo_bits) + (t & ((1u << cb) - 1)); }
};
// where tile element t lives in LDS (limb-major): at t with stride TOT, or -- the register kernel -- with one pad word per 32
template <bool PAD> MG_DEV u32 ntt_lds_at(u32 t) { return PAD ? t + (t >> 5) : t; }
// HBM -> LDS, every input option: the arkworks-format input gathered at the bit-reversed index, the packed form, the work form
template <class FrC, bool PAD>
MG_DEV void ntt_tile_fill(u32 *__restrict__ sm, u32 stride, const NttTile &T, const u32 *__restrict__ data, unsigned lg, const NttIo &io) {
    typedef FpR<FrC> R;
    for (u32 t = threadIdx.x; t < T.TOT; t += blockDim.x) {
        const size_t gi = T.gi(t);
        R r;
        if (io.in_std) { // arkworks format at the bit-reversed index -> work form (< 2p)
            const u32 j = __brev((u32)gi) >> (32 - lg);
            r = R::from_std_shift(Fp<FrC>::load(io.in_std + (size_t)j * 8));
            if (io.pre_rr) r = R::mul(r, R::load(io.pre_rr + (size_t)j * R::K));
        } else if (io.packed & 1u) {
            r = R::load_packed(data + gi * 8);
        } else {
            r = R::load(data + gi * R::K);
        }
        r.store_strided(sm + ntt_lds_at<PAD>(t), (int)stride);
    }
}
// LDS -> HBM, every output option: times post[i], or the pass's final reduce; then the arkworks format, the packed form, the work form
template <class FrC, bool DIF, bool PAD>
MG_DEV void ntt_tile_drain(const u32 *__restrict__ sm, u32 stride, const NttTile &T, u32 *__restrict__ data, const u32 *__restrict__ post,
                           const NttIo &io, int B) {
    typedef FpR<FrC> R;
    for (u32 t = threadIdx.x; t < T.TOT; t += blockDim.x) {
        const size_t gi = T.gi(t);
        R v = R::load_strided(sm + ntt_lds_at<PAD>(t), (int)stride);
        if (post) v = R::mul(v, R::load(post + gi * R::K)); // any B <= 27 times a canonical table entry: < 2p
        else if (DIF ? B > 4 : true) v = R::template reduce<32>(v);
        if (io.out_std) { // work form (< 4p) -> arkworks format, times the constant of the plain inverse transform first
            if (io.scale_rr) v = R::mul(v, R::load(io.scale_rr));
            v.to_std().store(io.out_std + gi * 8);
        } else if (io.packed & 2u) { // (v < 2p and normalised: a product or a reduce made it)
            v.store_packed(data + gi * 8);
        } else {
            v.store(data + gi * R::K);
        }
    }
}
// the stages of a pass, one LDS round trip and one barrier each, over a tile already in LDS (limb-major, stride E 2^cb): local stages
// 1 .. ns = global stages s0 .. s0 + ns - 1, ascending (DIT) or descending (DIF). stw: the tile's twiddles in LDS (ntt_stage_twiddles)
// or null: each butterfly gathers its own from the table.
template <class FrC, bool DIF>
MG_DEV void ntt_tile_stages(u32 *__restrict__ sm, u32 E, unsigned ns, unsigned s0, unsigned lg, u32 lo_bits, u32 lo_base, unsigned cb,
                            const u32 *__restrict__ tw, const u32 *__restrict__ stw, int &B, u32 tid, u32 nthr) {
    typedef FpR<FrC> R;
    const u32 TOT = E << cb, CM = (1u << cb) - 1;
    for (unsigned st = 0; st < ns; ++st) {
        const unsigned tl = DIF ? ns - st : st + 1; // local stage 1..ns
        const unsigned s = s0 + tl - 1;             // global stage
        const u32 half = 1u << (tl - 1);
        const bool has_w = s > 1;
        const bool red = ntt_stage_reduces<DIF>(B); // uniform
        for (u32 k = tid; k < TOT / 2; k += nthr) {
            const u32 c = k & CM, kk = k >> cb;
            const u32 jl = kk & (half - 1), g = kk >> (tl - 1);
            const u32 i0 = (((g << tl) | jl) << cb) + c, i1 = i0 + (half << cb);
            R a = R::load_strided(sm + i0, (int)TOT), b = R::load_strided(sm + i1, (int)TOT);
            R w;
            if (has_w && stw) w = R::load_strided(stw + (half - 1 + jl), (int)E);
            else if (has_w) w = ntt_load_tw<FrC>(tw, (((size_t)jl << lo_bits) | (lo_base + c)) << (lg - s));
            ntt_butterfly<FrC, DIF>(a, b, w, has_w, red, false);
            a.store_strided(sm + i0, (int)TOT), b.store_strided(sm + i1, (int)TOT);
        }
        B = ntt_bound_step<DIF>(B, has_w, false);
        __syncthreads();
    }
}
template <class FrC, bool DIF>
__global__ __launch_bounds__(1024) void ntt_pass_rr(u32 *__restrict__ d0, u32 *__restrict__ d1, u32 *__restrict__ d2,
                                                   const u32 *__restrict__ tw, unsigned lg, unsigned s0, unsigned ns,
                                                   unsigned cb, const u32 *__restrict__ post, NttIo io) {
    MG_PRIO_WM();
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    constexpr int K = FpR<FrC>::K;
    u32 *__restrict__ data = (blockIdx.y == 0 ? d0 : (blockIdx.y == 1 ? d1 : d2)) + ((size_t)blockIdx.z << lg) * K;
    const NttTile T(s0, ns, cb);
    u32 *__restrict__ stw = (io.packed & 4u) ? sm + (size_t)K * T.TOT : nullptr;
    if (stw) ntt_stage_twiddles<FrC>(stw, T.E, tw, lg, s0, T.lo_bits, T.lo_base);
    ntt_tile_fill<FrC, false>(sm, T.TOT, T, data, lg, io);
    __syncthreads();
    int B = 4; // every value in the tile is < B*p
    ntt_tile_stages<FrC, DIF>(sm, T.E, ns, s0, lg, T.lo_bits, T.lo_base, cb, tw, stw, B, threadIdx.x, blockDim.x);
    ntt_tile_drain<FrC, DIF, false>(sm, T.TOT, T, data, post, io, B);
}

// ---------------------------------------------------------------------------------------------------
// Round 5: pass FUSION for the witness map of ONE proof. With single-column tiles the low pass of the inverse
// transform and the low pass of the forward coset transform that follows it work on the SAME contiguous tile, and so do the high pass
// of the forward transform, the pointwise step and the high pass of the last inverse transform on the same strided tile: 7 launches
// (2 + 2 + pointwise + 2) become 4, three LDS fill / drain pairs and three trips through HBM of a | b | c go away -- on a chain whose
// every launch is latency (six launches of 30-45 us at ~1.5 wavefronts per SIMD). Both run ntt_tile_stages at cb = 0, twiddles gathered.
// low pass of the inverse transform (DIF stages ns .. 1, then the table `post`) + low pass of the forward transform (DIT stages 1 .. ns)
// on one contiguous tile of 2^ns elements; grid (n >> ns, vectors, batch), E / 2 threads
template <class FrC>
__global__ __launch_bounds__(512) void ntt_fused_low(u32 *__restrict__ d0, u32 *__restrict__ d1, u32 *__restrict__ d2,
                                                     const u32 *__restrict__ tw_inv, const u32 *__restrict__ tw_fwd, unsigned lg,
                                                     unsigned ns, const u32 *__restrict__ post) {
    MG_PRIO_WM();
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    typedef FpR<FrC> R;
    constexpr int K = R::K;
    u32 *__restrict__ data = (blockIdx.y == 0 ? d0 : (blockIdx.y == 1 ? d1 : d2)) + ((size_t)blockIdx.z << lg) * K;
    const u32 E = 1u << ns;
    const size_t base = (size_t)blockIdx.x << ns;
    for (u32 t = threadIdx.x; t < E; t += blockDim.x) R::load(data + (base + t) * K).store_strided(sm + t, (int)E);
    __syncthreads();
    int B = 4; // every value of the tile is < B p (the high pass left < 4p)
    ntt_tile_stages<FrC, true>(sm, E, ns, 1, lg, 0, 0, 0, tw_inv, nullptr, B, threadIdx.x, blockDim.x);
    for (u32 t = threadIdx.x; t < E; t += blockDim.x) // n^-1 g^bitrev(i): any B <= 27 times a canonical entry -> < 2p
        R::mul(R::load_strided(sm + t, (int)E), R::load(post + (base + t) * K)).store_strided(sm + t, (int)E);
    __syncthreads();
    B = 2;
    ntt_tile_stages<FrC, false>(sm, E, ns, 1, lg, 0, 0, 0, tw_fwd, nullptr, B, threadIdx.x, blockDim.x);
    for (u32 t = threadIdx.x; t < E; t += blockDim.x)
        R::template reduce<32>(R::load_strided(sm + t, (int)E)).store(data + (base + t) * K);
}
// high pass of the forward transform on a, b, c (DIT stages lo + 1 .. lg; a third of the workgroup each) + (a b - c) / Z + high pass of
// the inverse transform on the result (DIF stages lg .. lo + 1), one strided tile (column blockIdx.x) of 2^ns elements per vector;
// grid (n >> ns, 1, batch), 3 E / 2 threads
template <class FrC>
__global__ __launch_bounds__(1024) void ntt_fused_high_pw(u32 *__restrict__ a, u32 *__restrict__ b, u32 *__restrict__ c,
                                                          const u32 *__restrict__ tw_fwd, const u32 *__restrict__ tw_inv, unsigned lg,
                                                          unsigned ns, const u32 *__restrict__ zinv_rr) {
    MG_PRIO_WM();
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    typedef FpR<FrC> R;
    constexpr int K = R::K;
    const u32 E = 1u << ns, lo_bits = lg - ns, s0 = lo_bits + 1, lo_base = blockIdx.x;
    const u32 per = blockDim.x / 3, vec = threadIdx.x / per, tid = threadIdx.x - vec * per;
    u32 *__restrict__ data = (vec == 0 ? a : (vec == 1 ? b : c)) + ((size_t)blockIdx.z << lg) * K;
    u32 *__restrict__ tile = sm + (size_t)vec * K * E;
    for (u32 t = tid; t < E; t += per) R::load(data + ((size_t)lo_base + ((size_t)t << lo_bits)) * K).store_strided(tile + t, (int)E);
    __syncthreads();
    int B = 4;
    ntt_tile_stages<FrC, false>(tile, E, ns, s0, lg, lo_bits, lo_base, 0, tw_fwd, nullptr, B, tid, per);
    const R zinv = R::load(zinv_rr);
    u32 *ta = sm, *tb = sm + (size_t)K * E, *tc = sm + (size_t)2 * K * E;
    for (u32 t = threadIdx.x; t < E; t += blockDim.x) { // h = (a b - c) (g^D - 1)^-1 on the coset, < 2p
        const R x = R::template reduce<32>(R::load_strided(ta + t, (int)E)), y = R::template reduce<32>(R::load_strided(tb + t, (int)E)),
                z = R::template reduce<32>(R::load_strided(tc + t, (int)E));
        R::mul(R::template sub<5>(R::mul(x, y), z), zinv).store_strided(ta + t, (int)E);
    }
    __syncthreads();
    B = 2;
    ntt_tile_stages<FrC, true>(ta, E, ns, s0, lg, lo_bits, lo_base, 0, tw_inv, nullptr, B, threadIdx.x, blockDim.x);
    u32 *__restrict__ out = a + ((size_t)blockIdx.z << lg) * K;
    for (u32 t = threadIdx.x; t < E; t += blockDim.x) {
        R v = R::load_strided(ta + t, (int)E);
        if (B > 4) v = R::template reduce<32>(v);
        v.store(out + ((size_t)lo_base + ((size_t)t << lo_bits)) * K);
    }
}

// ---------------------------------------------------------------------------------------------------
// Round 4: the same pass with the butterflies of up to THREE consecutive stages done in REGISTERS. PMC of the kernel above
// (profiles/r04_pmc_ntt.txt, 2^20): 394 VALU instructions per butterfly of which 171 are multiply-adds, 40 LDS instructions per
// butterfly and bank conflicts in 54 % of the LDS-active cycles (stages whose partner distance is below 64 elements touch every
// other bank) -- the pass runs at 70-80 % of the issue bound of ITS OWN instruction stream, so the stream has to shrink. Here a
// thread owns the 2^LR (8) tile elements that differ in LR consecutive index bits, fetches them from LDS once, runs the LR stages
// that pair exactly those bits (12 butterflies, 7 distinct twiddles: index arithmetic and twiddle addressing once per thread and
// group, not once per butterfly and stage) and puts them back: ceil(ns / LR) LDS round trips and barriers per pass instead of
// ns. The tile is stored with one pad word per 32 (address t + t / 32): the strided accesses of the low groups -- 8 elements per
// lane, lane-to-lane stride 8 -- and the unit-stride ones of the high groups are both conflict-free.
// Same arguments, same bounds bookkeeping and same I/O options as ntt_pass_rr; tiles of at least 64 * 2^LR elements.
// A stage may leave its outputs lazy (ntt_butterfly)
// only as the FIRST of two consecutive in-register DIT stages of a two-bit group: its lazy outputs (limbs < 2^29 + 2^30) meet one
// normalising stage before they are stored; groups of three would stack two lazy stages (limbs up to 2^29 + 2 x 2^30: too wide)
template <bool DIF> MG_DEV bool ntt_lazy_stage(int q, int lr, unsigned bit, unsigned first_bit, unsigned gs, unsigned s) {
#ifdef MG_NTT_NO_LAZY
    return false;
#else
    return !DIF && lr == 2 && q == 0 && gs == 2 && bit == first_bit && s > 1;
#endif
}
// one butterfly stage on the 2^LR elements a lane holds in registers: pairs the owned bit Q; 2^Q distinct twiddles (the owned
// bits below Q), each shared by the 2^(LR-1-Q) butterflies that differ in the owned bits above Q
template <class FrC, bool DIF, int LR, int Q>
MG_DEV void ntt_reg_stage(FpR<FrC> (&v)[1 << LR], const u32 *__restrict__ tw, bool has_w, bool red, unsigned b0, u32 e_lo,
                          u32 lo_bits, u32 col, unsigned tw_shift, bool lazy, const u32 *__restrict__ stw, u32 ntw) {
    typedef FpR<FrC> R;
#pragma unroll
    for (int u = 0; u < (1 << Q); ++u) {
        const u32 jl = ((u32)u << b0) | e_lo; // the stage bits below the paired one
        R w;
        // the tile's twiddles staged in LDS (single-column tiles): entry 2^bit - 1 + jl, bit = b0 + Q
        if (has_w && stw) w = R::load_strided(stw + ((1u << (b0 + (unsigned)Q)) - 1u + jl), (int)ntw);
        else if (has_w) w = ntt_load_tw<FrC>(tw, (((size_t)jl << lo_bits) | col) << tw_shift);
#pragma unroll
        for (int h = 0; h < (1 << (LR - 1 - Q)); ++h) {
            const int i0 = (h << (Q + 1)) | u, i1 = i0 | (1 << Q);
            ntt_butterfly<FrC, DIF>(v[i0], v[i1], w, has_w, red, lazy);
        }
    }
}

#ifndef MG_NTT_REG_WAVES
#define MG_NTT_REG_WAVES 2
#endif
template <class FrC, bool DIF, int LR>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(MG_NTT_REG_WAVES, 8))) void ntt_pass_reg(u32 *__restrict__ d0, u32 *__restrict__ d1, u32 *__restrict__ d2,
                                                   const u32 *__restrict__ tw, unsigned lg, unsigned s0, unsigned ns,
                                                   unsigned cb, const u32 *__restrict__ post, NttIo io) {
    MG_PRIO_WM();
    extern __shared__ __attribute__((aligned(16))) u32 sm[];
    typedef FpR<FrC> R;
    constexpr int K = R::K, NE = 1 << LR;
    u32 *__restrict__ data = (blockIdx.y == 0 ? d0 : (blockIdx.y == 1 ? d1 : d2)) + ((size_t)blockIdx.z << lg) * K;
    const NttTile T(s0, ns, cb);
    const u32 TOTP = T.TOT + (T.TOT >> 5);
    u32 *__restrict__ stw = (io.packed & 4u) ? sm + (size_t)K * TOTP : nullptr;
    if (stw) ntt_stage_twiddles<FrC>(stw, T.E, tw, lg, s0, T.lo_bits, T.lo_base);
    ntt_tile_fill<FrC, true>(sm, TOTP, T, data, lg, io);
    __syncthreads();
    int B = 4; // every value in the tile is < B*p
    const u32 nthr = T.TOT >> LR;
    for (unsigned done = 0; done < ns;) {
        const unsigned gs = ns - done < (unsigned)LR ? ns - done : (unsigned)LR;
        // the LR stage bits this group's threads own: [b0, b0 + LR), the gs unprocessed ones among them are bits
        //   DIT (ascending):  done .. done + gs - 1          DIF (descending): ns - done - gs .. ns - done - 1
        const unsigned first_bit = DIF ? ns - done - gs : done;
        unsigned b0 = first_bit + gs >= (unsigned)LR ? (DIF ? first_bit : (first_bit + LR <= ns ? first_bit : ns - LR)) : 0;
        if (b0 + LR > ns) b0 = ns >= (unsigned)LR ? ns - LR : 0;
        const unsigned p0 = cb + b0;
        // per owned bit Q, in the order the stages run: is it one of this group's stages, is its sum reduced, may its outputs stay
        // lazy (DIT: a stage whose outputs are consumed by another stage of this group, not stored) -- and the bound after the
        // group. Uniform: once per group, the same for every thread, also for those without elements.
        bool on[LR], red[LR], lazy[LR];
#pragma unroll
        for (int k = 0; k < LR; ++k) {
            const int q = DIF ? LR - 1 - k : k;
            const unsigned bit = b0 + (unsigned)q, s = s0 + bit; // local stage bit (local stage number tl = bit + 1); global stage
            on[q] = bit >= first_bit && bit < first_bit + gs;
            lazy[q] = on[q] && ntt_lazy_stage<DIF>(q, LR, bit, first_bit, gs, s);
            red[q] = on[q] && ntt_stage_reduces<DIF>(B);
            if (on[q]) B = ntt_bound_step<DIF>(B, s > 1, lazy[q]);
        }
        for (u32 vt = threadIdx.x; vt < nthr; vt += blockDim.x) { // (one trip when the workgroup has a thread per 2^LR elements)
            const u32 lo = vt & ((1u << p0) - 1), hi = vt >> p0;
            const u32 tb = (hi << (p0 + LR)) | lo;
            const u32 c = lo & ((1u << cb) - 1), e_lo = lo >> cb; // column; the stage bits below b0
            R v[NE];
#pragma unroll
            for (int j = 0; j < NE; ++j) v[j] = R::load_strided(sm + ntt_lds_at<true>(tb + ((u32)j << p0)), (int)TOTP);
            // the stages of this group, one call per owned bit with the bit as a template constant (every register index static)
            auto run = [&](auto qc) {
                constexpr int Q = decltype(qc)::value;
                if (!on[Q]) return; // (uniform) not one of this group's stages
                const unsigned s = s0 + b0 + (unsigned)Q; // global stage
                ntt_reg_stage<FrC, DIF, LR, Q>(v, tw, s > 1, red[Q], b0, e_lo, T.lo_bits, T.lo_base + c, lg - s, lazy[Q], stw, T.E);
            };
            if constexpr (DIF) {
                if constexpr (LR > 2) run(std::integral_constant<int, 2>());
                run(std::integral_constant<int, 1>());
                run(std::integral_constant<int, 0>());
            } else {
                run(std::integral_constant<int, 0>());
                run(std::integral_constant<int, 1>());
                if constexpr (LR > 2) run(std::integral_constant<int, 2>());
            }
#pragma unroll
            for (int j = 0; j < NE; ++j) v[j].store_strided(sm + ntt_lds_at<true>(tb + ((u32)j << p0)), (int)TOTP);
        }
        __syncthreads();
        done += gs;
    }
    ntt_tile_drain<FrC, DIF, true>(sm, TOTP, T, data, post, io, B);
}

// The one kernel that fills a domain's tables: out[i] = scale * base^e(i), i < n, with e(i) = i or (brev_lg > 0) the reversal of
// the low brev_lg bits of i. The powers are products of the squarings sq[k] = base^(2^k), k < bits (arkworks format, computed on
// the host, passed by value). RR = false: the 8 arkworks words of the element; RR = true: its canonical (< p) reduced-radix limbs,
// `stride` words per entry, pad words zero.
struct FrPowers {
    u32 sq[32][8], scale[8];
};
template <class FrC, bool RR>
__global__ __launch_bounds__(256) void domain_table_kernel(u32 *__restrict__ out, u32 stride, u32 n, int bits, unsigned brev_lg,
                                                           const FrPowers pw) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef Fp<FrC> F;
    typedef FpR<FrC> R;
    const u32 e = brev_lg ? __brev(i) >> (32 - brev_lg) : i;
    F acc = F::load(pw.scale);
    for (int k = 0; k < bits; ++k)
        if ((e >> k) & 1) acc = F::mul(acc, F::load(pw.sq[k]));
    if (RR) {
        const R r = R::from_std(acc);
#pragma unroll
        for (int l = 0; l < R::K; ++l) out[(size_t)i * stride + l] = r.v[l];
        for (u32 l = R::K; l < stride; ++l) out[(size_t)i * stride + l] = 0;
    } else {
        acc.store(out + (size_t)i * 8);
    }
}
// public-API entry: out_rr[i] = in_std[bitrev(i)] (x pre[bitrev(i)] for the forward coset transform), < 2p
template <class FrC>
__global__ __launch_bounds__(256) void ntt_load_rr_kernel(const u32 *__restrict__ in_std, unsigned lg, const u32 *__restrict__ pre_rr,
                                                          u32 *__restrict__ out_rr) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << lg)) return;
    typedef FpR<FrC> R;
    const u32 j = lg ? (__brev(i) >> (32 - lg)) : 0;
    R r = R::from_std_shift(Fp<FrC>::load(in_std + (size_t)j * 8));
    if (pre_rr) r = R::mul(r, R::load(pre_rr + (size_t)j * R::K));
    r.store(out_rr + (size_t)i * R::K);
}
// reduced radix (< 4p) -> arkworks format, optionally times a constant first
template <class FrC>
__global__ __launch_bounds__(256) void rr_to_std_kernel(const u32 *__restrict__ in_rr, size_t n, const u32 *__restrict__ scale_rr,
                                                        u32 *__restrict__ out_std) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef FpR<FrC> R;
    R r = R::load(in_rr + i * R::K);
    if (scale_rr) r = R::mul(r, R::load(scale_rr));
    r.to_std().store(out_std + i * 8);
}

// the same for three matrices at once (blockIdx.z): A z, B z, C z of the witness map. Outputs are written in the
// reduced-radix form of the NTT pipeline (9 words per element); matrix 0 (A) also fills the input-consistency rows
// a[m + j] = z_j, j < P (mpc.rs:299-312).
struct Csr3 {
    const u32 *row_ptr[3], *col[3], *val[3];
    u32 *out[3];
};
template <class FrC>
__global__ __launch_bounds__(256) void spmv3_kernel(Csr3 M, const u32 *__restrict__ z, u32 m, u32 P, size_t z_stride, size_t out_stride,
                                                    u32 rows_total) {
    MG_PRIO_WM();
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.z;
    z += (size_t)blockIdx.y * z_stride; // batch member
    u32 *__restrict__ out = M.out[t] + (size_t)blockIdx.y * out_stride;
    typedef Fp<FrC> F;
    typedef FpR<FrC> R;
    if (i >= m + (t == 0 ? P : 0)) {
        // rows past the constraints (and, in A, past the input-consistency rows) up to the domain size are zero -- written here, by the
        // kernel that owns the vector, not by a memset node in front of it (round 5: a hipMemsetAsync node of a LINEAR captured graph
        // replays with a wrong fill pattern once other work has gone through the runtime: profiles/r05_linear_graph_defect.txt)
        if (i < rows_total) {
#pragma unroll
            for (int k = 0; k < R::K; ++k) out[(size_t)i * R::K + k] = 0u;
        }
        return;
    }
    F acc = F::zero();
    if (i >= m) {
        acc = F::load(z + (size_t)(i - m) * 8);
    } else {
        const u32 *__restrict__ row_ptr = M.row_ptr[t], *__restrict__ col = M.col[t], *__restrict__ val = M.val[t];
        const F one = F::one();
        for (u32 k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
            F c = F::load(val + (size_t)k * 8);
            F x = F::load(z + (size_t)col[k] * 8);
            acc = F::add(acc, c == one ? x : F::mul(x, c));
        }
    }
    R::from_std_shift(acc).store(out + (size_t)i * R::K);
}

// R1CS satisfaction (R1CS::is_satisfied, manta-crypto/src/arkworks/constraint/mod.rs:130-132 -> ark-relations
// ConstraintSystem::which_is_unsatisfied): <A_i, z> <B_i, z> == <C_i, z> for the m constraint rows of one assignment per blockIdx.y.
// Nothing else is looked at -- not the input-consistency rows a[m + j] = z_j, not the padding up to the domain size, not z_0 -- as
// in ark-relations. One row per lane, its three dot products one after the other in the arithmetic of spmv3_kernel (canonical
// Fp values, the coefficient-equals-one shortcut); the row loop is a copy of that kernel's on purpose: spmv3_kernel is on the
// path that bounds a single proof and its code stays what it was measured as.
// The verdict: rows rise with the lane, so the lowest set bit of the wavefront's 64-bit ballot is its first failing row. Only a
// wavefront that has one touches memory: a minimum into first[y] (0xFFFFFFFF before: r1cs_check) and its population count added
// to count[y]. Both are order-independent, so the result is the same on every run; a satisfied batch issues no atomic at all.
template <class FrC> MG_DEV Fp<FrC> r1cs_row_dot(const u32 *__restrict__ row_ptr, const u32 *__restrict__ col, const u32 *__restrict__ val,
                                                 const u32 *__restrict__ z, u32 i) {
    typedef Fp<FrC> F;
    const F one = F::one();
    F acc = F::zero();
    for (u32 k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
        F c = F::load(val + (size_t)k * 8);
        F x = F::load(z + (size_t)col[k] * 8);
        acc = F::add(acc, c == one ? x : F::mul(x, c));
    }
    return acc;
}
template <class FrC>
__global__ __launch_bounds__(256) void r1cs_check_kernel(Csr3 M, const u32 *__restrict__ z, u32 m, size_t z_stride, u32 *__restrict__ first,
                                                         u32 *__restrict__ count) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    z += (size_t)blockIdx.y * z_stride; // batch member
    typedef Fp<FrC> F;
    bool bad = false;
    if (i < m) {
        const F a = r1cs_row_dot<FrC>(M.row_ptr[0], M.col[0], M.val[0], z, i), b = r1cs_row_dot<FrC>(M.row_ptr[1], M.col[1], M.val[1], z, i),
                c = r1cs_row_dot<FrC>(M.row_ptr[2], M.col[2], M.val[2], z, i);
        bad = !(F::mul(a, b) == c);
    }
    // (no lane has left: workgroups are 256 lanes, four whole wavefronts, and rows past m merely vote "fine")
    const u64 failing = __ballot(bad);
    if (failing && (threadIdx.x & 63u) == 0) {
        atomicMin(first + blockIdx.y, i + (u32)__ffsll((unsigned long long)failing) - 1u);
        atomicAdd(count + blockIdx.y, (u32)__popcll(failing));
    }
}

// a[i] = (a[i] b[i] - c[i]) * (g^D - 1)^-1, reduced-radix vectors (inputs < 4p, output < 2p)
template <class FrC>
__global__ __launch_bounds__(256) void qap_pointwise_kernel(u32 *__restrict__ a, const u32 *__restrict__ b,
                                                            const u32 *__restrict__ c, const u32 *__restrict__ zinv_rr,
                                                            u32 n) {
    MG_PRIO_WM();
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef FpR<FrC> R;
    const size_t o = ((size_t)blockIdx.y * n + i) * R::K; // batch member
    R ab = R::mul(R::load(a + o), R::load(b + o));            // 4 * 4 <= LIM: < 2p
    ab = R::template sub<5>(ab, R::load(c + o));              // + 5p - c (c < 4p): < 7p
    R::mul(ab, R::load(zinv_rr)).store(a + o);
}

// ---------------------------------------------------------------------------------------------------
// The passes of one transform, decided on the host before anything is launched (ntt_plan) and launched as decided (run_passes).
// The tile limits every shape decision and every LDS maximum below derives from:
constexpr unsigned NTT_PASS_STAGES = 10; // stages per pass at most
constexpr unsigned NTT_TILE_LG = 11;     // a tile holds at most 2^11 elements = 72 KB of LDS (two workgroups per CU)
constexpr unsigned NTT_CB_MAX = 3;       // adjacent columns per tile: 2^3 at most
// the fused witness map (qap_quotient): domains 2^12 .. 2^18, whose high half is at most 2^9 elements for each of a, b, c
constexpr unsigned NTT_FUSE_LG_MIN = 12, NTT_FUSE_LG_MAX = 18, NTT_FUSE_TILE_LG = NTT_FUSE_LG_MAX - NTT_FUSE_LG_MAX / 2;
constexpr u32 ntt_padded(u32 tot) { return tot + (tot >> 5); } // the register kernel's tile: one pad word per 32 (ntt_lds_at)
// a tile of `tot` elements of K words: LDS bytes, and threads -- a butterfly per thread and stage (a full tile: 1024 threads = 4
// wavefronts per SIMD; a pass is a chain of dependent multiplications, more resident waves hide its latency), a wavefront at least
template <int K> constexpr size_t ntt_tile_bytes(u32 tot) { return (size_t)(4 * K) * tot; }
constexpr u32 ntt_tile_threads(u32 tot) { return tot / 2 > 64u ? tot / 2 : 64u; }

// The A/B knobs of the passes (tuning.h ab_knob).
struct NttKnobs {
    // stages per LDS round trip. Measured (profiles/r04_ntt_register_stages.txt): the DIT passes gain from two stages per round
    // trip (2^20 public transform 0.191 -> 0.17 ms; the 3-vector passes of a 32-proof witness map 268 + 428 -> 248 + 313 us), the
    // DIF passes do not (318 + 415 -> 340 + 433 us: their product comes AFTER the subtraction, the extra live registers cost
    // occupancy) and three stages per round trip lose everywhere (215-256 VGPRs). MANTA_NTT_R = 0 / 2 / 3 forces one; -1: by direction
    int reg_bits = -1;
    u32 threads = 0; // MANTA_NTT_THREADS: threads of an ntt_pass_rr workgroup; 0 = by tile
    // a SINGLE proof's witness map is a latency chain of six passes over three 2^16-element vectors: with 2048-element tiles a
    // pass is 32-96 workgroups on 256 CUs. Narrower column groups = more, smaller workgroups (the vectors live in L2: the
    // coalescing the wide groups buy is worth nothing here). MANTA_NTT_MIN_WGS = workgroups a pass should have.
    u32 min_wgs = 512;
    // single-column tiles of a LATENCY-bound launch (one proof's witness map: <= 2 workgroups per CU): twiddles staged in LDS
    // (E entries of 36 B more). A 2^20 transform is 1 024 workgroups per pass and throughput-bound: there the larger LDS
    // footprint costs 8 % (0.154 -> 0.166 ms, tools/ntt_ab_r5.sh), so it keeps the per-stage gathers. MANTA_NTT_TWL = 0: never
    bool twl = true;
};
struct NttPass {
    unsigned s0, ns, cb; // global stages s0 .. s0 + ns - 1 on tiles of 2^ns elements x 2^cb columns
    u32 blocks, threads;
    size_t lds; // dynamic LDS bytes: the tile (padded for the register kernel) and, with `twl`, its twiddles behind it
    int reg;    // 0: ntt_pass_rr; 2 / 3: ntt_pass_reg with that many stages per LDS round trip
    bool twl;   // NttIo::packed bit 2
    u32 pack;   // NttIo::packed bits 0 and 1: the public transform's passes hand the vector on in the packed form
};
struct NttPlan {
    unsigned n = 0;
    NttPass p[4]; // lg <= 32, ten stages per pass
};
// every stage of a 2^lg transform (lg >= 1) of `nvec` vectors x `batch` as LDS-fused passes, in launch order: DIT walks the stages
// upwards, DIF downwards. pub: the public transform (arkworks format in and out, the work vector a scratch vector). K: words per element
template <int K> inline NttPlan ntt_plan(unsigned lg, int nvec, u32 batch, bool dif, bool pub, const NttKnobs &kn) {
    NttPlan plan;
    const unsigned npass = (lg + NTT_PASS_STAGES - 1) / NTT_PASS_STAGES;
    const int lr = kn.reg_bits >= 0 ? kn.reg_bits : (dif ? 0 : 2);
    unsigned done = 0;
    for (unsigned i = 0; i < npass; ++i) {
        NttPass &p = plan.p[plan.n++];
        p.ns = (lg - done + (npass - i) - 1) / (npass - i); // balanced split
        p.s0 = dif ? (lg - done - p.ns + 1) : (done + 1);
        const unsigned lo_bits = p.s0 - 1;
        p.cb = std::min(std::min(NTT_TILE_LG - p.ns, lo_bits), NTT_CB_MAX);
        while (p.cb > 0 && ((((size_t)1 << lg) >> (p.ns + p.cb)) * (size_t)nvec * batch) < kn.min_wgs && (1u << (p.ns + p.cb - 1)) >= 128u)
            --p.cb;
        p.blocks = (u32)(((size_t)1 << lg) >> (p.ns + p.cb));
        const u32 tot = 1u << (p.ns + p.cb);
        p.twl = kn.twl && p.cb == 0 && p.ns >= 2 && (size_t)p.blocks * nvec * batch <= 512;
        const size_t twl_bytes = p.twl ? ntt_tile_bytes<K>(1u << p.ns) : 0;
        p.pack = pub && npass > 1 && !dif ? (i > 0 ? 1u : 0u) | (i + 1 < npass ? 2u : 0u) : 0u;
        // stages in registers (ntt_pass_reg) for every tile with a full wavefront of 2^lr-element lanes
        p.reg = lr && tot >= (64u << lr) && p.ns >= (unsigned)lr ? lr : 0;
        p.threads = p.reg ? std::min<u32>(512u, tot >> lr) : (kn.threads ? kn.threads : ntt_tile_threads(tot));
        p.lds = ntt_tile_bytes<K>(p.reg ? ntt_padded(tot) : tot) + twl_bytes;
        done += p.ns;
    }
    return plan;
}

// Domain: one per size, every table of the transforms of 2^log_n elements in ONE device allocation (the members point into it,
// each on a 16-byte boundary), written once in its final form by domain_table_kernel and never changed. Saturated
// (arkworks format, 8 words) are only the twiddles the group NTT reads through domain_twiddles; everything the Fr pipeline reads
// is in its reduced-radix form, canonical values: twiddles 12 words per entry (ntt_load_tw: three 16-byte loads), the rest 9.
// FrEngineT is the device half of the Fr engine, the domains and the launches; the host half is FrHostT (fr_host.h).
template <class FrC> class FrEngineT : public FrHostT<FrC> {
  public:
    typedef typename FrHostT<FrC>::HF HF;
    using FrHostT<FrC>::host_load;
    using FrHostT<FrC>::hpow2k;
    using FrHostT<FrC>::from_u64;
    struct Domain {
        u32 *tw_fwd = nullptr, *tw_inv = nullptr;             // omega^k, omega^-k, k < n/2, saturated (tw_fwd: the start of the block)
        u32 *tw_fwd_rr = nullptr, *tw_inv_rr = nullptr;       // the same in the reduced-radix form, TW_WORDS per entry
        u32 *coset_fwd_rr = nullptr, *coset_inv_rr = nullptr; // g^i; n^-1 g^-i
        u32 *t1_br_rr = nullptr;                              // n^-1 g^bitrev(p)   (between ifft and coset fft)
        u32 *t2_br_rr = nullptr;                              // n^-1 g^-bitrev(p)  (after the final coset ifft)
        u32 *consts_rr = nullptr;                             // [0] n^-1, [1] (g^n - 1)^-1
        u32 *scratch_rr = nullptr; // its own allocation, made on first use: the public transform's work vector (guarded by scratch_mu_)
    };
    static constexpr int RK = FpR<FrC>::K; // words per reduced-radix element
    static constexpr u32 TW_WORDS = 12;    // words per reduced-radix twiddle record

    // builds the domain of 2^log_n elements: one allocation, its launches on the setup stream, one wait. The allocation belongs
    // to `own` until the caller has stored the domain.
    typedef std::unique_ptr<void, hipError_t (*)(void *)> DevOwner;
    static int make_domain(unsigned log_n, Domain &d, DevOwner &own) {
        const size_t n = (size_t)1 << log_n, half = n > 1 ? n / 2 : 1;
        size_t words = 0;
        auto take = [&](size_t cnt, size_t stride) { // word offset of a sub-array of cnt entries, 16-byte aligned
            const size_t at = words;
            words += (cnt * stride + 3) & ~(size_t)3;
            return at;
        };
        const size_t o_tw_fwd = take(half, 8), o_tw_inv = take(half, 8), o_tw_fwd_rr = take(half, TW_WORDS), o_tw_inv_rr = take(half, TW_WORDS),
                     o_coset_fwd = take(n, RK), o_coset_inv = take(n, RK), o_t1 = take(n, RK), o_t2 = take(n, RK), o_consts = take(2, RK);
        void *p = nullptr;
        MG_HIP(hipMalloc(&p, words * 4));
        own.reset(p);
        u32 *const blk = (u32 *)p;
        d.tw_fwd = blk + o_tw_fwd, d.tw_inv = blk + o_tw_inv, d.tw_fwd_rr = blk + o_tw_fwd_rr, d.tw_inv_rr = blk + o_tw_inv_rr;
        d.coset_fwd_rr = blk + o_coset_fwd, d.coset_inv_rr = blk + o_coset_inv, d.t1_br_rr = blk + o_t1, d.t2_br_rr = blk + o_t2;
        d.consts_rr = blk + o_consts;
        const HF root = hpow2k(host_load(FrC::ROOT), FrC::TWO_ADICITY - (int)log_n), gen = host_load(FrC::GEN);
        const HF n_inv = HF::inv(from_u64((u64)n)), zinv = HF::inv(HF::sub(hpow2k(gen, (int)log_n), HF::one()));
        // out = scale * base^e(i): squarings of the base on the host, powers on the device
        auto fill = [&](u32 *out, bool rr, u32 stride, size_t cnt, HF base, const HF &scale, bool brev) {
            FrPowers pw{};
            for (unsigned k = 0; k < log_n; ++k) base.store_words(pw.sq[k]), base = HF::sqr(base);
            scale.store_words(pw.scale);
            const auto kern = rr ? &domain_table_kernel<FrC, true> : &domain_table_kernel<FrC, false>;
            hipLaunchKernelGGL(kern, dim3((u32)((cnt + 255) / 256)), dim3(256), 0, setup_stream(), out, stride, (u32)cnt, (int)log_n,
                               brev ? log_n : 0u, pw);
        };
        const HF one = HF::one(), root_inv = HF::inv(root), gen_inv = HF::inv(gen);
        fill(d.tw_fwd, false, 8, half, root, one, false);
        fill(d.tw_inv, false, 8, half, root_inv, one, false);
        fill(d.tw_fwd_rr, true, TW_WORDS, half, root, one, false);
        fill(d.tw_inv_rr, true, TW_WORDS, half, root_inv, one, false);
        fill(d.coset_fwd_rr, true, RK, n, gen, one, false);
        fill(d.coset_inv_rr, true, RK, n, gen_inv, n_inv, false);
        fill(d.t1_br_rr, true, RK, n, gen, n_inv, true);
        fill(d.t2_br_rr, true, RK, n, gen_inv, n_inv, true);
        fill(d.consts_rr, true, RK, 1, one, n_inv, false);
        fill(d.consts_rr + RK, true, RK, 1, one, zinv, false);
        MG_HIP(setup_sync());
        return MG_OK;
    }
    int get_domain(unsigned log_n, Domain **out) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = domains_.find(log_n);
        if (it != domains_.end()) {
            *out = &it->second;
            return MG_OK;
        }
        if ((int)log_n > FrC::TWO_ADICITY) return MG_ERR_DOMAIN;
        Domain d;
        DevOwner own(nullptr, hipFree);
        if (const int rc = make_domain(log_n, d, own)) return rc;
        *out = &domains_.emplace(log_n, d).first->second;
        own.release();
        return MG_OK;
    }

    static const NttKnobs &ntt_knobs() {
        static const NttKnobs k = [] { // read once per process
            const int r = ab_knob("MANTA_NTT_R", -1), w = ab_knob("MANTA_NTT_MIN_WGS", 512);
            return NttKnobs{r == 0 || r == 2 || r == 3 ? r : -1, (u32)ab_knob("MANTA_NTT_THREADS", 0), (u32)(w >= 1 ? w : 1),
                            ab_knob("MANTA_NTT_TWL", 1) != 0};
        }();
        return k;
    }
    static void allow_lds(const void *kernel, size_t bytes) { // above the 64 KB default of dynamic LDS
        hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    }
    // one launch of a pass kernel as planned; first / last: the transform's I/O options and `post` apply at its ends only
    template <bool DIF>
    static void launch_pass(const NttPass &p, u32 *d0, u32 *d1, u32 *d2, int nvec, const u32 *tw_rr, unsigned lg, const u32 *post_rr,
                            hipStream_t s, u32 batch, const NttIo &io, bool first, bool last) {
        const NttIo pio{first ? io.in_std : nullptr, first ? io.pre_rr : nullptr, last ? io.out_std : nullptr, last ? io.scale_rr : nullptr,
                        p.pack | (p.twl ? 4u : 0u)};
        const auto kern = p.reg == 3 ? &ntt_pass_reg<FrC, DIF, 3> : p.reg == 2 ? &ntt_pass_reg<FrC, DIF, 2> : &ntt_pass_rr<FrC, DIF>;
        hipLaunchKernelGGL(kern, dim3(p.blocks, nvec, batch), dim3(p.threads), p.lds, s, d0, d1, d2, tw_rr, lg, p.s0, p.ns, p.cb,
                           last ? post_rr : (const u32 *)nullptr, pio);
    }
    // all stages of one transform over up to 3 reduced-radix vectors as LDS-fused passes of <= 10 stages
    template <bool DIF>
    static void run_passes(u32 *d0, u32 *d1, u32 *d2, int nvec, const u32 *tw_rr, unsigned lg, const u32 *post_rr, hipStream_t s,
                           u32 batch = 1, NttIo io = NttIo{}) {
        if (lg == 0) return;
        static const bool attr_set = [] { // the largest tile, with its padding in the register kernel
            allow_lds(reinterpret_cast<const void *>(&ntt_pass_rr<FrC, DIF>), ntt_tile_bytes<RK>(1u << NTT_TILE_LG));
            allow_lds(reinterpret_cast<const void *>(&ntt_pass_reg<FrC, DIF, 3>), ntt_tile_bytes<RK>(ntt_padded(1u << NTT_TILE_LG)));
            allow_lds(reinterpret_cast<const void *>(&ntt_pass_reg<FrC, DIF, 2>), ntt_tile_bytes<RK>(ntt_padded(1u << NTT_TILE_LG)));
            return true;
        }();
        (void)attr_set;
        const NttPlan plan = ntt_plan<RK>(lg, nvec, batch, DIF, io.in_std && io.out_std, ntt_knobs());
        for (unsigned i = 0; i < plan.n; ++i)
            launch_pass<DIF>(plan.p[i], d0, d1, d2, nvec, tw_rr, lg, post_rr, s, batch, io, i == 0, i + 1 == plan.n);
    }

    // single-column tiles of 2^ns elements (one proof's witness map): a butterfly per thread, 36 B of LDS per element
    static u32 tile_threads(unsigned ns) { return ntt_tile_threads(1u << ns); }
    static size_t tile_lds(unsigned ns) { return ntt_tile_bytes<RK>(1u << ns); }
    // one ntt_pass_rr pass over such tiles: stages s0 .. s0 + ns - 1 of the 2^lg transform of `nvec` vectors, plain work form in and out
    template <bool DIF>
    static void rr_pass(u32 *d0, u32 *d1, u32 *d2, int nvec, const u32 *tw_rr, unsigned lg, unsigned s0, unsigned ns, const u32 *post_rr,
                        hipStream_t s, u32 batch) {
        const NttPass p{s0, ns, 0u, (1u << lg) >> ns, tile_threads(ns), tile_lds(ns), 0, false, 0u};
        launch_pass<DIF>(p, d0, d1, d2, nvec, tw_rr, lg, post_rr, s, batch, NttIo{}, true, true);
    }

    // Radix2EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}_in_place on 2^log_n arkworks-format elements in HBM:
    // converted to the reduced-radix form on the way in (bit-reversal and the coset pre-scaling folded into that
    // kernel), DIT passes, scaled and converted back on the way out.
    int transform(u32 *d_data, unsigned log_n, bool inverse, bool coset, hipStream_t s) override {
        Domain *d;
        int rc = get_domain(log_n, &d);
        if (rc) return rc;
        const u32 n = 1u << log_n;
        const u32 gn = (n + 255) / 256;
        // the transform runs on a work vector owned by the domain: calls on one domain size are serialised (they are
        // synchronous at the ABI anyway), none pays an allocation
        std::lock_guard<std::mutex> g(scratch_mu_);
        if (!d->scratch_rr) MG_HIP(hipMalloc((void **)&d->scratch_rr, (size_t)n * RK * 4));
        u32 *tmp = d->scratch_rr;
        const bool timed = kernel_timing(); // bench.py's NTT leg: HIP events between the kernels of this call
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        if (timed)
            for (auto &e : ev) MG_HIP(hipEventCreate(&e));
        if (timed) MG_HIP(hipEventRecord(ev[0], s));
        const u32 *post = inverse && coset && log_n > 0 ? d->coset_inv_rr : nullptr; // n^-1 g^-i, natural order
        if (log_n > 0) {
            // conversions folded into the first / last pass: arkworks format (bit-reversed gather, coset pre-scaling) -> passes
            // on the work vector -> n^-1 of the plain inverse transform and arkworks format out
            if (timed) MG_HIP(hipEventRecord(ev[1], s));
            NttIo io{d_data, (!inverse && coset) ? d->coset_fwd_rr : (const u32 *)nullptr, d_data,
                     (inverse && !coset) ? d->consts_rr : (const u32 *)nullptr, 0u};
            // (no hazard on d_data: with one pass the single workgroup has the whole vector in LDS before it writes; with several,
            // the first pass only reads it -- into the work vector -- and only the last one writes it)
            run_passes<false>(tmp, tmp, tmp, 1, inverse ? d->tw_inv_rr : d->tw_fwd_rr, log_n, post, s, 1, io);
            if (timed) MG_HIP(hipEventRecord(ev[2], s));
            if (timed) MG_HIP(hipEventRecord(ev[3], s));
        } else {
            hipLaunchKernelGGL((ntt_load_rr_kernel<FrC>), dim3(gn), dim3(256), 0, s, d_data, log_n, (const u32 *)nullptr, tmp);
            if (timed) MG_HIP(hipEventRecord(ev[1], s));
            if (timed) MG_HIP(hipEventRecord(ev[2], s));
            hipLaunchKernelGGL((rr_to_std_kernel<FrC>), dim3(gn), dim3(256), 0, s, tmp, (size_t)n, (const u32 *)nullptr, d_data);
            if (timed) MG_HIP(hipEventRecord(ev[3], s));
        }
        hipError_t e = hipStreamSynchronize(s); // the scratch vector is handed to the next caller after this
        if (timed) {
            float v[4] = {0, 0, 0, 0};
            if (e == hipSuccess) {
                hipEventElapsedTime(&v[0], ev[0], ev[3]);
                hipEventElapsedTime(&v[1], ev[0], ev[1]);
                hipEventElapsedTime(&v[2], ev[1], ev[2]);
                hipEventElapsedTime(&v[3], ev[2], ev[3]);
            }
            std::memcpy(last_times().ntt_ms, v, sizeof(v));
            for (auto &x : ev) hipEventDestroy(x);
        }
        if (e != hipSuccess) {
            set_last_hip_error(e, "ntt transform", __FILE__, __LINE__);
            return MG_ERR_HIP;
        }
        MG_HIP(hipGetLastError());
        return MG_OK;
    }
    // QAP quotient in place on reduced-radix vectors: a, b, c hold the constraint evaluations; on return a holds the
    // coefficients of h = (A B - C)/Z in BIT-REVERSED order (the h-query bases are stored in the same order), < 2p.
    // ifft = DIF (natural -> bit-reversed) with n^-1 g^i folded into its last pass, coset fft = DIT
    // (bit-reversed -> natural): no permutation pass, 2 x ceil(lg/10) launches per transform, a/b/c batched.
    int qap_quotient(u32 *a, u32 *b, u32 *c, unsigned lg, hipStream_t s, u32 batch = 1) override {
        Domain *d;
        int rc = get_domain(lg, &d);
        if (rc) return rc;
        const u32 n = 1u << lg;
        if (lg == 0) { // degenerate domain: h = (a b - c) / (g - 1) scaled as the general path would
            hipLaunchKernelGGL((qap_pointwise_kernel<FrC>), dim3(1, batch), dim3(256), 0, s, a, b, c, d->consts_rr + RK, n);
            MG_HIP(hipGetLastError());
            return MG_OK;
        }
        // single proofs (single-column tiles, two passes per transform): four fused launches instead of seven (MANTA_NTT_FUSE=0: A/B)
        static const int fuse_on = [] { // bit 0: the low passes (ntt_fused_low), bit 1: high pass + pointwise + high pass
            return ab_knob("MANTA_NTT_FUSE", 3) & 3;
        }();
        const unsigned L = lg / 2, H = lg - L; // low / high stages of every transform
        if (fuse_on && lg >= NTT_FUSE_LG_MIN && lg <= NTT_FUSE_LG_MAX && (size_t)batch * 3 * ((size_t)n >> (H + 1)) < 512) {
            static const bool attr_set = [] { // a | b | c tiles of the largest high half
                allow_lds(reinterpret_cast<const void *>(&ntt_fused_high_pw<FrC>), 3 * tile_lds(NTT_FUSE_TILE_LG));
                return true;
            }();
            (void)attr_set;
            // inverse transform, high stages lg .. L + 1 (strided tiles of 2^H), a | b | c
            rr_pass<true>(a, b, c, 3, d->tw_inv_rr, lg, L + 1, H, nullptr, s, batch);
            // its low stages + n^-1 g^i + the forward coset transform's low stages (contiguous tiles of 2^L)
            if (fuse_on & 1) {
                hipLaunchKernelGGL((ntt_fused_low<FrC>), dim3(n >> L, 3, batch), dim3(tile_threads(L)), tile_lds(L), s, a, b, c, d->tw_inv_rr,
                                   d->tw_fwd_rr, lg, L, d->t1_br_rr);
            } else {
                rr_pass<true>(a, b, c, 3, d->tw_inv_rr, lg, 1u, L, d->t1_br_rr, s, batch);
                rr_pass<false>(a, b, c, 3, d->tw_fwd_rr, lg, 1u, L, nullptr, s, batch);
            }
            // forward high stages on a, b, c + (a b - c) / Z + the last inverse transform's high stages
            if (fuse_on & 2) {
                hipLaunchKernelGGL((ntt_fused_high_pw<FrC>), dim3(n >> H, 1, batch), dim3(3 * tile_threads(H)), 3 * tile_lds(H), s, a, b, c,
                                   d->tw_fwd_rr, d->tw_inv_rr, lg, H, d->consts_rr + RK);
            } else {
                rr_pass<false>(a, b, c, 3, d->tw_fwd_rr, lg, L + 1, H, nullptr, s, batch);
                hipLaunchKernelGGL((qap_pointwise_kernel<FrC>), dim3((n + 255) / 256, batch), dim3(256), 0, s, a, b, c, d->consts_rr + RK, n);
                rr_pass<true>(a, a, a, 1, d->tw_inv_rr, lg, L + 1, H, nullptr, s, batch);
            }
            // its low stages + n^-1 g^-i
            rr_pass<true>(a, a, a, 1, d->tw_inv_rr, lg, 1u, L, d->t2_br_rr, s, batch);
            MG_HIP(hipGetLastError());
            return MG_OK;
        }
        run_passes<true>(a, b, c, 3, d->tw_inv_rr, lg, d->t1_br_rr, s, batch);
        run_passes<false>(a, b, c, 3, d->tw_fwd_rr, lg, nullptr, s, batch);
        hipLaunchKernelGGL((qap_pointwise_kernel<FrC>), dim3((n + 255) / 256, batch), dim3(256), 0, s, a, b, c, d->consts_rr + RK, n);
        run_passes<true>(a, a, a, 1, d->tw_inv_rr, lg, d->t2_br_rr, s, batch);
        MG_HIP(hipGetLastError());
        return MG_OK;
    }
    int work_words() const override { return RK; }
    int spmv3(const DevCsr &A, const DevCsr &B, const DevCsr &C, const u32 *d_z, u32 *d_a, u32 *d_b, u32 *d_c, u64 m, u64 P,
              hipStream_t s, u32 batch = 1, size_t z_stride = 0, size_t out_stride = 0, u64 rows_total = 0) override {
        if (rows_total < m + P) rows_total = m + P; // (0: the caller has zeroed the vectors itself)
        if (rows_total == 0) return MG_OK; // (m == 0 with rows to write still launches: the kernel owns the zero rows up to rows_total)
        Csr3 M{{A.row_ptr, B.row_ptr, C.row_ptr}, {A.col, B.col, C.col}, {A.val, B.val, C.val}, {d_a, d_b, d_c}};
        hipLaunchKernelGGL((spmv3_kernel<FrC>), dim3((u32)((rows_total + 255) / 256), batch, 3), dim3(256), 0, s, M, d_z, (u32)m, (u32)P,
                           z_stride, out_stride, (u32)rows_total);
        MG_HIP(hipGetLastError());
        return MG_OK;
    }
    int r1cs_check(const DevCsr &A, const DevCsr &B, const DevCsr &C, const u32 *d_z, u64 m, hipStream_t s, u32 batch, size_t z_stride,
                   u32 *d_first, u32 *d_count) override {
        if (batch == 0) return MG_OK;
        if (batch > FrEngine::R1CS_CHECK_MAX_BATCH || m >= ((u64)1 << 32)) return MG_ERR_ARG; // (the grid's y limit; rows are 32-bit, 2^32 - 1 = "none")
        // the result words, in front of the kernel on its stream (nothing here is ever captured: a memset is fine)
        MG_HIP(hipMemsetAsync(d_first, 0xFF, (size_t)batch * 4, s));
        MG_HIP(hipMemsetAsync(d_count, 0, (size_t)batch * 4, s));
        if (m == 0) return MG_OK; // no row, nothing fails
        Csr3 M{{A.row_ptr, B.row_ptr, C.row_ptr}, {A.col, B.col, C.col}, {A.val, B.val, C.val}, {nullptr, nullptr, nullptr}};
        hipLaunchKernelGGL((r1cs_check_kernel<FrC>), dim3((u32)((m + 255) / 256), batch), dim3(256), 0, s, M, d_z, (u32)m, z_stride, d_first,
                           d_count);
        MG_HIP(hipGetLastError());
        return MG_OK;
    }
    // reduced-radix vector -> arkworks format (tests / mg_witness_map)
    int work_to_std(const u32 *d_rr, size_t n, u32 *d_std, hipStream_t s) override {
        hipLaunchKernelGGL((rr_to_std_kernel<FrC>), dim3((u32)((n + 255) / 256)), dim3(256), 0, s, d_rr, n, (const u32 *)nullptr, d_std);
        MG_HIP(hipGetLastError());
        return MG_OK;
    }
    int domain_twiddles(unsigned log_n, bool inverse, const u32 **d_tw, u64 n_inv_canonical[4]) override {
        Domain *d;
        int rc = get_domain(log_n, &d);
        if (rc) return rc;
        *d_tw = inverse ? d->tw_inv : d->tw_fwd;
        const HF ninv = HF::from_mont(HF::inv(from_u64((u64)1 << log_n)));
        std::memcpy(n_inv_canonical, ninv.v, 32);
        return MG_OK;
    }

  private:
    std::mutex mu_, scratch_mu_;
    std::map<unsigned, Domain> domains_;
};

} // namespace mg
