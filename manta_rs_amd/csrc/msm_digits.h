// Pippenger MSM, stage K5: scalars -> signed window digits -> (bucket key, base index | sign) pairs. Part of msm_impl.h.
#pragma once
#include "msm_common.h"
#include "sort_scatter.h"

namespace mg {

// --------------------------------------------------------------------------------------------
// K5: digits
// --------------------------------------------------------------------------------------------
// The scalar a lane recodes: loaded and converted by `mont` (0: the integer itself, 1: arkworks Montgomery words, 2: the witness
// map's reduced-radix work form), reduced below r and folded to the smaller of k and r - k; s = 0 without a scalar (`have`
// false). flip = 1 if r - k was taken. Every lane of a wavefront calls it together: the reduction loop leaves wave-uniformly.
// Shared by digits_kernel and the fused pair digits_hist / digits_scatter. WORK = false compiles the work form out (the fused
// kernels are never launched on it). All three kernels have to stay within 64 VGPRs, and the allocation
// follows the shape of this function: with `flip` as the return value digits_kernel came to 76 and the fused pair to 58 / 61,
// with the reference 54 and 46 / 52 (hipcc -Rpass-analysis=kernel-resource-usage; profiles/dense_front_ab.txt).
template <class FrC, bool WORK = true>
__device__ __forceinline__ void folded_scalar(const u32 *__restrict__ scalars, u32 src, bool have, int mont, u32 (&s)[8], u32 &flip) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0;
    if (WORK && have && mont == 2) { // the witness map's reduced-radix work form (9 words): one product with the integer 1
        typedef FpR<FrC> R;
        const Fp<FrC> f = R::load(scalars + (size_t)src * R::K).to_canonical();
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = f.v[j];
    } else if (have) {
        const uint4 *p = reinterpret_cast<const uint4 *>(scalars + (size_t)src * 8);
        uint4 a = p[0], b = p[1];
        s[0] = a.x, s[1] = a.y, s[2] = a.z, s[3] = a.w, s[4] = b.x, s[5] = b.y, s[6] = b.z, s[7] = b.w;
        if (mont) { // ark-ff into_repr on the device
            Fp<FrC> f;
#pragma unroll
            for (int j = 0; j < 8; ++j) f.v[j] = s[j];
            f = Fp<FrC>::from_mont(f);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = f.v[j];
        }
    }
    // k P = (r - k)(-P): the smaller of k and r - k is below 2^(BITS - 1), so ceil(BITS / c) signed windows hold it -- one fewer
    // than the ceil((BITS + 1) / c) a scalar up to r - 1 needs whenever c divides BITS (BLS12-381, 255 bits: 15 windows of 17
    // bits instead of 16). The sign of every digit flips with the scalar.
    // A scalar that is NOT below r (the ABI says canonical, arkworks' multi_scalar_mul takes any BigInteger256 and treats it as
    // the integer it is) is first reduced: k P = (k mod r) P, and 2^256 < 6 r on both curves. Without this its top window could
    // exceed B and drop a carry. Wave-uniform early exit: canonical input pays one borrow chain.
    for (int it = 0; it < 6; ++it) {
        u32 t[8], bw = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const u64 d = (u64)s[j] - FrC::P[j] - bw;
            t[j] = (u32)d;
            bw = (u32)(d >> 63);
        }
        if (!__any(!bw)) break; // every lane's scalar is below r
        if (!bw) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = t[j];
        }
    }
    flip = 0;
    {
        u32 t[8], bw = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const u64 d = (u64)FrC::P[j] - s[j] - bw;
            t[j] = (u32)d;
            bw = (u32)(d >> 63);
        }
        bool lt = false; // r - k < k
#pragma unroll
        for (int j = 0; j < 8; ++j) lt = t[j] != s[j] ? t[j] < s[j] : lt;
        if (!bw && lt) {
            flip = 1;
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = t[j];
        }
    }
}
// The signed c-bit digits of a folded scalar, lowest window first. next(): the magnitude of the next window's digit (0 = nothing
// to add) and whether it is negative -- a window value above B = 2^(c-1) borrows 2^c from the next window -- then the scalar moves
// right by c: eight funnel shifts instead of a dynamically indexed limb pair (~90 instructions per window in selects, which made
// the digit kernel issue-bound at 5k instructions per scalar: 172 -> 127 us for 32 x 2^15 scalars, 40 -> 23 us for one 2^15)
struct DigitWalk {
    int c;
    u32 B, carry = 0;
    __device__ __forceinline__ DigitWalk(int c_, u32 B_) : c(c_), B(B_) {}
    __device__ __forceinline__ u32 next(u32 (&t)[8], u32 &neg) {
        const u32 d = (t[0] & ((1u << c) - 1)) + carry;
#pragma unroll
        for (int j = 0; j < 7; ++j) t[j] = __funnelshift_r(t[j], t[j + 1], c);
        t[7] >>= c;
        neg = d > B;
        carry = neg;
        return neg ? (1u << c) - d : d;
    }
};

// One lane per (stored base, scalar vector of the batch): W signed c-bit digits -> (bucket key, base index | sign)
// pairs. Zero digits produce NO pair: real witnesses are 40 % zeros and 25 % ones, so two thirds of all digits
// vanish here instead of being carried through the sort. The surviving pairs are appended to the arrays in
// wave-sized, window-major groups (one atomicAdd on `count` per wavefront, positions by ballot/popcount: the
// order is irrelevant, the sort follows); every later stage reads the pair count from the device.
// (A count -> scan -> write version without the atomic was measured too: the kernel is bound by the scalar loads and the
// Montgomery conversion, not by the append, so running it twice costs more than the atomics do -- 2 x 105 + 46 us against
// 127 us for 32 x 2^15 scalars.)
// count == nullptr selects the fixed layout o = w*n + i with an `invalid` key for zero digits (library-sort path).
template <class FrC>
__global__ __launch_bounds__(1024) void digits_kernel(const u32 *__restrict__ scalars, u32 n, int c, int W, u32 B,
                                                     int precomp, u32 tstride, int mont, u32 invalid,
                                                     u32 *__restrict__ keys, u32 *__restrict__ vals,
                                                     const u32 *__restrict__ map, u32 n_scalars,
                                                     size_t scalar_stride, u32 seg_keys, u32 *__restrict__ count,
                                                     u32 n_sets = 1, u32 set_len = 0, u32 i_first = 0) {
    MG_PRIO_HIGH();
    const u32 i = i_first + blockIdx.x * blockDim.x + threadIdx.x; // (i_first: one launch per query, lanes [i_first, n))
    // blockIdx.y = scalar vector of a batch: its own scalars, its own range of bucket keys; the bases (and so
    // the values) are shared
    scalars += (size_t)blockIdx.y * scalar_stride;
    u32 src = (i < n) ? (map ? map[i] : i) : 0xffffffffu; // which scalar belongs to stored base i
    // concatenated queries (BaseSet::n_sets): original entry j = query j / set_len, scalar j % set_len; every (vector, query)
    // pair has its own range of bucket keys
    u32 set = 0;
    if (n_sets > 1 && i < n) {
        set = src / set_len;
        src -= set * set_len;
    }
    const u32 key0 = (blockIdx.y * n_sets + set) * seg_keys;
    const bool have = i < n && src < n_scalars; // the scalar vector may be shorter than the base set: zip
    u32 s[8];
    u32 flip;
    folded_scalar<FrC>(scalars, src, have, mont, s, flip);
    DigitWalk walk(c, B);
    u32 neg;
    if (!count) { // fixed layout
        if (i >= n) return;
        keys += (size_t)blockIdx.y * W * n;
        vals += (size_t)blockIdx.y * W * n;
        for (int w = 0; w < W; ++w) {
            const u32 d = walk.next(s, neg); // s = 0 without a scalar
            const size_t o = (size_t)w * n + i;
            keys[o] = d ? key0 + (precomp == 2 ? 0u : precomp ? (d - 1) : ((u32)w * B + d - 1)) : invalid;
            vals[o] = d ? ((precomp == 2 ? ((u32)w * tstride + i) * B + (d - 1) : precomp ? ((u32)w * tstride + i) : i) | ((neg ^ flip) << 31)) : 0;
        }
        return;
    }
    // pass 1: how many pairs does this wavefront produce
    const int lane = threadIdx.x & 63;
    u32 total = 0;
    {
        u32 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = s[j];
        DigitWalk count_walk(c, B);
        for (int w = 0; w < W; ++w) total += (u32)__popcll(__ballot(count_walk.next(t, neg) != 0));
    }
    // one atomic per WORKGROUP (up to sixteen wavefronts add up through LDS): the counter is a single address shared
    // by the whole grid, and atomics on it serialise at ~50 ns each -- one per wavefront (16 384 at 2^20 scalars) made the
    // kernel 0.41 ms, one per 256 threads 0.28 ms
    __shared__ u32 wave_tot[16], block_base;
    const int wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    if (lane == 0) wave_tot[wv] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 t = 0;
        for (int q = 0; q < nwv; ++q) t += wave_tot[q];
        block_base = t ? atomicAdd(count, t) : 0;
    }
    __syncthreads();
    u32 base = block_base;
    for (int q = 0; q < wv; ++q) base += wave_tot[q];
    // pass 2: write them, window-major inside the wavefront's slice
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int w = 0; w < W; ++w) {
        const u32 d = walk.next(s, neg);
        const unsigned long long m = __ballot(d != 0);
        if (d) {
            const u32 o = base + (u32)__popcll(m & lt);
            keys[o] = key0 + (precomp == 2 ? 0u : precomp ? (d - 1) : ((u32)w * B + d - 1));
            vals[o] = (precomp == 2 ? ((u32)w * tstride + i) * B + (d - 1) : precomp ? ((u32)w * tstride + i) : i) | ((neg ^ flip) << 31);
        }
        base += (u32)__popcll(m);
    }
}

// --------------------------------------------------------------------------------------------
// K5 + the first pass of K6, fused: a dense single MSM on window tables
// --------------------------------------------------------------------------------------------
// One scalar vector against window tables, W <= SORT_ITEMS windows, no compaction asked for (GroupEngineT::dense_front). The
// unsorted pair stream is never written: a tile of the first radix pass is 256 scalars x W pairs, a lane holds one scalar and
// its W digits as its items, and both kernels of the pass recompute the digits from the scalars (8 KB a tile instead of up to
// 32 KB of pairs written once and read twice).
//   digits_hist     the tile's counts of the low key byte, in the layout radix_scan_rows takes: hist[digit][tile]
//   digits_scatter  the same digits again, ranked and scattered by sort_scatter.h radix_scatter_tile
// A zero digit is the pair (key 0, inf_index): the all-zero record bases_create leaves behind the last window table, which the
// accumulate kernel's mixed addition skips at its first test. So the pair count is n W, known on the host: no device counter, no
// `invalid` key (and with 2^16 buckets no third radix pass for it), no second walk over the digits. Uniform scalars have one
// zero digit in 2^17.
struct DenseFront {
    const u32 *scalars, *map; // map: stored base i takes scalar map[i] (or nullptr)
    u32 n, n_scalars;         // stored bases = lanes; scalars (the vector may be shorter than the base set: zip)
    int c, W, mont;            // mont: 0 the integers themselves, 1 Montgomery words (the work form does not come here)
    u32 B, tstride, inf_index; // table w starts tstride records behind table w - 1
};
static_assert(MSM_DENSE_MAX_WINDOWS == SORT_ITEMS, "a lane's items are its scalar's windows");
// the key word of an item across the ranking: the key (digit magnitude - 1, below 2^24) | DIGIT_ZERO | DIGIT_NEG
static constexpr u32 DIGIT_ZERO = 1u << 30, DIGIT_NEG = 1u << 31;
// each(j, word) for the windows j < W of this lane's scalar; false: the lane is past the last stored base (no item is valid)
template <class FrC, class Each> __device__ __forceinline__ bool dense_digit_words(const DenseFront &a, Each each) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    const u32 src = i < a.n ? (a.map ? a.map[i] : i) : 0xffffffffu;
    u32 s[8];
    u32 flip;
    folded_scalar<FrC, false>(a.scalars, src, i < a.n && src < a.n_scalars, a.mont, s, flip);
    DigitWalk walk(a.c, a.B);
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        if (j >= a.W) break;
        u32 neg;
        const u32 d = walk.next(s, neg);
        each(j, d ? (d - 1) | ((neg ^ flip) << 31) : DIGIT_ZERO);
    }
    return i < a.n;
}
template <class FrC>
__global__ __launch_bounds__(256) void digits_hist(DenseFront a, u32 ntiles, u32 *__restrict__ hist) {
    MG_PRIO_HIGH();
    __shared__ u32 cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const bool lane_valid = blockIdx.x * 256u + threadIdx.x < a.n;
    dense_digit_words<FrC>(a, [&](int, u32 word) {
        if (lane_valid) atomicAdd(&cnt[word & 255u], 1u);
    });
    __syncthreads();
    hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}
// sort_scatter.h's policy over computed pairs: item j = window j. The lanes past the last stored base are the highest lanes of
// the last tile and the steps j >= W have no valid lane at all, as radix_scatter_tile's ranking requires.
template <class FrC> struct DigitPairs {
    const DenseFront &a;
    u32 left, i;
    __device__ __forceinline__ bool valid(int j) const { return i < a.n && j < a.W; }
    __device__ __forceinline__ void keys(u32 (&k)[SORT_ITEMS]) const {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) k[j] = 0;
        dense_digit_words<FrC>(a, [&](int j, u32 word) { k[j] = word; });
    }
    __device__ __forceinline__ void vals(u32 (&v)[SORT_ITEMS], const u32 (&k)[SORT_ITEMS]) const {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) v[j] = (k[j] & DIGIT_ZERO) ? a.inf_index : (((u32)j * a.tstride + i) | (k[j] & DIGIT_NEG));
    }
    __device__ __forceinline__ u32 digit(u32 word) const { return word & 255u; }
    __device__ __forceinline__ u32 key(u32 word) const { return word & 0x00ffffffu; }
};
template <class FrC>
__global__ __launch_bounds__(256) void digits_scatter(DenseFront a, u32 ntiles, const u32 *__restrict__ hist,
                                                      const u32 *__restrict__ totals, u32 *__restrict__ keys_out,
                                                      u32 *__restrict__ vals_out) {
    MG_PRIO_HIGH();
    const u32 first = blockIdx.x * 256u, lanes = a.n - first > 256u ? 256u : a.n - first; // the grid is cdiv(n, 256): first < n
    const DigitPairs<FrC> in{a, lanes * (u32)a.W, first + threadIdx.x};
    radix_scatter_tile(in, keys_out, vals_out, ntiles, hist, totals);
}

} // namespace mg
