// K6, the device side shared by sort.hip and msm_digits.h: the tile geometry, the key a pass sorts by, and the body of a radix
// scatter -- rank, lay the tile out digit-sorted in LDS, store -- over a tile whose (key, value) pairs come from a policy: loaded
// from the unsorted arrays (radix_scatter, sort.hip) or computed from the tile's scalars (digits_scatter, msm_digits.h). The
// lane-mask ranking exists here and nowhere else.
#pragma once
#include "engine.h"

namespace mg {

static constexpr int SORT_TILE = 4096; // elements per workgroup: 4 waves x 16 items x 64 lanes
static constexpr int SORT_ITEMS = 16;

// The key a pass sorts by. Normally the key itself. Batched MSMs in the fixed layout arrive proof-major (vector q's pairs, then
// vector q + 1's) with key = q * seg + bucket, seg a power of two: a STABLE sort by the bucket bits alone leaves every (q, bucket)
// run contiguous -- order (bucket, q) instead of (q, bucket), which the run-detecting consumers do not care about -- and saves the
// passes over the vector bits (the dense h MSM of 32 proofs: 14 bits = two passes instead of 19 = three over 40 M pairs). Keys
// from `inv_from` up (the invalid key of zero digits) sort behind every bucket. lowmask = ~0: the identity -- there is no value
// behind the masked keys then, and lowmask + 1 would send the key ~0 to the FRONT of a 32-bit sort.
__device__ __forceinline__ u32 sort_key(u32 k, u32 lowmask, u32 inv_from) {
    return (k >= inv_from && lowmask != 0xffffffffu) ? lowmask + 1u : (k & lowmask);
}

// MG_SCATTER_MASKS (default 1): the ranking inside a wave-step goes through the per-wave LDS lane masks; 0: the eight-ballot
// "match" (an A/B twin through tools/build_variant.sh; both are measured in profiles/radix_scatter_masks_ab.txt).
#ifndef MG_SCATTER_MASKS
#define MG_SCATTER_MASKS 1
#endif

// The pairs of a tile as the scatter body sees them. Item j of lane l of wave w is element w * 1024 + j * 64 + l of the tile's
// unsorted order. A policy provides
//   u32  left                    the tile's elements (what the body places and stores)
//   bool valid(j)                whether this lane's item j is one of them
//   void keys(k)                 k[j] = the item's key word for every valid item (any word digit() and key() understand), else 0
//   void vals(v, k)              v[j] = the item's value, asked for behind the ranking
//   u32  digit(word), key(word)  the radix digit of a key word; the key that is stored
// An item that is not valid sets no bit of a lane mask and clears none. That is safe wherever the valid items of a wave-step are
// its lowest lanes (a partial last tile) or none at all (a step past a tile's last item): a mask's first lane is then valid.
struct LoadedPairs {
    const u32 *__restrict__ keys_in, *__restrict__ vals_in;
    u32 left, mine; // mine: the tile-local index of this lane's item 0
    size_t base;    // its index in the arrays
    int shift;
    u32 lowmask, inv_from;
    bool ident; // lowmask == ~0: the sort key is the key itself (a single MSM) and a digit is one bit-field extract of it
    __device__ __forceinline__ bool valid(int j) const { return mine + (u32)j * 64 < left; }
    __device__ __forceinline__ void keys(u32 (&k)[SORT_ITEMS]) const {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) k[j] = valid(j) ? keys_in[base + (size_t)j * 64] : 0u;
    }
    __device__ __forceinline__ void vals(u32 (&v)[SORT_ITEMS], const u32 (&)[SORT_ITEMS]) const {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; ++j) v[j] = valid(j) ? vals_in[base + (size_t)j * 64] : 0u;
    }
    __device__ __forceinline__ u32 digit(u32 word) const { return ((ident ? word : sort_key(word, lowmask, inv_from)) >> shift) & 255u; }
    __device__ __forceinline__ u32 key(u32 word) const { return word; }
};

// Register budget: at most 64 VGPRs, so that a workgroup finds room on a SIMD beside two resident BLS12-381 accumulate
// wavefronts. A lane keeps its 16 key words and, two to a register, their 16 ranks across the ranking; the
// 16 values are requested behind it and arrive during the offset scan.
// hist / totals: the scanned histogram of the pass (radix_scan_rows, radix_scan_totals), digit-major, `ntiles` columns.
template <class Pairs>
__device__ __forceinline__ void radix_scatter_tile(const Pairs &in, u32 *__restrict__ keys_out, u32 *__restrict__ vals_out, u32 ntiles,
                                                   const u32 *__restrict__ hist, const u32 *__restrict__ totals) {
    __shared__ u32 wcount[4][256]; // per-wave running digit counts, then per-wave tile-local offsets
    __shared__ u32 gbase[256];     // global position of the tile's first element of each digit, minus its local offset
    // the tile, locally sorted by digit (stable): 4096 keys, then 4096 values. Up to the barrier behind the offset scan its first
    // 8 KB are the lane masks of the ranking, [wave][digit]: bit l is set while lane l of the wave-step in hand holds that digit
    typedef unsigned long long __attribute__((may_alias)) lane_mask;
    __shared__ __attribute__((aligned(8))) u32 tile[2 * SORT_TILE];
    u32 *const sk = tile, *const sv = tile + SORT_TILE;
    lane_mask *const masks = (lane_mask *)tile;
    constexpr int HALF = SORT_ITEMS / 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        wcount[w][threadIdx.x] = 0;
        if (MG_SCATTER_MASKS) masks[w * 256 + threadIdx.x] = 0;
    }
    __syncthreads();
    const u32 left = in.left;
    u32 k[SORT_ITEMS], rk2[HALF]; // rk2[j / 2]: the ranks (< 1024) of items j (low half) and j + 1
    in.keys(k);
#if MG_SCATTER_MASKS
    // The rank of an item inside its wave-step is the number of lower lanes that hold its digit. Every valid lane ORs its bit into
    // the digit's mask, reads the mask back and counts the bits below its own; the first of the peers adds all of them to the
    // wave's count and clears the mask for the next step. Lanes without an item set no bit and clear nothing (see the policy
    // contract above: a mask's first lane is never one of them). The LDS executes one wavefront's operations in program
    // order, so OR -> read -> clear needs no barrier; the wavefront-scope fences only keep the compiler from moving or merging them.
    lane_mask *const wmask = masks + wave * 256;
    const unsigned long long lane_bit = 1ull << lane;
    unsigned long long none = 0;
    asm volatile("" : "+v"(none)); // the cleared mask in a register pair: as a constant it is materialised again for every item
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const bool valid = in.valid(j);
        const u32 d = in.digit(k[j]);
        if (valid) __hip_atomic_fetch_or(&wmask[d], lane_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const unsigned long long peers = __hip_atomic_load(&wmask[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        const u32 before = wcount[wave][d]; // every peer reads the count, then the first peer bumps it
        const u32 lo = (u32)peers, hi = (u32)(peers >> 32);
        const u32 rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, before)); // + the peers in the lanes below
        const bool first = valid && rank == before;
        if (j & 1)
            rk2[j >> 1] |= rank << 16;
        else
            rk2[j >> 1] = rank;
        asm volatile("" : "+v"(rk2[j >> 1])); // packed here and now: left to itself the compiler carries the ranks unpacked to the placement
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (first) {
            wcount[wave][d] = (u32)__builtin_popcount(hi) + ((u32)__builtin_popcount(lo) + before);
            __hip_atomic_store(&wmask[d], none, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
#else
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const bool valid = in.valid(j);
        const u32 d = in.digit(k[j]);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bb = __ballot(bit);
            peers &= bit ? bb : ~bb;
        }
        const u32 before = wcount[wave][d]; // every peer reads the count, then the first peer bumps it
        const u32 r = (u32)__popcll(peers & lt_mask);
        if (j & 1)
            rk2[j >> 1] |= (before + r) << 16;
        else
            rk2[j >> 1] = before + r;
        asm volatile("" : "+v"(rk2[j >> 1])); // packed here and now: left to itself the compiler carries `before` and `r` to the placement
        if (valid && r == 0) wcount[wave][d] = before + (u32)__popcll(peers);
    }
#endif
    // (the digits are worked out again behind the scan, from keys the compiler cannot see through: it would otherwise keep all 16
    // digit addresses of the ranking alive beside the keys)
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) asm volatile("" : "+v"(k[j]));
    u32 v[SORT_ITEMS]; // requested here, in flight across the scan
    in.vals(v, k);
    __syncthreads();
    { // tile-local exclusive offsets: digit-major, wave-minor (stable); one thread per digit + a 256-wide scan
        const u32 d = threadIdx.x;
        const u32 c0 = wcount[0][d], c1 = wcount[1][d], c2 = wcount[2][d], c3 = wcount[3][d];
        const u32 tot = c0 + c1 + c2 + c3;
        gbase[d] = tot;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            const u32 x = d >= (u32)s ? gbase[d - s] : 0;
            __syncthreads();
            gbase[d] += x;
            __syncthreads();
        }
        const u32 loc = gbase[d] - tot; // exclusive local offset of digit d
        __syncthreads();
        wcount[0][d] = loc;
        wcount[1][d] = loc + c0;
        wcount[2][d] = loc + c0 + c1;
        wcount[3][d] = loc + c0 + c1 + c2;
        gbase[d] = hist[(size_t)d * ntiles + blockIdx.x] + totals[d] - loc;
    }
    __syncthreads(); // every wavefront is past its ranking: the lane masks are dead and the tile may be written
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        if (in.valid(j)) {
            const u32 rank = (j & 1) ? rk2[j >> 1] >> 16 : rk2[j >> 1] & 0xffffu;
            const u32 lp = wcount[wave][in.digit(k[j])] + rank;
            sk[lp] = in.key(k[j]);
            sv[lp] = v[j];
        }
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < left; t += 256) { // consecutive lanes -> consecutive addresses within a digit run
        const u32 kk = sk[t];
        const u32 pos = gbase[in.digit(kk)] + t;
        keys_out[pos] = kk;
        vals_out[pos] = sv[t];
    }
}

} // namespace mg
