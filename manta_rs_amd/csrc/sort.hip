// K6: sort of the (bucket key, base index) pairs by key -- a hand-written LSD radix sort for gfx950.
//
// The general-purpose device sort (hipCUB / rocPRIM) takes 0.8 ms for the 16.7 M pairs of a 2^20 MSM. This one
// is specialised to what the MSM needs -- 32-bit pairs, keys of at most 24 significant bits (usually 16 -> two
// 8-bit passes), stable, no temporary beyond a per-tile histogram -- and needs ~0.45 ms of kernel time; in the
// pipelined bench (three MSMs in flight) the two are equal within noise because the step is bounded by the
// accumulate kernel. Per pass:
//   radix_hist     per 4096-element tile, digit counts in LDS (ds_add) -> hist[digit][tile]
//   radix_scan_*   exclusive scan over hist (digit-major): one workgroup per digit row, then the 256 row totals
//   radix_scatter  every wavefront ranks its 1024 elements 64 at a time through a table of 256 lane masks of
//                  its own in LDS: the lanes OR their bit into the mask of their digit (ds_or_b64, nothing
//                  returned) and read it back; an element's rank is the count of the mask's bits below its
//                  lane (v_mbcnt) plus the wave's running count for the digit, and the first lane of a mask
//                  adds the mask's popcount to that count and clears the mask for the next 64. Lanes in lane
//                  order, steps in program order: stable by construction. The masks (4 x 256 x 8 B) lie in
//                  the first 8 KB of the tile buffer, which is not written before the barrier behind the
//                  offset scan, so they add nothing to the kernel's LDS. With -DMG_SCATTER_MASKS=0 the lanes
//                  holding the same digit are found by intersecting eight v_cmp/ballot masks instead
//                  (wave64 "match", ~80 VALU an element against ~10; profiles/radix_scatter_masks_ab.txt).
//                  The tile is then laid out digit-sorted in LDS so that consecutive lanes store to
//                  consecutive addresses within each digit run.
//                  (the body is sort_scatter.h radix_scatter_tile, which the MSM's fused digits_scatter shares)
// 20 B of HBM traffic per element per pass. The only sort on the product path: keys wider than 32 bits' worth of
// 8-bit passes do not occur (msm_launch caps the bucket-key space at 2^24), and no library sort is linked.
#include "sort_scatter.h"
#include <algorithm>
#include <cstdlib>

namespace mg {

// (`count`: when non-null the number of elements is read from the device -- the MSM's digit kernel compacts
// away zero digits and only it knows how many pairs are left; the grid is sized for the maximum and tiles
// beyond the count contribute zero histograms and no elements)
__global__ __launch_bounds__(256) void radix_hist(const u32 *__restrict__ keys, u32 M, int shift, u32 ntiles,
                                                  u32 *__restrict__ hist, const u32 *__restrict__ count, u32 lowmask, u32 inv_from) {
    MG_PRIO_HIGH();
    if (count) M = *count;
    if ((size_t)blockIdx.x * SORT_TILE >= M) { // a tile past the last element: an all-zero histogram column
        hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = 0;
        return;
    }
    __shared__ u32 cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const size_t e = base + (size_t)j * 256 + threadIdx.x;
        if (e < M) atomicAdd(&cnt[(sort_key(keys[e], lowmask, inv_from) >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of every digit row hist[d][0..ntiles) in place (one workgroup per digit) + the row total
__global__ __launch_bounds__(256) void radix_scan_rows(u32 *__restrict__ hist, u32 ntiles, u32 *__restrict__ totals) {
    MG_PRIO_HIGH();
    __shared__ u32 part[256];
    u32 *row = hist + (size_t)blockIdx.x * ntiles;
    const u32 per = (ntiles + 255) / 256;
    const u32 lo = threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
    u32 s = 0;
    for (u32 i = lo; i < hi; ++i) s += row[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const u32 v = threadIdx.x >= (u32)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    u32 run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (u32 i = lo; i < hi; ++i) {
        const u32 c = row[i];
        row[i] = run;
        run += c;
    }
    if (threadIdx.x == 255) totals[blockIdx.x] = part[255];
}
// exclusive scan of the 256 row totals in place
__global__ __launch_bounds__(256) void radix_scan_totals(u32 *__restrict__ totals) {
    MG_PRIO_HIGH();
    __shared__ u32 part[256];
    const u32 mine = totals[threadIdx.x];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const u32 v = threadIdx.x >= (u32)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    totals[threadIdx.x] = part[threadIdx.x] - mine;
}

// One tile of a pass over pairs that lie in memory: sort_scatter.h radix_scatter_tile over LoadedPairs (54 VGPRs).
// IDENT: lowmask == ~0, the sort key is the key itself (a single MSM) and a digit is one bit-field extract of it.
template <bool IDENT>
__global__ __launch_bounds__(256) void radix_scatter(const u32 *__restrict__ keys_in, const u32 *__restrict__ vals_in,
                                                     u32 *__restrict__ keys_out, u32 *__restrict__ vals_out, u32 M,
                                                     int shift, u32 ntiles, const u32 *__restrict__ hist,
                                                     const u32 *__restrict__ totals, const u32 *__restrict__ count, u32 lowmask,
                                                     u32 inv_from) {
    MG_PRIO_HIGH();
    if (count) M = *count;
    if ((size_t)blockIdx.x * SORT_TILE >= M) return; // a tile past the last element
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 tile0 = blockIdx.x * (u32)SORT_TILE; // below M < 2^32
    const u32 mine = wave * (SORT_ITEMS * 64) + lane;
    const LoadedPairs in{keys_in, vals_in, M - tile0 > (u32)SORT_TILE ? (u32)SORT_TILE : M - tile0, mine, (size_t)tile0 + mine, shift, lowmask,
                         inv_from, IDENT};
    radix_scatter_tile(in, keys_out, vals_out, ntiles, hist, totals);
}

// tiles1: the tiles of a first pass that is the caller's own (sort_scratch), where they outnumber the sort's
static size_t hist_columns(size_t n, size_t tiles1) { return std::max((n + SORT_TILE - 1) / SORT_TILE, tiles1); }
size_t sort_pairs_temp_bytes(size_t n, size_t tiles1) {
    return 2 * n * 4 /* ping-pong pair */ + 256 * hist_columns(n, tiles1) * 4 + 256 * 4 + 256;
}
SortScratch sort_scratch(void *tmp, size_t n, size_t tiles1) {
    u32 *const tk = (u32 *)tmp, *const hist = tk + 2 * n;
    return SortScratch{tk, tk + n, hist, hist + (size_t)256 * hist_columns(n, tiles1)};
}
void sort_scan_hist(const SortScratch &t, u32 ntiles, hipStream_t s) {
    hipLaunchKernelGGL(radix_scan_rows, dim3(256), dim3(256), 0, s, t.hist, ntiles, t.totals);
    hipLaunchKernelGGL(radix_scan_totals, dim3(1), dim3(256), 0, s, t.totals);
}

bool sort_pairs_takes_device_count(int end_bit) { return end_bit >= 1 && end_bit <= 32; }

int sort_pairs(const u32 *keys_in, u32 *keys_out, const u32 *vals_in, u32 *vals_out, size_t n, int end_bit,
               void *tmp, size_t tmp_bytes, hipStream_t s, const u32 *d_count, u32 lowmask, u32 inv_from, int first_pass,
               size_t tiles1) {
    if (n == 0) return MG_OK;
    if (end_bit < 1 || end_bit > 32 || n >= (1ull << 32) || tmp_bytes < sort_pairs_temp_bytes(n, tiles1) || first_pass < 0) return MG_ERR_ARG;
    const u32 M = (u32)n;
    const u32 ntiles = (u32)((n + SORT_TILE - 1) / SORT_TILE);
    const int passes = (end_bit + 7) / 8;
    // ping-pong so that the LAST pass lands in (keys_out, vals_out): with an even number of passes the first
    // one writes to the scratch pair
    const SortScratch t = sort_scratch(tmp, n, tiles1);
    u32 *const tk = t.keys, *const tv = t.vals, *const hist = t.hist, *const totals = t.totals;
    const u32 *ik = keys_in, *iv = vals_in;
    for (int p = first_pass; p < passes; ++p) {
        const bool to_out = ((passes - 1 - p) % 2) == 0;
        u32 *ok = to_out ? keys_out : tk, *ov = to_out ? vals_out : tv;
        hipLaunchKernelGGL(radix_hist, dim3(ntiles), dim3(256), 0, s, ik, M, 8 * p, ntiles, hist, d_count, lowmask, inv_from);
        sort_scan_hist(t, ntiles, s);
        hipLaunchKernelGGL(lowmask == 0xffffffffu ? radix_scatter<true> : radix_scatter<false>, dim3(ntiles), dim3(256), 0, s, ik, iv, ok, ov, M,
                           8 * p, ntiles, hist, totals, d_count, lowmask, inv_from);
        ik = ok;
        iv = ov;
    }
    MG_HIP(hipGetLastError());
    return MG_OK;
}

} // namespace mg
