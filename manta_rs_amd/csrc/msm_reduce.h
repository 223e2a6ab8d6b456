// Pippenger MSM, stages K7b / K8 / K9: merge of partial runs, bucket reduce (scan tiles, work-efficient front levels),
// device-side fold of the window sums. Part of msm_impl.h.
// Every kernel of K7b / K8 exists twice, `x` and `x_coop`: ONE body (x_body) instantiated with the two TailAdd policies below.
#pragma once
#include "msm_common.h"

namespace mg {

// --------------------------------------------------------------------------------------------
// How a tail kernel adds, and which hardware unit is one 64-lane "logical wave" of its algorithm.
//   plain        one wavefront per logical wave; every lane adds and stores for itself. For the levels with many waves.
//   cooperative  one 256-thread workgroup per logical wave: its four wavefronts hold identical copies of the lanes' state and
//                share every addition (CoopAdd, ec_dev.h: 4 product-times instead of 14), wavefront 0 stores. For the levels
//                with few waves, which are nothing but chains of dependent additions. The addition contains barriers, so
//                every lane of the workgroup calls add_if, in loops whose trip count is the same for all of them (UNIFORM:
//                the two serial loops, which the plain kernels leave as soon as a lane's entries end, run masked instead).
// --------------------------------------------------------------------------------------------
template <class F, bool COOP> struct TailAdd;
template <class F> struct TailAdd<F, false> {
    static constexpr bool UNIFORM = false;
    const int lane = threadIdx.x & 63;
    MG_DEV u32 unit() const { return blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }
    MG_DEV bool writer() const { return true; }
    MG_DEV void add_if(XYZZ<F> &acc, const XYZZ<F> &o, bool take) const {
        if (take) acc.add(o);
    }
    MG_DEV void publish() const {} // a lane re-reads only what it stored itself
};
template <class F> struct TailAdd<F, true> {
    static constexpr bool UNIFORM = true;
    u32 *lds; // CoopAdd<F>::LDS_WORDS words
    const int lane = threadIdx.x & 63, pw = threadIdx.x >> 6;
    MG_DEV u32 unit() const { return blockIdx.x; }
    MG_DEV bool writer() const { return pw == 0; }
    MG_DEV void add_if(XYZZ<F> &acc, XYZZ<F> o, bool take) const {
        if (!take) o = XYZZ<F>::inf();
        CoopAdd<F>::add(acc, o, lds, pw, lane);
    }
    MG_DEV void publish() const { // what the writer stored is re-read by all four wavefronts
        __threadfence_block();
        __syncthreads();
    }
};

// --------------------------------------------------------------------------------------------
// K7b: merge of partials. The partial array is a key-sorted sequence of (key, point) entries, two per
// producer (head run, tail run; a producer whose whole range was one run emits (key, sum), (key, inf)).
// Every lane first folds G consecutive entries serially -- work-efficient: one addition per entry, and none at
// all for G = 2 on accumulate output, where the pair never shares a summable key -- which leaves it with a
// head run (parked in its own consumed input slot) and a tail run, or one run that spans the lane. The wave then
// runs ONE segmented scan over the tail runs (a run only crosses a lane if that lane is a single run, so
// equality of the sorted tail keys at distance d is the segment test) and one fix-up addition for the head
// runs. Runs that end inside the wave and do not touch its first element go to their bucket; the wave's first
// and last runs become the next level's two entries. 64*G entries -> 2 per wave.
// --------------------------------------------------------------------------------------------
template <class F, class A>
MG_DEV void merge_body(const A a, u32 *__restrict__ pkeys, u32 *__restrict__ ppts, u32 cnt, u32 G, u32 invalid, int final_level,
                       u32 *__restrict__ buckets, u32 *__restrict__ okeys, u32 *__restrict__ opts, u32 *__restrict__ std_final) {
    constexpr size_t XW = XYZZ<F>::WORDS;
    const u32 wave = a.unit();
    const int lane = a.lane;
    const size_t b = ((size_t)wave * 64 + lane) * G;
    u32 kh = invalid, cur = invalid; // keys of the lane's first and current run
    bool single = true, open = false; // the lane holds one run only; it still has valid entries ahead
    XYZZ<F> acc = XYZZ<F>::inf();     // sum of the current run
    if (b < cnt) {
        cur = pkeys[b];
        if (cur != invalid) {
            kh = cur;
            acc = XYZZ<F>::load(ppts + b * XW);
            open = true;
        }
    }
    // a run that ends inside the lane: the first one is parked in slot b (already consumed; pkeys[b] == kh), later ones are complete;
    // an invalid key ends the lane (sorted last)
    if constexpr (A::UNIFORM) {
        for (u32 off = 1; off < G; ++off) {
            const size_t j = b + off;
            const bool have = open && j < cnt;
            const u32 k = have ? pkeys[j] : invalid;
            XYZZ<F> p = XYZZ<F>::inf();
            if (have && k != invalid) p = XYZZ<F>::load(ppts + j * XW);
            const bool same = have && k == cur;
            if (have && k != cur) {
                if (a.writer()) acc.store(single ? ppts + b * XW : buckets + (size_t)cur * XW);
                single = false;
                cur = k;
                acc = p;
                if (k == invalid) open = false;
            }
            if (__any(same && !p.is_inf())) a.add_if(acc, p, same);
        }
    } else if (open) {
        const size_t end = b + G < cnt ? b + G : cnt;
        for (size_t j = b + 1; j < end; ++j) {
            const u32 k = pkeys[j];
            if (k != cur) {
                if (single) {
                    acc.store(ppts + b * XW);
                    single = false;
                } else {
                    acc.store(buckets + (size_t)cur * XW);
                }
                cur = k;
                acc = XYZZ<F>::inf();
                if (k == invalid) break;
                acc = XYZZ<F>::load(ppts + j * XW);
            } else {
                const XYZZ<F> p = XYZZ<F>::load(ppts + j * XW);
                if (!p.is_inf()) acc.add(p);
            }
        }
    }
    const u32 kt = cur; // key of the lane's last run, acc its sum
    a.publish();
    // inclusive segmented scan over (kt, acc)
    for (int d = 1; d < 64; d <<= 1) {
        const u32 nk = __shfl_up(kt, d, 64);
        const bool take = (lane >= d) && (nk == kt) && (kt != invalid);
        if (!__any(take)) break;
        a.add_if(acc, XYZZ<F>::shfl(acc, lane - d < 0 ? lane : lane - d), take);
    }
    const u32 prev_kt = __shfl_up(kt, 1, 64), next_kh = __shfl_down(kh, 1, 64);
    const u32 key0 = __shfl(kh, 0, 64);
    const bool need_in = !single && lane > 0 && prev_kt == kh; // the previous lane's last run flows into my head run
    const bool any_in = __any(need_in);
    XYZZ<F> prev = XYZZ<F>::inf();
    if (any_in) prev = XYZZ<F>::shfl(acc, lane > 0 ? lane - 1 : 0);
    // the run that ends at this lane's right edge
    const bool cont = lane < 63 && next_kh == kt;
    if (a.writer() && kt != invalid && !cont) {
        if (final_level) {
            // (std_final: one key in all -- a single MSM on full tables --, the last run IS the result: it leaves in the host's format)
            if (std_final) acc.store_std(std_final + (size_t)kt * XYZZ<typename F::Std>::WORDS);
            else acc.store(buckets + (size_t)kt * XW);
        } else if (kt == key0) {
            okeys[2 * wave] = kt;
            acc.store(opts + (size_t)(2 * wave) * XW);
            if (lane == 63) { // the whole wave is one run
                okeys[2 * wave + 1] = kt;
                XYZZ<F>::inf().store(opts + (size_t)(2 * wave + 1) * XW);
            }
        } else if (lane == 63) {
            okeys[2 * wave + 1] = kt;
            acc.store(opts + (size_t)(2 * wave + 1) * XW);
        } else {
            acc.store(buckets + (size_t)kt * XW);
        }
    }
    if (a.writer() && !final_level && lane == 63 && kt == invalid) { // all further entries are invalid too (sorted last)
        okeys[2 * wave + 1] = invalid;
        if (key0 == invalid) okeys[2 * wave] = invalid;
    }
    // the head run of a lane with several runs ends inside the lane
    XYZZ<F> h = XYZZ<F>::inf();
    if (!single) h = XYZZ<F>::load(ppts + b * XW);
    if (any_in) a.add_if(h, prev, need_in);
    if (a.writer() && !single) {
        if (!final_level && kh == key0) {
            okeys[2 * wave] = kh;
            h.store(opts + (size_t)(2 * wave) * XW);
        } else if (final_level && std_final) {
            h.store_std(std_final + (size_t)kh * XYZZ<typename F::Std>::WORDS);
        } else {
            h.store(buckets + (size_t)kh * XW);
        }
    }
}
template <class F>
__global__ __launch_bounds__(256) MG_TAIL_ATTR void merge_partials(u32 *__restrict__ pkeys, u32 *__restrict__ ppts, u32 cnt, u32 G,
                                                      u32 invalid, int final_level, u32 *__restrict__ buckets,
                                                      u32 *__restrict__ okeys, u32 *__restrict__ opts, u32 n_waves,
                                                      u32 *__restrict__ std_final) {
    MG_PRIO_FOR(F);
    const TailAdd<F, false> a{};
    if (a.unit() >= n_waves) return; // the grid is rounded up to four wavefronts per workgroup
    merge_body<F>(a, pkeys, ppts, cnt, G, invalid, final_level, buckets, okeys, opts, std_final);
}
template <class F>
__global__ __launch_bounds__(256) MG_TAIL_COOP_ATTR void merge_partials_coop(u32 *__restrict__ pkeys, u32 *__restrict__ ppts, u32 cnt, u32 G,
                                                           u32 invalid, int final_level, u32 *__restrict__ buckets,
                                                           u32 *__restrict__ okeys, u32 *__restrict__ opts,
                                                           u32 *__restrict__ std_final) {
    MG_PRIO_FOR(F);
    __shared__ __attribute__((aligned(16))) u32 lds[CoopAdd<F>::LDS_WORDS];
    merge_body<F>(TailAdd<F, true>{lds}, pkeys, ppts, cnt, G, invalid, final_level, buckets, okeys, opts, std_final);
}

// --------------------------------------------------------------------------------------------
// K8: per-tile weighted sum. For the 64 items X_0..X_63 of a tile (missing items = infinity):
//   A = sum_j X_j,  S = sum_j (j+1) X_j  -- via suffix scan (acc_j = sum_{i>=j} X_i) then sum of acc_j.
// One tile per logical wave. Cooperative for the few-tile reduces of proof-sized MSMs.
// --------------------------------------------------------------------------------------------
template <class F, class A>
MG_DEV void tile_reduce_body(const A a, const u32 *__restrict__ in, u32 seg_stride /*points*/, u32 item_off, u32 n_items,
                             u32 tiles_per_seg, u32 *__restrict__ outA, u32 *__restrict__ outS, int std_out) {
    const u32 wave = a.unit();
    const int lane = a.lane;
    const u32 seg = wave / tiles_per_seg, tile = wave % tiles_per_seg;
    const u32 idx = tile * 64 + lane;
    XYZZ<F> acc = XYZZ<F>::inf();
    if (idx < n_items) acc = XYZZ<F>::load(in + ((size_t)seg * seg_stride + item_off + idx) * XYZZ<F>::WORDS);
    int top = 1; // lanes actually populated in this tile, rounded up to a power of two
    {
        const u32 left = n_items - tile * 64;
        const int lim = left < 64 ? (int)left : 64;
        while (top < lim) top <<= 1;
    }
    for (int d = 1; d < top; d <<= 1) // suffix scan
        a.add_if(acc, XYZZ<F>::shfl(acc, lane + d > 63 ? lane : lane + d), lane + d < 64);
    constexpr int SW = XYZZ<typename F::Std>::WORDS; // arkworks-format words per point (host staging)
    const bool store = a.writer() && lane == 0;
    if (store) {
        if (std_out)
            acc.store_std(outA + (size_t)wave * SW);
        else
            acc.store(outA + (size_t)wave * XYZZ<F>::WORDS);
    }
    if (outS) {
        for (int d = top >> 1; d >= 1; d >>= 1) // tree sum of the suffix sums
            a.add_if(acc, XYZZ<F>::shfl(acc, lane + d > 63 ? lane : lane + d), lane < d);
        if (store) {
            if (std_out)
                acc.store_std(outS + (size_t)wave * SW);
            else
                acc.store(outS + (size_t)wave * XYZZ<F>::WORDS);
        }
    }
}
template <class F>
__global__ __launch_bounds__(256) MG_TAIL_ATTR void tile_reduce(const u32 *__restrict__ in, u32 seg_stride /*points*/,
                                                   u32 item_off, u32 n_items, u32 tiles_per_seg, u32 n_waves,
                                                   u32 *__restrict__ outA, u32 *__restrict__ outS, int std_out) {
    MG_PRIO_FOR(F);
    const TailAdd<F, false> a{};
    if (a.unit() >= n_waves) return; // the grid is rounded up to four wavefronts per workgroup
    tile_reduce_body<F>(a, in, seg_stride, item_off, n_items, tiles_per_seg, outA, outS, std_out);
}
template <class F>
__global__ __launch_bounds__(256) MG_TAIL_COOP_ATTR void tile_reduce_coop(const u32 *__restrict__ in, u32 seg_stride /*points*/,
                                                        u32 item_off, u32 n_items, u32 tiles_per_seg,
                                                        u32 *__restrict__ outA, u32 *__restrict__ outS, int std_out) {
    MG_PRIO_FOR(F);
    __shared__ __attribute__((aligned(16))) u32 lds[CoopAdd<F>::LDS_WORDS];
    tile_reduce_body<F>(TailAdd<F, true>{lds}, in, seg_stride, item_off, n_items, tiles_per_seg, outA, outS, std_out);
}

// --------------------------------------------------------------------------------------------
// K8 front level (work-efficient): every LANE walks S consecutive items from the top with a running sum,
//   A = sum_i X_i,   Sx = sum_i (i+1) X_i   (i = 0 .. S-1 inside the lane's stretch)
// -- 2 (S-1) additions for S items where the wavefront scan of tile_reduce spends 12 per item. With lane t covering
// items tS .. tS+S-1:  sum_k (k+1) X_k = sum_t Sx_t + S * sum_{t>=1} t A_t, i.e. a plain sum of the Sx_t plus S times the
// SAME weighted sum over the A_t (t >= 1), S times shorter: levels of this kernel shrink a window of 2^19 buckets (c = 20)
// to a few thousand items for the scan kernels below, and make wide windows affordable (2^20 BLS12-381 G1: the c = 20
// accumulate kernel is 20 % shorter than the c = 16 one, and the scan-only reduce gave all of it back).
// outS == nullptr: plain partial sums (one addition per item), used for the sums of the Sx arrays.
// Cooperative for the levels with few lanes -- from the second level on the front levels are chains of 2 (S-1) dependent
// additions and nothing else.
// --------------------------------------------------------------------------------------------
template <class F, class A>
MG_DEV void serial_reduce_body(const A a, const u32 *__restrict__ in, u32 seg_stride /*points*/, u32 item_off, u32 n_items, u32 S,
                               u32 lanes_per_seg, u32 n_lanes, u32 *__restrict__ outA, u32 *__restrict__ outS) {
    constexpr size_t XW = XYZZ<F>::WORDS;
    const u32 g = a.unit() * 64 + a.lane;
    const bool live = g < n_lanes;
    if (!A::UNIFORM && !live) return;
    const u32 seg = live ? g / lanes_per_seg : 0, l = live ? g % lanes_per_seg : 0;
    const u32 i0 = l * S;
    const u32 *base = in + ((size_t)seg * seg_stride + item_off) * XW;
    XYZZ<F> acc = XYZZ<F>::inf(), sum = XYZZ<F>::inf();
    if constexpr (A::UNIFORM) {
        for (u32 j = S; j-- > 0;) {
            const u32 i = i0 + j;
            const bool have = live && i < n_items; // false on a lane's first steps only: acc is still infinity there
            XYZZ<F> x = XYZZ<F>::inf();
            if (have) x = XYZZ<F>::load(base + (size_t)i * XW);
            a.add_if(acc, x, have);
            if (outS) a.add_if(sum, acc, have);
        }
    } else {
        const u32 i1 = i0 + S < n_items ? i0 + S : n_items;
        for (u32 i = i1; i-- > i0;) {
            acc.add(XYZZ<F>::load(base + (size_t)i * XW));
            if (outS) sum.add(acc);
        }
    }
    if (live && a.writer()) {
        acc.store(outA + (size_t)g * XW);
        if (outS) sum.store(outS + (size_t)g * XW);
    }
}
template <class F>
__global__ __launch_bounds__(256) MG_SERIAL_ATTR void serial_reduce(const u32 *__restrict__ in, u32 seg_stride /*points*/, u32 item_off,
                                                     u32 n_items, u32 S, u32 lanes_per_seg, u32 n_lanes,
                                                     u32 *__restrict__ outA, u32 *__restrict__ outS) {
    MG_PRIO_FOR(F);
    serial_reduce_body<F>(TailAdd<F, false>{}, in, seg_stride, item_off, n_items, S, lanes_per_seg, n_lanes, outA, outS);
}
template <class F>
__global__ __launch_bounds__(256) MG_TAIL_COOP_ATTR void serial_reduce_coop(const u32 *__restrict__ in, u32 seg_stride /*points*/, u32 item_off,
                                                          u32 n_items, u32 S, u32 lanes_per_seg, u32 n_lanes,
                                                          u32 *__restrict__ outA, u32 *__restrict__ outS) {
    MG_PRIO_FOR(F);
    __shared__ __attribute__((aligned(16))) u32 lds[CoopAdd<F>::LDS_WORDS];
    serial_reduce_body<F>(TailAdd<F, true>{lds}, in, seg_stride, item_off, n_items, S, lanes_per_seg, n_lanes, outA, outS);
}

// --------------------------------------------------------------------------------------------
// Second (last) reduce level for 2 <= T0 <= 64 tiles per window, ONE launch, two logical waves per window (plain: the two
// wavefronts of a 128-thread workgroup, on different SIMDs; cooperative: two workgroups): part 0 turns the tile totals A_t
// into X = sum_{t>=1} t*A_t (suffix scan + tree sum, only ceil(log2 T0) steps each), part 1 sums the S_t. The host gets
// (X, sumS): window sum = sumS + 64*X.
// Together with the level-0 tile_reduce that is 12 + 2*log2(T0) dependent additions (20 for B = 1024)
// instead of 36 over three launches -- on a latency-bound tail the depth is what matters.
// --------------------------------------------------------------------------------------------
template <class F, class A>
MG_DEV void reduce_level1_body(const A a, u32 seg, int part, const u32 *__restrict__ A0, const u32 *__restrict__ S0, u32 T0,
                               u32 *__restrict__ out_std) {
    constexpr int XW = XYZZ<F>::WORDS;
    constexpr int SW = XYZZ<typename F::Std>::WORDS;
    const int lane = a.lane;
    int top = 1;
    while (top < (int)T0) top <<= 1;
    XYZZ<F> acc = XYZZ<F>::inf();
    if (part == 0) { // X = sum_{t>=1} t*A_t  =  sum_{j>=1} (sum_{t>=j} A_t)
        if (lane >= 1 && lane < (int)T0) acc = XYZZ<F>::load(A0 + ((size_t)seg * T0 + lane) * XW);
        for (int d = 1; d < top; d <<= 1)
            a.add_if(acc, XYZZ<F>::shfl(acc, lane + d > 63 ? lane : lane + d), lane + d < 64);
        if (lane == 0) acc = XYZZ<F>::inf(); // lane 0's suffix (the total) carries weight 0
    } else {
        if (lane < (int)T0) acc = XYZZ<F>::load(S0 + ((size_t)seg * T0 + lane) * XW);
    }
    for (int d = top >> 1; d >= 1; d >>= 1)
        a.add_if(acc, XYZZ<F>::shfl(acc, lane + d > 63 ? lane : lane + d), lane < d);
    if (a.writer() && lane == 0) acc.store_std(out_std + ((size_t)seg * 2 + part) * SW);
}
template <class F>
__global__ __launch_bounds__(128) MG_TAIL_ATTR void reduce_level1(const u32 *__restrict__ A0, const u32 *__restrict__ S0, u32 T0,
                                                     u32 *__restrict__ out_std) {
    MG_PRIO_FOR(F);
    reduce_level1_body<F>(TailAdd<F, false>{}, blockIdx.x, threadIdx.x >> 6, A0, S0, T0, out_std);
}
template <class F>
__global__ __launch_bounds__(256) MG_TAIL_COOP_ATTR void reduce_level1_coop(const u32 *__restrict__ A0, const u32 *__restrict__ S0, u32 T0,
                                                          u32 *__restrict__ out_std) {
    MG_PRIO_FOR(F);
    __shared__ __attribute__((aligned(16))) u32 lds[CoopAdd<F>::LDS_WORDS];
    reduce_level1_body<F>(TailAdd<F, true>{lds}, blockIdx.x >> 1, blockIdx.x & 1, A0, S0, T0, out_std);
}

// --------------------------------------------------------------------------------------------
// K9 on the device: the fold msm_finish does on the host, for one bucket window per scalar vector (bases with precomputed
// multiples). One wavefront per vector; every lane computes the same chain (a dozen additions and doublings), lane 0 stores.
// Layouts: engine.h MsmTail, as staged for the host.
// --------------------------------------------------------------------------------------------
struct FoldDesc { // a kernel argument: field order and sizes are fixed
    const u32 *tail, *extra;
    u32 kind, T1, nP, segs, n_extra, tail_shift; // kind: MsmTailKind
    u32 extra_shift[8];
};
static_assert(sizeof(FoldDesc::extra_shift) == sizeof(MsmTail::extra_shift), "FoldDesc::extra_shift holds MsmTail::MAX_EXTRA shifts");
template <class F>
__global__ __launch_bounds__(64) void fold_windows(FoldDesc d, u32 *__restrict__ out, size_t out_stride) {
    MG_PRIO_FOR(F);
    typedef typename F::Std S;
    constexpr int SW = XYZZ<S>::WORDS;
    const u32 q = blockIdx.x;
    auto ld = [](const u32 *p) {
        const XYZZ<S> s = XYZZ<S>::load(p);
        if (s.is_inf()) return XYZZ<F>::inf();
        return XYZZ<F>{F::from_std(s.x), F::from_std(s.y), F::from_std(s.zz), F::from_std(s.zzz)};
    };
    auto pow2 = [](XYZZ<F> p, u32 k) {
        for (u32 i = 0; i < k; ++i) p = XYZZ<F>::dbl(p);
        return p;
    };
    XYZZ<F> win = XYZZ<F>::inf();
    if (d.kind == TAIL_WINDOW_SUMS) {
        win = ld(d.tail + (size_t)q * SW);
    } else if (d.kind == TAIL_X_SUMS) {
        win = pow2(ld(d.tail + ((size_t)q * 2 + 0) * SW), 6);
        win.add(ld(d.tail + ((size_t)q * 2 + 1) * SW));
    } else {
        const u32 *A1 = d.tail + (size_t)q * d.T1 * SW;
        const u32 *S1 = d.tail + ((size_t)d.segs * d.T1 + (size_t)q * d.T1) * SW;
        const u32 *P0 = d.tail + ((size_t)d.segs * 2 * d.T1 + (size_t)q * d.nP) * SW;
        XYZZ<F> sumS = XYZZ<F>::inf(), run = XYZZ<F>::inf(), uA = XYZZ<F>::inf();
        for (int u = (int)d.T1 - 1; u >= 0; --u) {
            sumS.add(ld(S1 + (size_t)u * SW));
            if (u >= 1) {
                run.add(ld(A1 + (size_t)u * SW));
                uA.add(run);
            }
        }
        XYZZ<F> X = pow2(uA, 6);
        X.add(sumS);
        win = pow2(X, 6);
        for (u32 u = 0; u < d.nP; ++u) win.add(ld(P0 + (size_t)u * SW));
    }
    if (d.tail_shift) win = pow2(win, d.tail_shift);
    for (u32 e = 0; e < d.n_extra; ++e) win.add(pow2(ld(d.extra + ((size_t)e * d.segs + q) * SW), d.extra_shift[e]));
    if (threadIdx.x == 0) win.store_std(out + (size_t)q * out_stride);
}

} // namespace mg
