// Host orchestration of the MSM pipeline: GroupEngineT (base sets, plan, launch stages, finish and fold, the digit stage alone, QAP
// column sums) -- one instantiation per (curve, group), on top of the bulk group operations of GroupOpsT (group_ops.h).
// Part of msm_impl.h.
#pragma once
#include "group_ops.h" // (first: it compiles without anything below)
#include "msm_digits.h"
#include "msm_accumulate.h"
#include "msm_reduce.h"
#include "qap_columns.h"

namespace mg {

// --------------------------------------------------------------------------------------------
// host orchestration
// --------------------------------------------------------------------------------------------

// The zero-fills of an MSM launch (pair counter, bucket array or direct result, timing words) as ONE kernel of ours instead of
// hipMemsetAsync calls: inside a stream capture those become memset nodes, and a memset node of a LINEAR captured graph was found
// to replay with a wrong fill pattern once other work had gone through the runtime (round 5: profiles/r05_linear_graph_defect.txt;
// the runtime pre-builds the AQL packets of such graphs, its own fill kernel included). No node of the library's graphs is a
// runtime-generated fill any more; one launch instead of two or three also shortens the chain.
// two word ranges device -> pinned host memory, a system-scope fence, then the token (msm_launch, MsmWorkspace::notify)
static __global__ __launch_bounds__(256) void stage_and_notify_kernel(const u32 *__restrict__ src0, u32 *__restrict__ dst0, u32 n0,
                                                                      const u32 *__restrict__ src1, u32 *__restrict__ dst1, u32 n1,
                                                                      u32 *__restrict__ flag) {
    for (u32 i = threadIdx.x; i < n0; i += 256) dst0[i] = src0[i];
    for (u32 i = threadIdx.x; i < n1; i += 256) dst1[i] = src1[i];
    __threadfence_system(); // every lane's stores are visible system-wide before it reaches the barrier ...
    __syncthreads();
    if (threadIdx.x == 0 && flag) {
        __atomic_store_n(flag, 1u, __ATOMIC_RELEASE); // ... and the token goes last
        __threadfence_system();
    }
}
struct ZeroRanges {
    u32 *p[3];
    u32 n[3]; // words
};
template <class F> __global__ __launch_bounds__(256) void zero_ranges(ZeroRanges r) {
    const u32 stride = gridDim.x * 256u, i0 = blockIdx.x * 256u + threadIdx.x;
#pragma unroll
    for (int t = 0; t < 3; ++t)
        for (u32 i = i0; i < r.n[t]; i += stride) r.p[t][i] = 0u;
}

// The A/B knobs of the MSM pipeline (tuning.h ab_knob), read once: the shipped library compiles these defaults in, the diagnosis
// twin reads the environment. (`static`: one copy per unit, as a variant build may compile a single unit with -DMG_DIAG.)
//
// Front levels of the bucket reduce (serial_reduce): 2^lgS0 items per lane while a level has >= 2^18 items, 2^lgS below
// (MANTA_RED_S0 / MANTA_RED_S; MANTA_RED_S=0: scan kernels only; unset = 3), applied while a window segment has at
// least min_items items (MANTA_RED_MIN); 2^lgSP items per lane in the plain sums of the Sx arrays (MANTA_RED_SP), which
// run on a side stream next to the weighted chain unless MANTA_RED_SIDE=0.
// History (profiles/r03_window_and_tail_study.txt): the first versions -- serial chains for the plain sums, a side stream per
// workspace -- lost 6-9 % of the pipelined rate and were off by default; c = 20 tables (accumulate kernel 19 % shorter) still do
// not pay: the 2^19-bucket reduce is eight more dependent launches and a third sort pass.
static int ab_knob_in(const char *name, int lo, int hi, int dflt) {
    const int v = ab_knob(name, dflt);
    return v < lo ? lo : (v > hi ? hi : v);
}
struct MsmKnobs {
    int msm_L = ab_knob("MANTA_MSM_L", 0);                        // entries per accumulate lane, > 0 overrides plan_for
    int acc_round_waves = ab_knob("MANTA_ACC_ROUND_WAVES", -1);   // acc_round_lanes
    int coop_tiles = ab_knob("MANTA_COOP_TILES", 64);             // coop_tiles
    u32 coop_waves = (u32)ab_knob("MANTA_COOP_WAVES", 512);       // merge and front levels of at most this many 64-entry waves: cooperative
    u32 merge_g = [](int v) { return (u32)(v >= 1 && v <= 64 ? v : 0); }(ab_knob("MANTA_MERGE_G", 0)); // merge_g1; 0 = by size
    int lgS0 = ab_knob_in("MANTA_RED_S0", 1, 8, 2), lgS = ab_knob_in("MANTA_RED_S", -1, 8, -1), lgSP = ab_knob_in("MANTA_RED_SP", 1, 8, 3);
    // stand-alone MSMs and single proofs: a window segment takes front levels from this many buckets on
    u32 min_items = (u32)ab_knob_in("MANTA_RED_MIN", 128, 1 << 30, 16384);
    // Passes of several scalar vectors (batched proofs): from this many on. Round 6, with the front levels legal inside a slot's
    // graphs: 12-bit windows for a / b_g1 / b_g2 / l (2 048 buckets per proof and MSM) and front levels from 2 048 buckets on --
    // the h MSM's 8 192 too -- against 11-bit windows and scan tiles only: +3.4 % (W) / +4.2 % (dense) proofs/s,
    // profiles/r06_batched_windows_front_levels.txt. (an explicit MANTA_RED_MIN rules both thresholds unless MANTA_RED_MIN_BATCH
    // says otherwise)
    u32 min_items_batch = (u32)ab_knob_in("MANTA_RED_MIN_BATCH", 128, 1 << 30, ab_knob("MANTA_RED_MIN", -1) >= 0 ? (int)min_items : 2048);
    bool side = ab_knob_in("MANTA_RED_SIDE", 0, 1, 1) != 0;
    bool sort_low = ab_knob("MANTA_SORT_LOW", 1) != 0; // sort a batched pass by the bucket bits only
    // MANTA_ACC_SINGLE: bit 0 = G1, bit 1 = G2. Default G1 only (sequential PrivateTransfer proofs, sparse / W / dense, two
    // alternations on one box: off 0.770 / 0.859 / 1.258 ms, G1 0.755 / 0.852 / 1.270, G2 0.749 / 0.853 / 1.286, both 0.739 /
    // 0.863 / 1.314 -- over Fp2 the cooperative additions are ~20 us each and the dense G2 chain gets longer)
    int acc_single = ab_knob("MANTA_ACC_SINGLE", 1);
    // workgroup of the compacting digit kernel, 256 / 512 / 1024 -- measured: 256 beats 512 and 1024 on the same box
    u32 digits_threads = [](int v) { return (u32)(v == 256 || v == 512 || v == 1024 ? v : 256); }(ab_knob("MANTA_DIGITS_THREADS", 0));
    bool z3_sort = ab_knob("MANTA_Z3_SORT", 0) != 0;
    // the fused front end wherever msm_dense_front_applies and the launch is stand-alone; 0: the compacting digit kernel and the
    // whole sort for those launches too (profiles/dense_front_ab.txt)
    bool dense_front = ab_knob_in("MANTA_DENSE_FRONT", 0, 1, 1) != 0;
};
static const MsmKnobs &msm_knobs() {
    static const MsmKnobs k; // (first use: the first MSM of the process)
    return k;
}

template <class Curve, int CURVE_ID, int GROUP> class GroupEngineT : public GroupOpsT<Curve, CURVE_ID, GROUP> {
  public:
    typedef GroupOpsT<Curve, CURVE_ID, GROUP> Ops; // its types, formats and host-point cast, by name
    using typename Ops::F;
    using typename Ops::FIO;
    using typename Ops::HP;
    using typename Ops::FrC;
    using Ops::AW;
    using Ops::XW;
    using Ops::AW_IO;
    using Ops::XW_IO;
    using Ops::hp;
    static constexpr bool SAME = std::is_same<F, FIO>::value;
    // stride of one point in a BaseSet: the internal affine record padded to a multiple of 32 B (BLS12-381
    // G1: 28 -> 32 words = one 128 B line per gathered point instead of a record straddling two)
    static constexpr int AWS = SAME ? AW : (AW + 7) / 8 * 8;

    int base_record_bytes() const override { return AWS * 4; }

    // ---------------------------------------------------------------- bases
    int bases_create(const u32 *pts_in, size_t n_in, bool src_on_device, int pre_c, BaseSet **out,
                     bool drop_infinity = false, u32 n_sets = 1) override {
        if (!pts_in || !n_in || !out || n_sets == 0 || n_in % n_sets) return MG_ERR_ARG;
        const u32 *pts = pts_in;
        size_t n = n_in;
        std::vector<u32> compact, map;
        if (drop_infinity && !src_on_device && compact_infinity(pts_in, n_in, compact, map)) {
            pts = compact.data();
            n = map.size();
        }
        prime_occupancy();
        BaseSet *bs = new BaseSet();
        struct Guard { // at every return: the window tables of full tables go, and on failure the half-built set
            GroupEngineT *eng;
            BaseSet *bs;
            u32 *win_pts;
            ~Guard() {
                if (win_pts) hipFree(win_pts);
                if (bs) eng->bases_destroy(bs);
            }
        } guard{this, bs, nullptr};
        bs->curve = CURVE_ID;
        bs->group = GROUP;
        bs->device = current_device();
        bs->n = n;
        bs->n_orig = n_in;
        bs->n_sets = n_sets;
        bs->set_len = n_in / n_sets;
        set_query_ranges(bs, map.data(), map.size());
        if (!map.empty()) {
            if (hipMalloc((void **)&bs->d_map, map.size() * 4) != hipSuccess ||
                memcpy_sync(bs->d_map, map.data(), map.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
                return MG_ERR_OOM;
        }
        // pre_c < 0: FULL tables of window width -pre_c -- besides 2^(c w) P every multiple m 2^(c w) P, m = 1 .. 2^(c-1), so that
        // a signed digit addresses its summand directly and the MSM is one plain sum: no buckets, no sort, no bucket reduce
        const bool full = pre_c < 0;
        if (full) pre_c = -pre_c;
        int W = 1;
        if (pre_c > 0) {
            W = windows_of(pre_c);
            bs->pre_c = pre_c;
            bs->pre_W = W;
            bs->full = full;
        }
        const u32 FB = full ? 1u << (pre_c - 1) : 1u; // table entries per (window, base)
        if (full && (pre_c < 2 || pre_c > 12 || (size_t)W * n * FB >= ((size_t)1 << 31))) return MG_ERR_ARG;
        bs->inf_record = pre_c > 0 && !full;
        if (bs->inf_record && (size_t)W * n + 1 >= ((size_t)1 << 31)) return MG_ERR_ARG; // (key_layout refuses the launch too)
        bs->bytes = ((size_t)W * n * FB + (bs->inf_record ? 1u : 0u)) * AWS * 4;
        hipError_t e = hipMalloc((void **)&bs->d_pts, bs->bytes);
        if (e == hipSuccess && bs->inf_record) {
            const std::vector<u32> zero(AWS, 0u);
            e = memcpy_sync(bs->d_pts + (size_t)W * n * AWS, zero.data(), (size_t)AWS * 4, hipMemcpyHostToDevice);
        }
        u32 *&win_pts = guard.win_pts; // full: the window tables are an intermediate
        if (e == hipSuccess && full) e = hipMalloc((void **)&win_pts, (size_t)W * n * AWS * 4);
        if (e != hipSuccess) return hip_failure(e, "hipMalloc(bases)", MG_ERR_OOM);
        u32 *const dst = full ? win_pts : bs->d_pts;
        int rc;
        if ((rc = upload_bases(pts, n, src_on_device, dst)) || (W > 1 && (rc = precompute_windows(dst, n, pre_c, W))) ||
            (full && (rc = expand_full_tables(win_pts, bs->d_pts, n, W, FB))))
            return rc;
        guard.bs = nullptr;
        *out = bs;
        return MG_OK;
    }
    // where every query of a concatenated set starts among the n stored points (map: ascending, or none)
    static void set_query_ranges(BaseSet *bs, const u32 *map, size_t map_len) {
        const size_t n = bs->n;
        const u32 n_sets = bs->n_sets;
        if (n_sets <= 1 || n_sets > BaseSet::MAX_SETS) return;
        for (u32 q = 0; q <= n_sets; ++q) {
            const size_t first = (size_t)q * bs->set_len; // original index
            bs->set_first[q] = !map_len ? (u32)(first < n ? first : n) : (u32)(std::lower_bound(map, map + map_len, (u32)first) - map);
        }
        bs->set_first[n_sets] = (u32)n;
    }
    static int windows_of(int c) { return (FrC::BITS + c - 1) / c; } // digits_kernel: |k| < 2^(BITS - 1)
    static int hip_failure(hipError_t e, const char *what, int rc) { set_last_hip_error(e, what, __FILE__, __LINE__); return rc; }
    // drop_infinity: the points other than infinity go to `compact`, map[i] = the original index of stored point i; one infinity
    // entry is kept if nothing else is left, so that the set is never empty. false: there is nothing to drop.
    static bool compact_infinity(const u32 *pts, size_t n, std::vector<u32> &compact, std::vector<u32> &map) {
        auto finite = [&](size_t i) { return std::any_of(pts + i * AW_IO, pts + (i + 1) * AW_IO, [](u32 x) { return x != 0; }); };
        size_t kept = 0;
        for (size_t i = 0; i < n; ++i) kept += finite(i);
        if (kept == n) return false;
        compact.reserve(kept * AW_IO), map.reserve(kept);
        for (size_t i = 0; i < n; ++i)
            if (finite(i)) compact.insert(compact.end(), pts + i * AW_IO, pts + (i + 1) * AW_IO), map.push_back((u32)i);
        if (!kept) compact.assign(AW_IO, 0u), map.assign(1, 0u);
        return true;
    }
    // arkworks-format points -> internal records of AWS words at dst (table 0)
    int upload_bases(const u32 *pts, size_t n, bool src_on_device, u32 *dst) {
        hipError_t e = hipSuccess;
        if (SAME) {
            e = memcpy_sync(dst, pts, n * AW * 4, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        } else { // convert arkworks limbs -> internal representation on the device
            u32 *stage = nullptr;
            const u32 *src = pts;
            if (!src_on_device) {
                e = hipMalloc((void **)&stage, n * AW_IO * 4);
                if (e == hipSuccess) e = memcpy_sync(stage, pts, n * AW_IO * 4, hipMemcpyHostToDevice);
                src = stage;
            }
            if (e == hipSuccess) {
                hipLaunchKernelGGL((bases_to_internal<F>), dim3(cdiv(n, 256)), dim3(256), 0, setup_stream(), src, n, dst, (u32)AWS);
                e = setup_sync();
            }
            if (stage) hipFree(stage);
        }
        return e == hipSuccess ? MG_OK : hip_failure(e, "upload/convert bases", MG_ERR_HIP);
    }
    // tables 1 .. W-1 behind table 0: table w = 2^(c w) * P
    int precompute_windows(u32 *dst, size_t n, int pre_c, int W) {
        u32 *tmp = nullptr;
        const size_t cnt = (size_t)(W - 1) * n;
        hipError_t e = hipMalloc((void **)&tmp, cnt * XW * 4);
        if (e != hipSuccess) return hip_failure(e, "hipMalloc(precompute tmp)", MG_ERR_OOM);
        hipLaunchKernelGGL((precompute_chain<F>), dim3(cdiv(n, 256)), dim3(256), 0, setup_stream(), dst, (u32)AWS, (u32)n,
                           pre_c, W, tmp);
        xyzz_to_affine_launch<F>(setup_stream(), tmp, cnt, dst + n * AWS, AWS);
        e = setup_sync();
        hipFree(tmp);
        return e == hipSuccess ? MG_OK : hip_failure(e, "precompute kernels", MG_ERR_HIP);
    }
    // full tables: expand the window tables, a slice of (window, base) pairs at a time (<= 512 MB of XYZZ points in flight)
    int expand_full_tables(const u32 *win_pts, u32 *final_pts, size_t n, int W, u32 FB) {
        const size_t pairs = (size_t)W * n;
        size_t slice = ((size_t)512 << 20) / ((size_t)FB * XW * 4);
        if (slice < 256) slice = 256;
        if (slice > pairs) slice = pairs;
        u32 *tmp = nullptr;
        hipError_t e = hipMalloc((void **)&tmp, slice * FB * XW * 4);
        constexpr int KBF = 64; // one Fermat inversion per 64 points
        for (size_t j0 = 0; e == hipSuccess && j0 < pairs; j0 += slice) {
            const size_t cntp = pairs - j0 < slice ? pairs - j0 : slice;
            hipLaunchKernelGGL((full_table_chain<F>), dim3(cdiv(cntp, 256)), dim3(256), 0, setup_stream(), win_pts, (u32)AWS, j0, (u32)cntp, FB,
                               tmp);
            xyzz_to_affine_launch<F, KBF>(setup_stream(), tmp, cntp * FB, final_pts + j0 * FB * AWS, AWS);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = setup_sync();
        else (void)setup_sync();
        if (tmp) hipFree(tmp);
        return e == hipSuccess ? MG_OK : hip_status(e, "full-table kernels");
    }
    void bases_destroy(BaseSet *bs) override {
        if (!bs) return;
        if (bs->d_map) hipFree(bs->d_map);
        if (bs->d_pts) hipFree(bs->d_pts);
        delete bs;
    }

    // ---------------------------------------------------------------- plan
    MsmPlan plan_for(const BaseSet *bs, size_t n, int c_override, u32 batch = 1) const override {
        MsmPlan p;
        if (bs->pre_c > 0) {
            p.c = bs->pre_c;
            p.W = bs->pre_W;
            p.precomp = true;
            p.full = bs->full;
            p.Wb = 1;
        } else {
            int lg = 0;
            while (((size_t)1 << lg) < n) ++lg;
            // (2^20 plain bases, one MSM at a time: c = 14 / 15 / 16 / 17 -> 4.98 / 4.77 / 4.48 / 5.02 ms with the front levels of the
            // bucket reduce, which 16 windows of 32 768 buckets need: profiles/r03_plain_bases_sweep.txt)
            int c = c_override > 0 ? c_override : (lg <= 8 ? 5 : lg <= 12 ? 8 : lg <= 15 ? 10 : lg <= 18 ? 12 : lg <= 19 ? 14 : 16);
            p.c = c;
            p.W = windows_of(c);
            p.Wb = p.W;
        }
        p.B = 1u << (p.c - 1);
        // entries per lane. Large MSMs: the grid is a whole number of rounds of 2 wavefronts per SIMD (256 CUs x 4 SIMDs x 2 x 64 =
        // 131 072 lanes) -- the accumulate kernel holds two waves per SIMD, so 1.5 rounds leave half the SIMDs idle for a third of
        // the kernel; longer chunks mean fewer partials for the merge levels, hence as few rounds as keep L <= 192. Proof-sized
        // MSMs are latency chains (L mixed additions, then the merge levels): shorter chunks, twice the lanes, never fewer than 6
        // entries each. Batched proofs: most digit entries are invalid (sorted last), so the lanes are kept plentiful (L <= 96).
        // (sweeps: profiles/history/code_comment_measurements.md "chunk length")
        const size_t M = n * (size_t)p.W * batch;
        size_t L;
        if (M < ((size_t)8 << 20)) {
            L = M / (192 * 1024);
            if (L < 6) L = 6;
            // (full tables: no sort and no bucket reduce behind the merge levels any more, and the balance moves to short chunks for
            // all five MSMs of a proof -- PrivateTransfer, sequential proof, 300 proofs per run, same box: L = 1 / 2 / 3 / 4 / 5 / 6 ->
            // 0.98-1.02 / 0.93-0.98 / 0.87-0.89 / 0.89-0.93 / 0.90-0.93 / 0.91-0.92 ms)
            if (p.full) L = 3;
        } else {
            const size_t round = 128 * 1024, lmax = batch > 1 ? 96 : 192;
            const size_t rounds = (M + round * lmax - 1) / (round * lmax);
            L = (M + round * rounds - 1) / (round * rounds);
        }
        if (msm_knobs().msm_L > 0) L = (size_t)msm_knobs().msm_L;
        p.L = (u32)L;
        return p;
    }

    // lanes of one full round of the accumulate kernel: what the device holds at the kernel's own occupancy (single MSMs: the
    // shortest chain) or at two wavefronts per SIMD (batched passes: that saturates the integer pipe, and fewer lanes mean fewer
    // partials to merge). MANTA_ACC_ROUND_WAVES = wavefronts per SIMD, 0 = off (host-side chunk length only).
    u32 acc_round_lanes(bool batched, bool single = false) {
        const int knob = msm_knobs().acc_round_waves;
        if (knob == 0) return 0;
        const int dev = current_device();
        if (dev < 0 || dev >= 64 || !occ_[dev].cus.load(std::memory_order_acquire)) return 0; // (primed by bases_create)
        u32 w = single && occ_[dev].blocks_single ? occ_[dev].blocks_single : occ_[dev].blocks; // 256-thread blocks per CU = wavefronts per SIMD
        if (knob > 0) w = (u32)knob < w ? (u32)knob : w;
        else if (batched && w > 2) w = 2;
        return w * 256u * occ_[dev].cus.load(std::memory_order_relaxed);
    }
    struct Occ {
        u32 blocks = 0, blocks_single = 0; // accumulate_chunks / accumulate_single (more registers, LDS: its own round size)
        std::atomic<u32> cus{0};
    } occ_[64];
    // (asked once per device outside any stream capture: bases_create runs before the first MSM on its device)
    void prime_occupancy() {
        const int dev = current_device();
        if (dev < 0 || dev >= 64 || occ_[dev].cus.load(std::memory_order_acquire)) return;
        int nb = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, accumulate_chunks<F, false>, 256, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || nb < 1 || cus < 1) {
            (void)hipGetLastError();
            return;
        }
        int nbs = 0;
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&accumulate_single<F>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)AccSingle<F>::LDS_BYTES) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbs, accumulate_single<F>, 256, AccSingle<F>::LDS_BYTES) != hipSuccess || nbs < 1) {
            (void)hipGetLastError();
            nbs = 0;
        }
        std::lock_guard<std::mutex> g(side_mu_);
        occ_[dev].blocks_single = (u32)nbs;
        occ_[dev].blocks = (u32)nb;
        occ_[dev].cus.store((u32)cus, std::memory_order_release);
    }

    // few tiles = a pure latency chain: spread each addition over the workgroup's four wavefronts
    static bool coop_tiles(u32 tiles) { return (int)tiles <= msm_knobs().coop_tiles; }
    // entries folded serially per lane in the first merge level. Large MSMs: 4 (throughput). Proof-sized MSMs: 16 --
    // the level then has few enough logical waves (<= MsmKnobs::coop_waves) for the cooperative kernel, whose additions
    // cost a third: 15 cooperative serial steps + the scan beat 3 plain steps + the scan and shrink the next level.
    static u32 merge_g1(size_t M) {
        if (const u32 g = msm_knobs().merge_g) return g;
        return M < ((size_t)8 << 20) ? 16u : 4u;
    }

    // One launch site per pair of a plain and a cooperative kernel (the cooperative one: a workgroup per wave or tile); the argument
    // after the stream counts the items: tiles (segments x tiles per segment), lanes (segments x lanes per segment), 64-entry
    // waves, segments. tile_reduce is cooperative where the tiles are few and the site allows it.
    static void tile_reduce_launch(hipStream_t st, u32 items, bool may_coop, const u32 *in, u32 stride, u32 off, u32 n, u32 tiles,
                                   u32 *A, u32 *S, int std_out) {
        if (may_coop && coop_tiles(items))
            hipLaunchKernelGGL((tile_reduce_coop<F>), dim3(items), dim3(256), 0, st, in, stride, off, n, tiles, A, S, std_out);
        else
            hipLaunchKernelGGL((tile_reduce<F>), dim3(cdiv(items, 4)), dim3(256), 0, st, in, stride, off, n, tiles, items, A, S, std_out);
    }
    static void serial_reduce_launch(hipStream_t st, size_t lanes_all, const u32 *in, u32 stride, u32 off, u32 n, u32 S, u32 lanes,
                                     u32 *A, u32 *Sx) {
        if (cdiv(lanes_all, 64) <= msm_knobs().coop_waves)
            hipLaunchKernelGGL((serial_reduce_coop<F>), dim3(cdiv(lanes_all, 64)), dim3(256), 0, st, in, stride, off, n, S, lanes,
                               (u32)lanes_all, A, Sx);
        else
            hipLaunchKernelGGL((serial_reduce<F>), dim3(cdiv(lanes_all, 256)), dim3(256), 0, st, in, stride, off, n, S, lanes,
                               (u32)lanes_all, A, Sx);
    }
    static void merge_partials_launch(hipStream_t st, u32 waves, u32 *pkeys, u32 *ppts, u32 cnt, u32 G, u32 invalid, int fin,
                                      u32 *buckets, u32 *okeys, u32 *opts, u32 *std_final) {
        if (waves <= msm_knobs().coop_waves)
            hipLaunchKernelGGL((merge_partials_coop<F>), dim3(waves), dim3(256), 0, st, pkeys, ppts, cnt, G, invalid, fin, buckets,
                               okeys, opts, std_final);
        else
            hipLaunchKernelGGL((merge_partials<F>), dim3(cdiv(waves, 4)), dim3(256), 0, st, pkeys, ppts, cnt, G, invalid, fin, buckets,
                               okeys, opts, waves, std_final);
    }
    static void reduce_level1_launch(hipStream_t st, u32 segs, const u32 *A0, const u32 *S0, u32 T0, u32 *out) {
        if (coop_tiles(segs * 2))
            hipLaunchKernelGGL((reduce_level1_coop<F>), dim3(segs * 2), dim3(256), 0, st, A0, S0, T0, out);
        else
            hipLaunchKernelGGL((reduce_level1<F>), dim3(segs), dim3(128), 0, st, A0, S0, T0, out);
    }

    hipStream_t engine_side_stream() {
        std::lock_guard<std::mutex> g(side_mu_);
        if (!side_stream_) {
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
                hipStreamCreateWithPriority(&side_stream_, hipStreamNonBlocking, hi) != hipSuccess)
                side_stream_ = nullptr;
        }
        return side_stream_;
    }
    std::mutex side_mu_;
    hipStream_t side_stream_ = nullptr; // process lifetime

    // ---------------------------------------------------------------- launch
    int msm_launch(const BaseSet *bs, const u32 *d_scalars, size_t n, int scalar_mode, int c_override,
                   MsmWorkspace *ws, u32 batch = 1, size_t scalar_stride_words = 0, bool sparse = false) override {
        if (!bs || !d_scalars || !ws || n == 0 || n > bs->n_orig || batch == 0 || batch > 65535) return MG_ERR_ARG;
        if (bs->curve != CURVE_ID || bs->group != GROUP) return MG_ERR_ARG;
        const u32 nsets = bs->n_sets; // concatenated queries over one scalar vector: nsets results per vector
        if (nsets > 1 && n > bs->set_len) return MG_ERR_ARG;
        const size_t n_scalars = n;                          // scalars supplied by the caller (indexed by original position)
        if (bs->d_map || n > bs->n || nsets > 1) n = bs->n; // entries = stored points; the kernel zips to the shorter side
        // batch > 1: several scalar vectors against the same bases (a pass of several proofs)
        Launch r{bs, d_scalars, ws, msm_stream_of(ws), nullptr, n, n_scalars, scalar_stride_words, scalar_mode, batch, nsets, batch > 1,
                 sparse, plan_for(bs, n, c_override, batch)};
        int rc;
        if ((rc = launch_reserve(r))) return rc;
        launch_digits(r);
        if ((rc = launch_sort(r)) || (rc = launch_accumulate(r))) return rc;
        launch_merge(r);
        if ((rc = launch_front_levels(r)) || (rc = launch_scan_tail(r)) || (rc = launch_stage(r))) return rc;
        if (!ws->capturing) MG_HIP(hipEventRecord(ws->done, r.s));
        MG_HIP(hipGetLastError());
        ws->plan = r.pl, ws->tail = r.tail, ws->batch = r.batch; // what msm_finish / msm_fold_device read
        ws->pending = 1;
        return MG_OK;
    }

    static int stage_reserve(MsmWorkspace *ws, size_t bytes) {
        if (ws->h_stage_cap >= bytes) return MG_OK;
        if (ws->h_stage) hipHostFree(ws->h_stage);
        ws->h_stage = nullptr;
        ws->h_stage_cap = 0;
        size_t cap = bytes < 65536 ? 65536 : bytes;
        MG_HIP(hipHostMalloc(&ws->h_stage, cap, hipHostMallocDefault));
        ws->h_stage_cap = cap;
        return MG_OK;
    }

    // ---------------------------------------------------------------- finish (host fold)
    int msm_finish(MsmWorkspace *ws, HostPoint *out, bool already_synced = false) override {
        if (!ws || !ws->pending) return MG_ERR_STATE;
        if (!already_synced) MG_HIP(hipEventSynchronize(ws->done));
        ws->pending = 0;
        if (ws->timed && !already_synced) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ws->t0, ws->t1) == hipSuccess) last_times().accumulate_ms = ms;
            const unsigned long long ck[2] = {((volatile unsigned long long *)ws->h_clk)[0], ((volatile unsigned long long *)ws->h_clk)[1]};
            int khz = 0, dev = 0;
            if (ck[1] && hipGetDevice(&dev) == hipSuccess &&
                hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess)
                last_times().accumulate_mhz = (float)((double)ck[0] / (double)ck[1] * (double)khz / 1e3);
        }
        const MsmPlan &pl = ws->plan;
        const MsmTail &t = ws->tail;
        const u32 Wb = (u32)pl.Wb, segs = t.segs, T1 = t.T1, nP = t.nP;
        const u32 *st = (const u32 *)ws->h_stage;
        for (u32 q = 0; q < ws->batch; ++q) {
            HP total = HP::inf();
            for (int w = (int)((q + 1) * Wb) - 1; w >= (int)(q * Wb); --w) {
                HP win;
                if (t.kind == TAIL_WINDOW_SUMS) { // the staged point is the window sum
                    win = HP::from_xyzz_words(st + (size_t)w * XW_IO);
                } else if (t.kind == TAIL_X_SUMS) { // fused reduce: (X, sumS) per window, window = sumS + 64 X
                    const HP X = HP::from_xyzz_words(st + ((size_t)w * 2 + 0) * XW_IO);
                    const HP sumS = HP::from_xyzz_words(st + ((size_t)w * 2 + 1) * XW_IO);
                    win = HP::add(sumS, HP::mul_pow2(X, 6));
                } else { // TAIL_TWO_LEVELS
                    const u32 *A1 = st + ((size_t)w * T1) * XW_IO;
                    const u32 *S1 = st + ((size_t)segs * T1 + (size_t)w * T1) * XW_IO;
                    const u32 *P0 = st + ((size_t)segs * 2 * T1 + (size_t)w * nP) * XW_IO;
                    // X = sum_{t>=1} t*A0[t] = sum_u ( S1[u] + 64*u*A1[u] )
                    HP sumS = HP::inf(), run = HP::inf(), uA = HP::inf();
                    for (int u = (int)T1 - 1; u >= 0; --u) {
                        sumS = HP::add(sumS, HP::from_xyzz_words(S1 + (size_t)u * XW_IO));
                        if (u >= 1) {
                            run = HP::add(run, HP::from_xyzz_words(A1 + (size_t)u * XW_IO));
                            uA = HP::add(uA, run); // sum_u u*A1[u]
                        }
                    }
                    HP X = HP::add(sumS, HP::mul_pow2(uA, 6));
                    HP sumP = HP::inf();
                    for (u32 u = 0; u < nP; ++u) sumP = HP::add(sumP, HP::from_xyzz_words(P0 + (size_t)u * XW_IO));
                    win = HP::add(sumP, HP::mul_pow2(X, 6));
                }
                if (t.tail_shift) win = HP::mul_pow2(win, t.tail_shift); // front levels: window = 2^shift * tail + extras
                for (u32 e = 0; e < t.n_extra; ++e) {
                    const HP x = HP::from_xyzz_words(st + (t.extra_off_pts + (size_t)e * segs + (size_t)w) * XW_IO);
                    win = HP::add(win, t.extra_shift[e] ? HP::mul_pow2(x, t.extra_shift[e]) : x);
                }
                if (w != (int)((q + 1) * Wb) - 1) total = HP::mul_pow2(total, (unsigned)pl.c);
                total = HP::add(total, win);
            }
            hp(out + q) = total;
        }
        return MG_OK;
    }

    // ---------------------------------------------------------------- finish on the device
    int msm_fold_device(MsmWorkspace *ws, u32 *d_out, size_t out_stride_words, hipStream_t on = nullptr) override {
        if (!ws || !ws->pending || !d_out || !ws->tail.d_tail) return MG_ERR_STATE;
        const MsmTail &t = ws->tail;
        if (ws->plan.Wb != 1) return MG_ERR_STATE; // plain bases keep the host fold (up to 255 Horner doublings: a host job)
        FoldDesc d{t.d_tail, ws->extra.as<u32>(), t.kind, t.T1, t.nP, t.segs, t.n_extra, t.tail_shift, {}};
        for (u32 e = 0; e < t.n_extra; ++e) d.extra_shift[e] = t.extra_shift[e];
        hipLaunchKernelGGL((fold_windows<F>), dim3(ws->batch), dim3(64), 0, on ? on : msm_stream_of(ws), d, d_out, out_stride_words);
        MG_HIP(hipGetLastError());
        return MG_OK;
    }

    // ---------------------------------------------------------------- the digit stage alone (parity-test surface)
    // What msm_launch does up to and including the digit kernel, for a base set that exists as a description only (the kernel
    // reads no point): the plan of plan_for, the key layout and refusals of launch_reserve, the launch of launch_digits. The pair
    // arrays start as the caller's, so what the kernel leaves alone comes back untouched. Which layout runs is the caller's choice
    // here (c.compact), where launch_reserve decides it.
    int msm_digits(const MsmDigitsCall &c) override {
        if (!c.scalars || !c.keys || !c.vals || !c.layout || (c.compact && !c.count) || c.n == 0 || c.n_scalars == 0 || c.batch == 0 ||
            c.batch > 65535 || (c.scalar_mode != SCALARS_CANONICAL && c.scalar_mode != SCALARS_MONT) || c.table_mode < 0 ||
            c.table_mode > 2 || c.c < 1 || c.c > 24 || (c.table_mode == 2 && (c.c < 2 || c.c > 12)) || c.n_sets == 0 || c.set_len == 0)
            return MG_ERR_ARG;
        BaseSet bs; // as bases_create leaves it, without the points
        bs.curve = CURVE_ID, bs.group = GROUP, bs.device = current_device();
        bs.n = c.n, bs.n_orig = (size_t)c.n_sets * c.set_len, bs.n_sets = c.n_sets, bs.set_len = c.set_len;
        if (c.table_mode) bs.pre_c = c.c, bs.pre_W = windows_of(c.c), bs.full = c.table_mode == 2;
        // the index ranges: stored bases beyond the logical length, scalars beyond a query (msm_launch), a map entry beyond the set
        if (bs.n > bs.n_orig || (!c.map && bs.n != bs.n_orig) || c.n_scalars > bs.n_orig || (c.n_sets > 1 && c.n_scalars > c.set_len))
            return MG_ERR_ARG;
        for (size_t i = 0; c.map && i < c.n; ++i)
            if (c.map[i] >= bs.n_orig) return MG_ERR_ARG;
        // (a map in any order is legal for the kernel; the per-query launches need the ascending one bases_create builds)
        if (!c.map || std::is_sorted(c.map, c.map + c.n)) set_query_ranges(&bs, c.map, c.map ? c.n : 0);
        Launch r{&bs, nullptr, nullptr, nullptr, nullptr, c.n, c.n_scalars, (size_t)c.n_scalars * 8, c.scalar_mode, c.batch, c.n_sets, c.batch > 1,
                 c.compact, plan_for(&bs, c.n, c.c, c.batch)};
        if (const int rc = key_layout(r)) return rc;
        c.layout[0] = (u32)r.pl.W, c.layout[1] = r.pl.B, c.layout[2] = r.seg_keys, c.layout[3] = r.invalid;
        const size_t sb = (size_t)c.batch * c.n_scalars * 32, pb = r.M * 4;
        DevCall m; // scalars | map | keys | vals | pair count
        if (const int rc = m.begin({sb, c.map ? (size_t)c.n * 4 : 0, pb, pb, c.compact ? 4u : 0u}, "mg_msm_digits")) return rc;
        r.s = m.stream(), r.d_scalars = m.dev<u32>(0), bs.d_map = m.dev<u32>(1), r.d_count = m.dev<u32>(4);
        m.up(0, c.scalars, sb);
        m.up(1, c.map, (size_t)c.n * 4);
        m.up(2, c.keys, pb);
        m.up(3, c.vals, pb);
        m.zero(4);
        m.run([&] { enqueue_digits(r, m.dev<u32>(2), m.dev<u32>(3)); });
        m.down(c.keys, 2, pb);
        m.down(c.vals, 3, pb);
        m.down(c.count, 4, 4);
        return m.finish();
    }

    // The fused front end alone, likewise for a base set that exists as a description only: what launch_reserve and launch_sort do
    // for a dense launch, up to the sorted pairs (n W of them; a zero digit is the pair (0, layout[3] = the infinity index)). The
    // output arrays start as the caller's. MG_ERR_ARG for a shape msm_dense_front_applies turns down.
    int msm_dense_front(const MsmDigitsCall &c) override {
        if (!c.scalars || !c.keys || !c.vals || !c.layout || c.n == 0 || c.n_scalars == 0 || c.c < 1 || c.c > 24 || c.set_len == 0 ||
            (c.scalar_mode != SCALARS_CANONICAL && c.scalar_mode != SCALARS_MONT) ||
            !msm_dense_front_applies(c.batch, c.n_sets, windows_of(c.c), c.table_mode, c.compact))
            return MG_ERR_ARG;
        BaseSet bs;
        bs.curve = CURVE_ID, bs.group = GROUP, bs.device = current_device();
        bs.n = c.n, bs.n_orig = c.set_len, bs.set_len = c.set_len;
        bs.pre_c = c.c, bs.pre_W = windows_of(c.c), bs.inf_record = true;
        if (bs.n > bs.n_orig || (!c.map && bs.n != bs.n_orig) || c.n_scalars > bs.n_orig) return MG_ERR_ARG;
        for (size_t i = 0; c.map && i < c.n; ++i)
            if (c.map[i] >= bs.n_orig) return MG_ERR_ARG;
        Launch r{&bs, nullptr, nullptr, nullptr, nullptr, c.n, c.n_scalars, 0, c.scalar_mode, 1, 1, false, false, plan_for(&bs, c.n, c.c, 1)};
        if (const int rc = key_layout(r)) return rc;
        r.end_bit = 1;
        while (r.nb > 1 && (1u << r.end_bit) <= r.nb - 1) ++r.end_bit; // (launch_reserve: the bits of the last bucket key)
        c.layout[0] = (u32)r.pl.W, c.layout[1] = r.pl.B, c.layout[2] = r.seg_keys, c.layout[3] = (u32)((size_t)r.pl.W * c.n);
        const size_t sb = (size_t)c.n_scalars * 32, pb = r.M * 4;
        DevCall m; // scalars | map | sorted keys | sorted vals | the sort's scratch
        if (const int rc = m.begin({sb, c.map ? (size_t)c.n * 4 : 0, pb, pb, sort_pairs_temp_bytes(r.M, cdiv(c.n, 256))}, "mg_msm_dense_front"))
            return rc;
        r.s = m.stream(), r.d_scalars = m.dev<u32>(0), bs.d_map = m.dev<u32>(1);
        m.up(0, c.scalars, sb);
        m.up(1, c.map, (size_t)c.n * 4);
        m.up(2, c.keys, pb);
        m.up(3, c.vals, pb);
        m.run([&] { return enqueue_dense_front(r, m.dev(4), m.dev<u32>(2), m.dev<u32>(3)); });
        m.down(c.keys, 2, pb);
        m.down(c.vals, 3, pb);
        return m.finish();
    }

    // ---------------------------------------------------------------- QAP column sums (qap_columns.h)
    void scalar_one_mont(u64 out[4]) const override {
        const host::HFp<FrC> one = host::HFp<FrC>::one();
        std::memcpy(out, one.v, 32);
    }
    u64 qap_max_columns() const override { return ((u64)1 << 32) / XWM - 2; } // (columns + 1) XW words stay below 2^32
    // sorted entries per lane of the segmented sum when the caller leaves it open: two wavefronts per SIMD of lanes (256 CUs) before
    // the chunks grow, never fewer than 4 entries (below that the partials outnumber the entries) nor more than 64 (a chain of 64
    // dependent general additions is already the longest stage of the call)
    static u32 qap_entries_per_lane(size_t N) {
        const size_t l = N / (128 * 1024);
        return (u32)(l < 4 ? 4 : l > 64 ? 64 : l);
    }
    int qap_columns(const u32 *d_bases, size_t n_bases, const QapEntries &en, u64 n_cols, u32 entries_per_lane,
                    u32 *out_affine_host) override {
        const size_t N = en.n;
        // what the 32-bit pairs and word counts cannot hold: 2^31 entries (the sort), 2^32 words of column sums (the zero-fill)
        if (!out_affine_host || n_cols == 0 || n_cols > qap_max_columns() || N >= ((size_t)1 << 31) ||
            (N && (!d_bases || !n_bases || !en.col || !en.src || !en.val)))
            return MG_ERR_ARG;
        for (size_t e = 0; e < N; ++e)
            if (en.col[e] >= n_cols || en.src[e] >= n_bases) return MG_ERR_ARG;
        const size_t out_bytes = (size_t)n_cols * AW_IO * 4;
        if (N == 0) {
            std::memset(out_affine_host, 0, out_bytes);
            return MG_OK;
        }
        const u32 L = entries_per_lane ? entries_per_lane : qap_entries_per_lane(N);
        const u32 T = cdiv(N, L), waves1 = cdiv((size_t)2 * T, 64), invalid = (u32)n_cols;
        int end_bit = 1;
        while (end_bit < 32 && ((u64)1 << end_bit) < n_cols) ++end_bit; // keys are below n_cols
        std::vector<u32> ids(N);
        for (size_t e = 0; e < N; ++e) ids[e] = (u32)e;
        const size_t sort_bytes = sort_pairs_temp_bytes(N);
        enum { SRC, VAL, KEYS, IDS, SKEYS, SIDS, SORT, PROD, PK0, PP0, PK1, PP1, SUMS, STD, AFF };
        std::vector<u32> stage((size_t)n_cols * AW_IO); // (out_affine_host is written only if the call succeeds)
        DevCall m;
        if (const int rc = m.begin({N * 4, N * 32, N * 4, N * 4, N * 4, N * 4, sort_bytes, N * XW * 4, (size_t)2 * T * 4,
                                    (size_t)2 * T * XW * 4, (size_t)2 * waves1 * 4, (size_t)2 * waves1 * XW * 4,
                                    (size_t)(n_cols + 1) * XW * 4, (size_t)n_cols * XW_IO * 4, out_bytes},
                                   "qap_columns"))
            return rc;
        hipStream_t st = m.stream();
        m.up(SRC, en.src, N * 4);
        m.up(VAL, en.val, N * 32);
        m.up(KEYS, en.col, N * 4);
        m.up(IDS, ids.data(), N * 4);
        u32 *const sums = m.dev<u32>(SUMS);
        m.run([&] {
            ZeroRanges zr{};
            zr.p[0] = sums, zr.n[0] = (u32)((size_t)(n_cols + 1) * XW);
            hipLaunchKernelGGL((zero_ranges<F>), dim3(zr.n[0] > 256u * 1024u ? 1024u : cdiv(zr.n[0], 256)), dim3(256), 0, st, zr);
            return sort_pairs(m.dev<u32>(KEYS), m.dev<u32>(SKEYS), m.dev<u32>(IDS), m.dev<u32>(SIDS), N, end_bit, m.dev(SORT), sort_bytes, st);
        });
        m.run([&] {
            hipLaunchKernelGGL((qap_entry_kernel<F, FrC>), dim3(cdiv(N, 256)), dim3(256), 0, st, m.dev<u32>(SIDS), (u32)N, m.dev<u32>(SRC),
                               m.dev<u32>(VAL), d_bases, m.dev<u32>(PROD));
            hipLaunchKernelGGL((qap_segsum_kernel<F>), dim3(cdiv(T, 256)), dim3(256), 0, st, m.dev<u32>(SKEYS), m.dev<u32>(PROD), (u32)N, L,
                               invalid, sums, m.dev<u32>(PK0), m.dev<u32>(PP0), T);
            u32 *pk[2] = {m.dev<u32>(PK0), m.dev<u32>(PK1)}, *pp[2] = {m.dev<u32>(PP0), m.dev<u32>(PP1)};
            merge_levels(st, pk, pp, 2 * T, merge_g1(N), invalid, sums, (u32 *)nullptr);
            hipLaunchKernelGGL((group_scale_store_kernel<F>), dim3(cdiv(n_cols, 256)), dim3(256), 0, st, sums, (const u32 *)nullptr,
                               (size_t)n_cols, m.dev<u32>(STD));
            xyzz_to_affine_launch<FIO>(st, m.dev<u32>(STD), (size_t)n_cols, m.dev<u32>(AFF), AW_IO);
        });
        m.down(stage.data(), AFF, out_bytes);
        if (const int rc = m.finish()) return rc;
        std::memcpy(out_affine_host, stage.data(), out_bytes);
        return MG_OK;
    }

  private:
    // ---------------------------------------------------------------- the stages of msm_launch
    struct Launch { // one msm_launch, handed from stage to stage (msm_launch initialises bs .. pl, in this order)
        const BaseSet *bs;
        const u32 *d_scalars;
        MsmWorkspace *ws;
        hipStream_t s, side; // side: plain sums of the front levels beside the weighted chain (stand-alone MSMs)
        size_t n, n_scalars, scalar_stride_words;
        int scalar_mode;
        u32 batch, nsets;
        bool batched_pass, sparse;
        MsmPlan pl;
        size_t M;
        int end_bit;
        u32 KB, seg_keys, nb, invalid, T, sort_mask = 0xffffffffu, sort_inv = 0xffffffffu; // sort_pairs: the full key unless masked
        bool direct, per_query, acc_single;
        bool dense; // the fused front end (msm_dense_front_applies): n W pairs, zero digits included, no device count
        u32 *d_count;
        const u32 *skeys, *svals; // the sorted pairs
        u32 parts;                // partials the accumulate kernel leaves for the merge levels
        // what the scan kernels reduce: (array, points per segment, first item, items) -- the buckets or the last front level's A
        const u32 *rin;
        u32 rstride, roff, rn;
        MsmTail tail;
    };

    // The pair count and the layout of the bucket keys of a launch (r.M, KB, seg_keys, nb, invalid), or MG_ERR_ARG for what the
    // 32-bit pairs cannot hold: 2^31 pairs, a key space of 2^24, a base index of 2^31.
    static int key_layout(Launch &r) {
        const MsmPlan &pl = r.pl;
        r.M = r.n * (size_t)pl.W * r.batch;
        // full tables: a digit addresses its summand, every pair of a scalar vector carries the same key and the "bucket" is the result
        r.KB = pl.full ? 1u : pl.B; // bucket keys per bucket window
        if (r.M >= (1ull << 31) || (size_t)r.batch * r.nsets * pl.Wb * r.KB >= (1ull << 24)) return MG_ERR_ARG;
        // with precomputed tables the base index is w*stride + i: table w starts bs->n points after w-1
        // (window tables: + the infinity record behind the last one)
        if ((size_t)pl.W * r.bs->n * (pl.full ? pl.B : 1u) + (pl.precomp && !pl.full ? 1u : 0u) >= (1ull << 31)) return MG_ERR_ARG;
        r.seg_keys = (u32)pl.Wb * r.KB;            // bucket keys per (scalar vector, query)
        r.nb = r.batch * r.nsets * r.seg_keys;     // real buckets; key nb = INVALID
        r.invalid = r.nb;
        return MG_OK;
    }

    // the sizes of the launch, the reservations of everything up to the merge levels, the layout of the keys
    int launch_reserve(Launch &r) {
        MsmWorkspace *const ws = r.ws; const MsmPlan &pl = r.pl;
        int rc;
        if ((rc = key_layout(r))) return rc;
        const size_t M = r.M;
        // A dense single MSM on window tables, stand-alone (not a proof slot's, not on a caller's stream, not being captured): the
        // fused front end. Every digit is a pair -- a zero digit points at the infinity record -- so there is no `invalid` key, no
        // pair count on the device and no unsorted stream to reserve.
        hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
        const bool stand_alone = !ws->capturing && !ws->run_on && !ws->in_graph_slot &&
                                 hipStreamIsCapturing(r.s, &cst) == hipSuccess && cst == hipStreamCaptureStatusNone;
        // (the witness map's work form -- the h MSM of a proof pass, never stand-alone -- is not compiled into the fused kernels)
        r.dense = msm_knobs().dense_front && stand_alone && r.bs->inf_record && r.scalar_mode != SCALARS_WORK &&
                  msm_dense_front_applies(r.batch, r.nsets, pl.W, pl.full ? 2 : (pl.precomp ? 1 : 0), r.sparse);
        if (pl.full) r.sparse = true; // compacting digit kernel: no invalid keys, so a single MSM needs no sort at all
        const u32 seg_keys = r.seg_keys, nb = r.nb, invalid = r.invalid;
        if ((rc = ws->keys_out.reserve(M * 4)) || (rc = ws->vals_out.reserve(M * 4)) ||
            (!r.dense && ((rc = ws->keys_in.reserve(M * 4)) || (rc = ws->vals_in.reserve(M * 4)))))
            return rc;
        if ((rc = ws->sort_tmp.reserve(sort_pairs_temp_bytes(M, r.dense ? cdiv(r.n, 256) : 0))) ||
            (rc = ws->buckets.reserve((size_t)(nb + 1) * XW * 4)))
            return rc;
        const u32 T = r.T = cdiv(M, pl.L);
        if ((rc = ws->pkeys[0].reserve((size_t)2 * T * 4)) || (rc = ws->ppts[0].reserve((size_t)2 * T * XW * 4)))
            return rc;
        const u32 waves1 = cdiv((size_t)2 * T, 64);
        if ((rc = ws->pkeys[1].reserve((size_t)2 * waves1 * 4)) ||
            (rc = ws->ppts[1].reserve((size_t)2 * waves1 * XW * 4)))
            return rc;

        int end_bit = 1;
        while ((1u << end_bit) <= invalid) ++end_bit;
        // the fixed layout marks a zero digit with the key `invalid` = one past the last bucket; where that key alone would cost
        // the sort another 8-bit pass (2^16 buckets: c = 17 tables) the compacting digit kernel is used instead -- its second walk
        // over the digits is a fifth of a radix pass
        int end_bit_real = 1;
        while (nb > 1 && (1u << end_bit_real) <= nb - 1) ++end_bit_real;
        if ((end_bit + 7) / 8 > (end_bit_real + 7) / 8 && !r.dense) r.sparse = true;
        if (r.sparse || r.dense) end_bit = end_bit_real; // no pair carries the invalid key there
        // Several scalar vectors in the fixed layout (the dense h MSM of a batched pass): the digit kernel writes vector q's pairs
        // behind vector q - 1's, and key = q * seg_keys + bucket with seg_keys a power of two -- a stable sort by the BUCKET bits
        // (+ one value for the invalid key) keeps every (q, bucket) run contiguous and needs bits(seg_keys) + 1 bits instead of
        // bits(batch * seg_keys) + 1: 14 instead of 19 for 32 proofs at c = 14, two radix passes over 40 M pairs instead of three
        // (sort.hip sort_key). MANTA_SORT_LOW=0: the full key (A/B).
        if (msm_knobs().sort_low && !r.sparse && r.batch > 1 && r.nsets == 1 && (seg_keys & (seg_keys - 1)) == 0) {
            int eb = 1;
            while ((1u << eb) <= seg_keys) ++eb; // keys 0 .. seg_keys - 1, and seg_keys for the invalid ones
            if ((eb + 7) / 8 < (end_bit + 7) / 8) r.sort_mask = seg_keys - 1, r.sort_inv = invalid, end_bit = eb;
        }
        r.end_bit = end_bit;
        // zero digits are compacted away by the digit kernel; how many pairs remain is known on the device only
        if (r.sparse && sort_pairs_takes_device_count(end_bit)) {
            if ((rc = ws->count.reserve(256))) return rc;
            r.d_count = ws->count.as<u32>();
        }
        // one key in all (full tables, one scalar vector): the run the last merge level closes IS the result -- it is stored in the
        // host's format straight away (no bucket array, no reduce launch: one node fewer on the latency chain of a proof's MSM)
#ifdef MG_NO_DIRECT // A/B builds (tools/build_variant.sh)
        r.direct = false;
#else
        r.direct = nb == 1;
#endif
        if (r.direct && ((rc = ws->redA.reserve((size_t)XWM * 4)) || (rc = ws->redS.reserve((size_t)XWM * 4)))) return rc;
        ws->timed = kernel_timing() && !ws->capturing;
        if (ws->timed && !ws->h_clk) MG_HIP(hipHostMalloc((void **)&ws->h_clk, 64, hipHostMallocDefault));
        return MG_OK;
    }
    static constexpr int XWM = XW > XW_IO ? XW : XW_IO; // a point in either format

    // the zero-fills, then the digit kernel: (key, value) pairs
    void launch_digits(Launch &r) {
        MsmWorkspace *const ws = r.ws; hipStream_t s = r.s;
        // every zero-fill of this launch, up front (none of the targets is touched by the digit kernel or the sort)
        ZeroRanges zr{};
        zr.p[0] = r.d_count, zr.n[0] = r.d_count ? 1u : 0u;
        // direct: no pair at all means the sum is the point at infinity; else the buckets (+ the slot of the invalid key)
        zr.p[1] = r.direct ? ws->redS.as<u32>() : ws->buckets.as<u32>();
        zr.n[1] = r.direct ? (u32)XWM : (u32)((size_t)(r.nb + 1) * XW);
        zr.p[2] = ws->timed ? (u32 *)ws->h_clk : nullptr, zr.n[2] = ws->timed ? 4u : 0u;
        const u32 most = zr.n[1] > 4u ? zr.n[1] : 4u;
        hipLaunchKernelGGL((zero_ranges<F>), dim3(most > 256u * 1024u ? 1024u : cdiv(most, 256)), dim3(256), 0, s, zr);
        if (!r.dense) enqueue_digits(r, ws->keys_in.as<u32>(), ws->vals_in.as<u32>()); // (dense: launch_sort makes the pairs)
        r.batch *= r.nsets; // from here on every (vector, query) pair is a vector of its own: its keys, its window sums, its result
    }
    // the digit kernel of a launch, writing its pairs to (keys, vals); sets r.per_query
    static void enqueue_digits(Launch &r, u32 *keys, u32 *vals) {
        const MsmPlan &pl = r.pl; const BaseSet *const bs = r.bs; hipStream_t s = r.s;
        // compacting path: fewer, larger workgroups = fewer atomics on the counter
        const u32 dthreads = r.d_count ? msm_knobs().digits_threads : 256u;
        // Concatenated queries on full tables, ONE scalar vector (the a | b_g1 | l MSM of a single proof): every pair's key is its
        // query. One digit launch per query, in stream order, appends query 0's pairs, then query 1's, ... -- the pairs ARE sorted
        // and the radix pass over them (histogram, two scans, scatter: 135-150 us on the chain that ends a W or dense proof) is
        // not run. MANTA_Z3_SORT=1 restores the single launch + sort (A/B).
        const u32 nsets = r.nsets;
        r.per_query = pl.full && nsets > 1 && nsets <= BaseSet::MAX_SETS && r.batch == 1 && r.d_count && !msm_knobs().z3_sort &&
                      bs->set_first[nsets] == (u32)bs->n;
        if (r.per_query) {
            for (u32 q = 0; q < nsets; ++q) {
                const u32 lo = bs->set_first[q], hi = bs->set_first[q + 1];
                if (hi <= lo) continue;
                hipLaunchKernelGGL((digits_kernel<FrC>), dim3(cdiv(hi - lo, dthreads), 1), dim3(dthreads), 0, s, r.d_scalars, hi, pl.c,
                                   pl.W, pl.B, 2, (u32)bs->n, r.scalar_mode, r.invalid, keys, vals,
                                   (const u32 *)bs->d_map, (u32)r.n_scalars, r.scalar_stride_words, r.seg_keys, r.d_count, nsets,
                                   (u32)bs->set_len, lo);
            }
        } else
            hipLaunchKernelGGL((digits_kernel<FrC>), dim3(cdiv(r.n, dthreads), r.batch), dim3(dthreads), 0, s, r.d_scalars, (u32)r.n,
                               pl.c, pl.W, pl.B, pl.full ? 2 : (pl.precomp ? 1 : 0), (u32)bs->n, r.scalar_mode, r.invalid,
                               keys, vals, (const u32 *)bs->d_map, (u32)r.n_scalars,
                               r.scalar_stride_words, r.seg_keys, r.d_count, nsets, (u32)bs->set_len);
    }

    // The fused front end of a dense launch: the scalars -> the pairs sorted by key in (keys_out, vals_out). Pass 0 of the sort
    // runs over tiles of 256 scalars whose pairs both kernels compute (msm_digits.h); the later passes are the sort's own.
    static int enqueue_dense_front(const Launch &r, void *sort_tmp, u32 *keys_out, u32 *vals_out) {
        const MsmPlan &pl = r.pl; const BaseSet *const bs = r.bs; hipStream_t s = r.s;
        const u32 tiles1 = cdiv(r.n, 256);
        const SortScratch t = sort_scratch(sort_tmp, r.M, tiles1);
        const DenseFront a{r.d_scalars, bs->d_map, (u32)r.n, (u32)r.n_scalars, pl.c, pl.W, r.scalar_mode,
                           pl.B, (u32)bs->n, (u32)((size_t)pl.W * bs->n)};
        const bool to_out = ((r.end_bit + 7) / 8 - 1) % 2 == 0; // where sort_pairs would have its pass 0 write
        hipLaunchKernelGGL((digits_hist<FrC>), dim3(tiles1), dim3(256), 0, s, a, tiles1, t.hist);
        sort_scan_hist(t, tiles1, s);
        u32 *const k0 = to_out ? keys_out : t.keys, *const v0 = to_out ? vals_out : t.vals;
        hipLaunchKernelGGL((digits_scatter<FrC>), dim3(tiles1), dim3(256), 0, s, a, tiles1, (const u32 *)t.hist, (const u32 *)t.totals, k0, v0);
        return sort_pairs(k0, keys_out, v0, vals_out, r.M, r.end_bit, sort_tmp, sort_pairs_temp_bytes(r.M, tiles1), s, nullptr,
                          0xffffffffu, 0xffffffffu, 1, tiles1);
    }

    int launch_sort(Launch &r) {
        MsmWorkspace *const ws = r.ws;
        if (r.dense) {
            r.skeys = ws->keys_out.as<u32>(), r.svals = ws->vals_out.as<u32>();
            return enqueue_dense_front(r, ws->sort_tmp.p, ws->keys_out.as<u32>(), ws->vals_out.as<u32>());
        }
        // one key in all (a single MSM on full tables, pairs compacted): any order is sorted; one digit launch per query: sorted
        const bool no_sort = (r.nb == 1 || r.per_query) && r.d_count;
        r.skeys = no_sort ? ws->keys_in.as<u32>() : ws->keys_out.as<u32>();
        r.svals = no_sort ? ws->vals_in.as<u32>() : ws->vals_out.as<u32>();
        return no_sort ? MG_OK
                       : sort_pairs(ws->keys_in.as<u32>(), ws->keys_out.as<u32>(), ws->vals_in.as<u32>(), ws->vals_out.as<u32>(), r.M,
                                    r.end_bit, ws->sort_tmp.p, sort_pairs_temp_bytes(r.M), r.s, r.d_count, r.sort_mask, r.sort_inv);
    }

    // the accumulate kernel: the sorted pairs -> one partial per chunk (or per workgroup) and key
    int launch_accumulate(Launch &r) {
        MsmWorkspace *const ws = r.ws; const MsmPlan &pl = r.pl; const BaseSet *const bs = r.bs; hipStream_t s = r.s;
        // Compacted pairs (witness MSMs: two thirds of the digits are zero): the host sized T for all n W digits, so the pairs
        // that remain fill an arbitrary part of it -- 1.35 rounds of wavefronts for the G2 MSM of a PrivateTransfer proof, i.e. two
        // rounds of 6 dependent additions where one round of 9 does, and 1.4 wavefronts per SIMD for a batched pass where two
        // balanced ones do. Launch one round of lanes and let the kernel derive the chunk length from the pair count.
        u32 Tl = r.T, adapt = 0;
        u32 Lk = pl.L; // the chunk length the kernel starts from (all of it where the pair count is the host's: no count, no adapt)
        // single-key MSMs sum inside the workgroup: one partial per workgroup (MANTA_ACC_SINGLE=0: the general kernel, A/B)
        const bool acc_single_on = ((msm_knobs().acc_single >> (GROUP - 1)) & 1) != 0;
        const int dev_now = current_device();
        const bool acc_single = r.acc_single = r.nb == 1 && r.d_count && acc_single_on && !(kernel_timing() && !ws->capturing) &&
                                               dev_now >= 0 && dev_now < 64 && occ_[dev_now].cus.load(std::memory_order_acquire) &&
                                               occ_[dev_now].blocks_single;
        if (r.d_count) {
            const u32 tgt = acc_round_lanes(r.batched_pass, acc_single);
            if (tgt && Tl > tgt) Tl = tgt, adapt = 1;
            // one LARGE scalar vector (host chunk length above 6: 2^20 scalars): whatever the lane count came to, the pair count
            // decides (a batched pass that fits one round keeps its host-side chunk length: measured, -12 % otherwise)
            else if (tgt && !r.batched_pass && pl.L > 6) adapt = 1;
            // The kernel takes max(Lk, ceil(pairs / lanes)). The host's L is sized for ALL n W digits (2^20 scalars: 120 entries per
            // lane): on a witness of which a tenth survives the compaction it left nine SIMDs in ten idle and the others walking 120
            // dependent additions -- the 2^20 BLS12-381 G2 accumulate of BASELINE configs[2] took 7.6 ms for 0.9 M pairs
            // (profiles/r04_config2_timeline.txt). With the round of lanes fixed the pair count alone decides the chunk length.
            if (adapt && Lk > 6) Lk = 6;
        }
        const u32 M = (u32)r.M, invalid = r.invalid;
        if (ws->timed) MG_HIP(hipEventRecord(ws->t0, s));
#ifdef MG_CALIBRATION
        static const bool gather_only = std::getenv("MANTA_ACC_GATHER_ONLY") != nullptr; // -DMG_CALIBRATION build only (wrong results)
        if (gather_only)
            hipLaunchKernelGGL((gather_only_chunks<F>), dim3(cdiv(r.T, 256)), dim3(256), 0, s, ws->keys_out.as<u32>(),
                               ws->vals_out.as<u32>(), M, pl.L, invalid, bs->d_pts, (u32)AWS, ws->pkeys[0].as<u32>(), r.T,
                               (const u32 *)r.d_count);
        else
#endif
        if (acc_single)
            hipLaunchKernelGGL((accumulate_single<F>), dim3(cdiv(Tl, 256)), dim3(256), AccSingle<F>::LDS_BYTES, s, r.svals, M, Lk, bs->d_pts, (u32)AWS,
                               ws->pkeys[0].as<u32>(), ws->ppts[0].as<u32>(), Tl, (const u32 *)r.d_count, adapt, invalid);
        else
        if (ws->timed)
            hipLaunchKernelGGL((accumulate_chunks<F, true>), dim3(cdiv(Tl, 256)), dim3(256), 0, s, r.skeys,
                               r.svals, M, Lk, invalid, bs->d_pts, (u32)AWS, ws->buckets.as<u32>(),
                               ws->pkeys[0].as<u32>(), ws->ppts[0].as<u32>(), Tl, (const u32 *)r.d_count, ws->h_clk, adapt);
        else
            hipLaunchKernelGGL((accumulate_chunks<F, false>), dim3(cdiv(Tl, 256)), dim3(256), 0, s, r.skeys,
                               r.svals, M, Lk, invalid, bs->d_pts, (u32)AWS, ws->buckets.as<u32>(),
                               ws->pkeys[0].as<u32>(), ws->ppts[0].as<u32>(), Tl, (const u32 *)r.d_count, (unsigned long long *)nullptr, adapt);
        if (ws->timed) MG_HIP(hipEventRecord(ws->t1, s));
        r.parts = acc_single ? cdiv(Tl, 256) : 2 * Tl;
        return MG_OK;
    }

    // merge levels: the partials -> the bucket array (direct: the result, in redS)
    void launch_merge(Launch &r) {
        MsmWorkspace *const ws = r.ws;
        u32 *pk[2] = {ws->pkeys[0].as<u32>(), ws->pkeys[1].as<u32>()}, *pp[2] = {ws->ppts[0].as<u32>(), ws->ppts[1].as<u32>()};
        merge_levels(r.s, pk, pp, r.parts, r.acc_single ? 2u : merge_g1(r.M), r.invalid, ws->buckets.as<u32>(),
                     r.direct ? ws->redS.as<u32>() : (u32 *)nullptr);
    }
    // The merge levels over `cnt` partials in (pkeys[0], ppts[0]), ping-ponging with (pkeys[1], ppts[1]) until one wave is left:
    // 64 G -> 2 entries per wave and level, complete runs to `buckets` (the last level: std_final, if given). G0 = entries
    // folded serially per lane in the first level, which is throughput-bound (as many entries as accumulate lanes x 2); later
    // levels are pure latency (G = 2); <= 512 entries finish in one wave. Shared by msm_launch and qap_columns.
    static void merge_levels(hipStream_t st, u32 *const pkeys[2], u32 *const ppts[2], u32 cnt, u32 G0, u32 invalid, u32 *buckets,
                             u32 *std_final) {
        int src = 0;
        for (int level = 0;; ++level) {
            u32 G = level == 0 ? G0 : 2;
            if (cnt <= 512) G = cnt <= 64 ? 1 : cdiv(cnt, 64);
            const u32 waves = cdiv(cdiv(cnt, G), 64);
            const int fin = waves == 1;
            merge_partials_launch(st, waves, pkeys[src], ppts[src], cnt, G, invalid, fin, buckets, pkeys[1 - src], ppts[1 - src], std_final);
            if (fin) break;
            cnt = 2 * waves;
            src ^= 1;
        }
    }

    // ---- bucket reduce
    // front levels: serial_reduce levels over the bucket array while a window segment has many buckets, each leaving one extra
    // point per segment and an A array for the next; the scan kernels take what is left
    int launch_front_levels(Launch &r) {
        MsmWorkspace *const ws = r.ws; const MsmPlan &pl = r.pl; hipStream_t s = r.s; MsmTail &t = r.tail;
        const u32 segs = t.segs = r.batch * (u32)pl.Wb;
        r.rin = ws->buckets.as<u32>(), r.rstride = r.KB, r.roff = 0, r.rn = r.KB;
        const MsmKnobs &rk = msm_knobs();
        // Work-efficient front levels: on (8 buckets per lane, 16 from 2^16 buckets on) wherever a window segment has >= min_items
        // buckets (profiles/r03_front_levels_ab.txt) -- since round 6 inside a proof slot's captured graphs too (the crash of
        // rounds 3-5 was the side stream, below): nothing at manta-pay sizes, whose windows stay below the threshold, -2.4 % on
        // the 2^20 proof of BASELINE configs[2] (profiles/r06_front_levels_in_graph.txt). The plain sums of STAND-ALONE MSMs ride
        // on ONE high-priority side stream per engine (a side stream per workspace aliased the runtime's shared hardware queues).
        const int lgS_eff = rk.lgS >= 0 ? rk.lgS : 3;
        const u32 min_items = r.batched_pass ? rk.min_items_batch : rk.min_items;
        if (lgS_eff <= 0 || r.rn < min_items) return MG_OK;
        // The side stream is for STAND-ALONE launches only, and never for a stream that is being captured. Round 6 root cause
        // (profiles/r06_front_levels_in_graph.txt): inside the forked capture of a proof slot the four G1 MSMs are four
        // branches, and the ONE side stream of the engine was forked from and joined into each of them in turn -- the
        // runtime's per-stream lists of "parallel capture streams" became cyclic (branch a <-> side <-> branch b) and
        // hipStreamEndCapture recursed over them until the stack was gone (SIGSEGV in hip::Stream::EndCapture, 25+ frames
        // of itself). That was the "pass fails" of profiles/r05_batched_ab.txt (3) and the reason behind in_graph_slot.
        hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
        const bool being_captured = hipStreamIsCapturing(s, &cst) != hipSuccess || cst != hipStreamCaptureStatusNone;
        if (!ws->capturing && !ws->run_on && !ws->in_graph_slot && !being_captured && rk.side) {
            // ONE side stream per engine, high priority (= the runtime's other pool of hardware queues)
            if (!(r.side = engine_side_stream())) return MG_ERR_HIP;
            if (!ws->side_fork) {
                MG_HIP(hipEventCreateWithFlags(&ws->side_fork, hipEventDisableTiming));
                MG_HIP(hipEventCreateWithFlags(&ws->side_join, hipEventDisableTiming));
            }
            ws->side_stream = r.side; // (for the abandon paths: they drain it; not owned by the workspace)
        }
        // two passes over the same loop: sizes first (one reservation), then the launches
        for (int pass = 0; pass < 2; ++pass) {
            size_t used = 0; // points
            auto take = [&](size_t pts) {
                u32 *p = pass ? ws->front.as<u32>() + used * XW : nullptr;
                used += pts;
                return p;
            };
            const u32 *in = ws->buckets.as<u32>();
            u32 stride = pl.B, off = 0, n = pl.B, shift = 0, ne = 0;
            while (n >= min_items && ne < (u32)MsmTail::MAX_EXTRA) {
                // the big first levels are throughput-bound: short stretches = enough lanes for two wavefronts per SIMD;
                // below that a level is a latency chain either way and longer stretches save a level (2^16 buckets: 16 per lane
                // leaves the scan kernels the 4 096 items they take at c = 16)
                const int lg = (size_t)segs * n >= ((size_t)1 << 18) ? rk.lgS0 : (rk.lgS < 0 && n >= (1u << 16) ? 4 : lgS_eff);
                const u32 lanes = cdiv(n, 1u << lg);
                u32 *A = take((size_t)segs * lanes), *Sx = take((size_t)segs * lanes);
                if (pass) serial_reduce_launch(s, (size_t)segs * lanes, in, stride, off, n, 1u << lg, lanes, A, Sx);
                // plain sum of the Sx_t: serial partial sums until one tile per segment is left, then one wavefront
                hipStream_t ps = r.side ? r.side : s;
                if (pass && r.side) {
                    MG_HIP(hipEventRecord(ws->side_fork, s));
                    MG_HIP(hipStreamWaitEvent(r.side, ws->side_fork, 0));
                }
                const u32 *pin = Sx;
                u32 pcnt = lanes;
                while (pcnt > 64) {
                    int plg = rk.lgSP;
                    while (plg > 1 && (pcnt >> plg) < 32 && pcnt > 64u << 1) --plg; // do not shrink below a tile
                    const u32 pl2 = cdiv(pcnt, 1u << plg);
                    u32 *tp = take((size_t)segs * pl2);
                    if (pass) serial_reduce_launch(ps, (size_t)segs * pl2, pin, pcnt, 0u, pcnt, 1u << plg, pl2, tp, (u32 *)nullptr);
                    pin = tp;
                    pcnt = pl2;
                }
                if (pass)
                    tile_reduce_launch(ps, segs, true, pin, pcnt, 0u, pcnt, 1u, ws->extra.as<u32>() + (size_t)ne * segs * XW_IO,
                                       (u32 *)nullptr, 1);
                t.extra_shift[ne++] = shift;
                shift += lg;
                in = A, stride = lanes, off = 1, n = lanes - 1;
            }
            int rc;
            if (pass) r.rin = in, r.rstride = stride, r.roff = off, r.rn = n, t.tail_shift = shift, t.n_extra = ne;
            else if ((rc = ws->front.reserve(used * XW * 4)) || (rc = ws->extra.reserve((size_t)MsmTail::MAX_EXTRA * segs * XW_IO * 4)))
                return rc;
        }
        return MG_OK;
    }

    // the scan kernels over what the front levels left (or the bucket array): the tail in one of the MsmTail layouts
    int launch_scan_tail(Launch &r) {
        MsmWorkspace *const ws = r.ws; hipStream_t s = r.s; MsmTail &t = r.tail;
        const u32 segs = t.segs, T0 = cdiv(r.rn, 64);
        int rc;
        if (r.direct) { // the last merge level left the result in redS
            t.extra_off_pts = segs;
        } else if (T0 == 1) { // a single tile per window: its S is the window sum
            if ((rc = ws->redA.reserve((size_t)segs * XWM * 4)) || (rc = ws->redS.reserve((size_t)segs * XWM * 4))) return rc;
            // (rn = 1, full tables: the scan kernel has no addition to make, it converts the point)
            tile_reduce_launch(s, segs, r.rn > 1, r.rin, r.rstride, r.roff, r.rn, 1u, ws->redA.as<u32>(), ws->redS.as<u32>(), 1);
            t.extra_off_pts = segs;
        } else if (T0 <= 64) { // two launches: tiles, then (X, sumS) per window
            if ((rc = ws->redA.reserve((size_t)segs * T0 * XW * 4)) || (rc = ws->redS.reserve((size_t)segs * T0 * XW * 4)) ||
                (rc = ws->misc.reserve((size_t)segs * 2 * XW_IO * 4)))
                return rc;
            tile_reduce_launch(s, segs * T0, true, r.rin, r.rstride, r.roff, r.rn, T0, ws->redA.as<u32>(), ws->redS.as<u32>(), 0);
            reduce_level1_launch(s, segs, ws->redA.as<u32>(), ws->redS.as<u32>(), T0, ws->misc.as<u32>());
            t.kind = TAIL_X_SUMS;
            t.extra_off_pts = (size_t)segs * 2;
        } else {
            if ((rc = ws->redA.reserve((size_t)segs * T0 * XWM * 4)) || (rc = ws->redS.reserve((size_t)segs * T0 * XWM * 4)))
                return rc;
            tile_reduce_launch(s, segs * T0, false, r.rin, r.rstride, r.roff, r.rn, T0, ws->redA.as<u32>(), ws->redS.as<u32>(), 0);
            const u32 T1 = t.T1 = cdiv(T0 - 1, 64); // level 1 over A0[1..T0-1]
            const u32 nP = t.nP = cdiv(T0, 64);     // plain sums of S0[0..T0-1]
            if ((rc = ws->misc.reserve((size_t)segs * (2 * T1 + nP) * XW_IO * 4))) return rc;
            u32 *A1 = ws->misc.as<u32>();
            u32 *S1 = A1 + (size_t)segs * T1 * XW_IO;
            u32 *P0 = S1 + (size_t)segs * T1 * XW_IO;
            tile_reduce_launch(s, segs * T1, true, ws->redA.as<u32>(), T0, 1u, T0 - 1, T1, A1, S1, 1);
            tile_reduce_launch(s, segs * nP, true, ws->redS.as<u32>(), T0, 0u, T0, nP, P0, (u32 *)nullptr, 1);
            t.kind = TAIL_TWO_LEVELS;
            t.extra_off_pts = (size_t)segs * (2 * T1 + nP);
        }
        t.d_tail = t.kind == TAIL_WINDOW_SUMS ? ws->redS.as<u32>() : ws->misc.as<u32>(); // the extras follow it in h_stage
        return MG_OK;
    }

    // the tail and the extras of the front levels -> h_stage (pinned); the side stream joins first
    int launch_stage(Launch &r) {
        MsmWorkspace *const ws = r.ws; hipStream_t s = r.s; MsmTail &t = r.tail;
        const size_t stage_pts = t.extra_off_pts, extra_pts = (size_t)t.n_extra * t.segs;
        // small results (every MSM of a proof) leave through stage_and_notify_kernel; large ones keep the runtime's copy
        const bool own_stage = ws->notify || (stage_pts + extra_pts) * XW_IO <= 16384;
        if (const int rc = stage_reserve(ws, (stage_pts + extra_pts) * XW_IO * 4)) return rc;
        if (!own_stage) MG_HIP(hipMemcpyAsync(ws->h_stage, t.d_tail, stage_pts * XW_IO * 4, hipMemcpyDeviceToHost, s));
        if (t.n_extra && r.side) { // the plain sums ran on the side stream: join
            MG_HIP(hipEventRecord(ws->side_join, r.side));
            MG_HIP(hipStreamWaitEvent(s, ws->side_join, 0));
        }
        if (t.n_extra && !own_stage)
            MG_HIP(hipMemcpyAsync((u32 *)ws->h_stage + stage_pts * XW_IO, ws->extra.p, extra_pts * XW_IO * 4, hipMemcpyDeviceToHost, s));
        if (own_stage) {
            // The staged points leave through a kernel of ours (no copy node of the runtime's in a captured graph), and where the host
            // polls for the end of this chain, the same kernel raises the token. The host polls *h_flag to learn that THIS chain has ended (prover.cpp finish_pass_body). Rounds 4-5 wrote the staged
            // points with one D2H copy and the token with a second one behind it in the same stream: stream order says when each
            // copy may START, not in which order two different dispatches' writes become visible to a host that polls memory -- the
            // soak (tools/soak.py, distinct assignments) caught one single proof in ~10^5 whose a / l sum was read before it had
            // arrived (A and C, or C alone, wrong; status 0). One kernel now writes the staged points to pinned memory, fences at
            // system scope, and only then writes the token.
            if (ws->notify && !ws->h_flag) {
                MG_HIP(hipHostMalloc((void **)&ws->h_flag, 64, hipHostMallocDefault));
                *ws->h_flag = 0;
            }
            hipLaunchKernelGGL(stage_and_notify_kernel, dim3(1), dim3(256), 0, s, t.d_tail, (u32 *)ws->h_stage, (u32)(stage_pts * XW_IO),
                               (const u32 *)ws->extra.p, (u32 *)ws->h_stage + stage_pts * XW_IO, (u32)(extra_pts * XW_IO),
                               ws->notify ? ws->h_flag : (u32 *)nullptr);
        }
        return MG_OK;
    }
};

} // namespace mg
