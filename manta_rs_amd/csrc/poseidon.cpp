// Host layer of batched Poseidon and the Merkle-tree hashing (mantagpu.h mg_poseidon_* / mg_merkle_*): parameter decoding,
// argument checks (all before any device work), chunking, the level schedule of trees and forests. Kernels in poseidon.h.
#include "poseidon.h"
#include "staging.h"
#include <cstring>
#include <vector>

struct mg_poseidon {
    int curve, width, full, partial;
    std::vector<mg::u64> prm; // keys | mds | tag, Montgomery, 4 u64 limbs each (= the device words)
};

namespace mg {

constexpr size_t POSEIDON_CHUNK = size_t(1) << 19; // = MG_POSEIDON_CHUNK of mantagpu.h

namespace {

hipError_t launch(const mg_poseidon *h, PoseidonLaunch a) {
    a.width = h->width;
    a.half_full = h->full / 2;
    a.partial = h->partial;
    return h->curve == 0 ? poseidon_launch_bn254(a) : poseidon_launch_bls381(a);
}

size_t prm_bytes(const mg_poseidon *h) { return h->prm.size() * 8; }

// PERMUTE (in place: one device array, 2^19 x 192 B at width 6) or HASH over n items from host memory, POSEIDON_CHUNK at a time,
// pageable: copies go straight from and to the caller's arrays
int run(const mg_poseidon *h, int op, const std::vector<Span> &arrays, size_t n) {
    return run_chunks(Staging{POSEIDON_CHUNK, false}, n, h->prm.data(), prm_bytes(h), arrays, 0, [&](const Chunk &c) {
        PoseidonLaunch a{};
        a.op = op;
        a.prm = (const u32 *)c.consts;
        a.in = (const u32 *)c.a[0];
        a.out = (u32 *)c.a.back();
        a.n = c.n;
        a.stream = c.stream;
        return launch(h, a);
    });
}

bool tree_args_ok(const mg_poseidon *h, unsigned height) { return h && h->width == 3 && height >= 2 && height <= 32; }

// Roots of n_trees trees of `height` whose leaves lie back to back (cnt[k] each). Levels 0 .. l0 - 1 go through one level kernel
// launch each over all trees, until no tree has more than MERKLE_TOP nodes on level l0; the top kernel finishes each tree in
// LDS. keep (one tree): every level is kept in one buffer and the k paths of `indices` are gathered from it; otherwise levels
// alternate between two buffers.
int merkle_run(const mg_poseidon *h, unsigned height, const u64 *leaves, const std::vector<u64> &cnt, bool keep, u64 *roots,
               const u64 *indices, size_t k, u64 *paths) {
    const size_t nt = cnt.size(), T1 = nt + 1, H = height;
    if (nt == 0) return MG_OK;
    // per-level offsets table: absolute positions in the kept levels, or positions within the level's own buffer
    std::vector<u64> off(H * T1), c(cnt);
    std::vector<u64> total(H);
    u64 base = 0;
    int l0 = -1;
    for (size_t l = 0; l < H; ++l) {
        if (l)
            for (size_t i = 0; i < nt; ++i) c[i] = (c[i] + 1) / 2;
        u64 acc = 0, mx = 0;
        for (size_t i = 0; i < nt; ++i) {
            off[l * T1 + i] = (keep ? base : 0) + acc;
            acc += c[i];
            mx = c[i] > mx ? c[i] : mx;
        }
        off[l * T1 + nt] = (keep ? base : 0) + acc;
        total[l] = acc;
        base += acc;
        if (l0 < 0 && (mx <= (u64)MERKLE_TOP || l == H - 1)) l0 = (int)l;
    }
    hipStream_t s = setup_stream();
    if (!s) return MG_ERR_OOM;
    const size_t pb = prm_bytes(h), tb = off.size() * 8;
    const size_t lvl_bytes = keep ? base * 32 : (total[0] + (H > 1 ? total[1] : 0)) * 32;
    const size_t path_len = H - 1;
    DevBlock m; // parameters | offsets table | levels | roots | path indices | paths
    if (const int rc = m.alloc({pb, tb, lvl_bytes, nt * 32, k * 8, k * path_len * 32}, "hipMalloc(merkle)")) return rc;
    uint8_t *d_prm = m.dev(0), *d_off = m.dev(1), *d_lv = m.dev(2), *d_roots = m.dev(3), *d_idx = m.dev(4), *d_paths = m.dev(5);
    uint8_t *buf[2] = {d_lv, keep ? d_lv : d_lv + total[0] * 32}; // level l lives in buf[l & 1]
    MG_HIP(hipMemcpyAsync(d_prm, h->prm.data(), pb, hipMemcpyHostToDevice, s));
    MG_HIP(hipMemcpyAsync(d_off, off.data(), tb, hipMemcpyHostToDevice, s));
    if (total[0]) MG_HIP(hipMemcpyAsync(d_lv, leaves, total[0] * 32, hipMemcpyHostToDevice, s));
    const u64 *d_table = (const u64 *)d_off;
    PoseidonLaunch a{};
    a.prm = (const u32 *)d_prm;
    a.n_trees = (int)nt;
    a.height = (int)H;
    a.stream = s;
    for (int l = 0; l < l0; ++l) {
        a.op = PoseidonLaunch::LEVEL;
        a.in = (const u32 *)buf[l & 1];
        a.src_off = d_table + l * T1;
        a.out = (u32 *)buf[(l + 1) & 1];
        a.dst_off = d_table + (l + 1) * T1;
        a.n = total[l + 1];
        MG_HIP(launch(h, a));
    }
    a.op = PoseidonLaunch::TOP;
    a.in = (const u32 *)buf[l0 & 1];
    a.src_off = d_table;
    a.level = l0;
    a.keep = keep ? (u32 *)d_lv : nullptr;
    a.roots = (u32 *)d_roots;
    MG_HIP(launch(h, a));
    if (keep && k) {
        MG_HIP(hipMemcpyAsync(d_idx, indices, k * 8, hipMemcpyHostToDevice, s));
        a.op = PoseidonLaunch::PATHS;
        a.in = (const u32 *)d_lv;
        a.n = k;
        a.indices = (const u64 *)d_idx;
        a.out = (u32 *)d_paths;
        MG_HIP(launch(h, a));
        MG_HIP(hipMemcpyAsync(paths, d_paths, k * path_len * 32, hipMemcpyDeviceToHost, s));
    }
    MG_HIP(hipMemcpyAsync(roots, d_roots, nt * 32, hipMemcpyDeviceToHost, s));
    MG_HIP(hipStreamSynchronize(s));
    return MG_OK;
}

} // namespace

int poseidon_create(int curve, int width, int full_rounds, int partial_rounds, const uint8_t *bytes, size_t len,
                    mg_poseidon **out) {
    if (!out || !bytes || (curve != 0 && curve != 1) || width < 3 || width > 6) return MG_ERR_ARG;
    if (full_rounds <= 0 || (full_rounds & 1) || partial_rounds < 0 || full_rounds + partial_rounds > 4096) return MG_ERR_ARG;
    const size_t count = (size_t)(full_rounds + partial_rounds) * width + (size_t)width * width + 1;
    if (len != count * 32) return MG_ERR_ARG;
    std::vector<u64> prm(count * 4);
    const bool ok = curve == 0 ? decode_canonical_elements<Bn254FrCfg>(bytes, count, prm.data())
                               : decode_canonical_elements<Bls381FrCfg>(bytes, count, prm.data());
    if (!ok) return MG_ERR_ARG;
    *out = new mg_poseidon{curve, width, full_rounds, partial_rounds, std::move(prm)};
    return MG_OK;
}

void poseidon_destroy(mg_poseidon *h) { delete h; }

int poseidon_permute(const mg_poseidon *h, u64 *states, size_t n) {
    if (!h || (n && !states)) return MG_ERR_ARG;
    return run(h, PoseidonLaunch::PERMUTE, {Span::inout(states, (size_t)h->width * 32)}, n);
}

int poseidon_hash(const mg_poseidon *h, const u64 *inputs, size_t n, u64 *out) {
    if (!h || (n && (!inputs || !out))) return MG_ERR_ARG;
    return run(h, PoseidonLaunch::HASH, {Span::in(inputs, (size_t)(h->width - 1) * 32), Span::out(out, 32)}, n);
}

int poseidon_hash_device(const mg_poseidon *h, const u64 *d_in, size_t n, u64 *d_out) {
    if (!h || (n && (!d_in || !d_out))) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    hipStream_t s = setup_stream();
    if (!s) return MG_ERR_OOM;
    DevBlock m;
    if (const int rc = m.alloc({prm_bytes(h)}, "hipMalloc(poseidon parameters)")) return rc;
    MG_HIP(hipMemcpyAsync(m.dev(0), h->prm.data(), prm_bytes(h), hipMemcpyHostToDevice, s));
    PoseidonLaunch a{};
    a.op = PoseidonLaunch::HASH;
    a.prm = m.dev<const u32>(0);
    a.in = (const u32 *)d_in;
    a.out = (u32 *)d_out;
    a.n = n;
    a.stream = s;
    MG_HIP(launch(h, a));
    MG_HIP(hipStreamSynchronize(s));
    return MG_OK;
}

int merkle_tree(const mg_poseidon *h, unsigned height, const u64 *leaves, size_t n, u64 *root_out, const u64 *indices, size_t k,
                u64 *paths_out) {
    if (!tree_args_ok(h, height) || !root_out || (n && !leaves) || (k && (!indices || !paths_out))) return MG_ERR_ARG;
    if ((u64)n > (u64(1) << (height - 1))) return MG_ERR_ARG;
    for (size_t q = 0; q < k; ++q)
        if (indices[q] >= n) return MG_ERR_ARG;
    if (n == 0) { // the empty tree: root = the sentinel 0, and no leaf to take a path of
        std::memset(root_out, 0, 32);
        return MG_OK;
    }
    return merkle_run(h, height, leaves, std::vector<u64>{n}, true, root_out, indices, k, paths_out);
}

// Appends leaves offsets[i] .. offsets[i + 1] - 1 to tree i of a forest known by its state (count, last leaf, current path per
// tree), gathers the k requested Paths of new leaves and refreshes the m Paths of older ones. Device memory follows the work:
// the recomputed nodes (level 0 = the new leaves; at most 2 B + n_trees x height for B leaves), the states and the requests.
// Levels below l0 -- the first with at most MERKLE_TOP recomputed nodes per tree, usually 0 -- take one launch each, the top
// kernel finishes every tree, one gather launch writes paths, current paths and last leaves.
int merkle_forest_append(const mg_poseidon *h, unsigned height, size_t n_trees, const u64 *old_counts, const u64 *old_last,
                         const u64 *old_paths, const u64 *leaves, const u64 *offsets, u64 *roots_out, u64 *new_counts,
                         u64 *new_last, u64 *new_paths, const u64 *path_trees, const u64 *path_indices, size_t k, u64 *paths_out,
                         const u64 *refresh_trees, const u64 *refresh_indices, size_t m, u64 *refresh_paths) {
    if (!tree_args_ok(h, height)) return MG_ERR_ARG;
    if (n_trees && (!old_counts || !old_last || !old_paths || !offsets || !roots_out || !new_counts || !new_last || !new_paths))
        return MG_ERR_ARG;
    if ((k && (!path_trees || !path_indices || !paths_out)) || (m && (!refresh_trees || !refresh_indices || !refresh_paths)))
        return MG_ERR_ARG;
    if (n_trees && offsets[0] != 0) return MG_ERR_ARG;
    const size_t nt = n_trees, T1 = nt + 1, H = height, len = H - 1;
    const u64 cap = u64(1) << len;
    std::vector<u64> n_new(nt);
    for (size_t i = 0; i < nt; ++i) {
        const u64 n_old = old_counts[i];
        if (offsets[i + 1] < offsets[i] || n_old > cap || offsets[i + 1] - offsets[i] > cap - n_old) return MG_ERR_ARG;
        n_new[i] = n_old + (offsets[i + 1] - offsets[i]);
        if (n_old == 0) continue;
        const u64 *path = old_paths + i * len * 4; // a current path has no right siblings (InnerPath::is_current)
        for (size_t l = 0; l < len; ++l)
            if (!(((n_old - 1) >> l) & 1) && (path[4 * l] | path[4 * l + 1] | path[4 * l + 2] | path[4 * l + 3])) return MG_ERR_ARG;
    }
    if (nt && offsets[nt] && !leaves) return MG_ERR_ARG;
    for (size_t q = 0; q < k; ++q)
        if (path_trees[q] >= nt || path_indices[q] < old_counts[path_trees[q]] || path_indices[q] >= n_new[path_trees[q]])
            return MG_ERR_ARG;
    for (size_t q = 0; q < m; ++q)
        if (refresh_trees[q] >= nt || refresh_indices[q] >= old_counts[refresh_trees[q]]) return MG_ERR_ARG;
    if (nt == 0) return MG_OK;
    // the table of the recomputed ranges: level l of tree i holds nodes n_old >> l .. ceil(n_new / 2^l) - 1
    std::vector<u64> off(H * T1), total(H);
    u64 base = 0;
    int l0 = -1;
    for (size_t l = 0; l < H; ++l) {
        u64 mx = 0;
        for (size_t i = 0; i < nt; ++i) {
            const u64 c = ((n_new[i] + (u64(1) << l) - 1) >> l) - (old_counts[i] >> l);
            off[l * T1 + i] = base;
            base += c;
            mx = c > mx ? c : mx;
        }
        off[l * T1 + nt] = base;
        total[l] = base - off[l * T1];
        if (l0 < 0 && (mx <= (u64)MERKLE_TOP || l == H - 1)) l0 = (int)l;
    }
    hipStream_t s = setup_stream();
    if (!s) return MG_ERR_OOM;
    const size_t pb = prm_bytes(h), n_req = k + m, path_bytes = len * 32;
    DevBlock d; // parameters | table | counts old, new | last leaves | current paths | chain | nodes | roots | requests | paths | new last
    if (const int rc = d.alloc({pb, off.size() * 8, nt * 8, nt * 8, nt * 32, nt * path_bytes, nt * 32, base * 32, nt * 32, n_req * 8,
                                n_req * 8, (n_req + nt) * path_bytes, nt * 32},
                               "hipMalloc(merkle append)"))
        return rc;
    const auto up = [&](size_t i, const void *src, size_t bytes, size_t at = 0) {
        return bytes ? hipMemcpyAsync(d.dev(i) + at, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    MG_HIP(up(0, h->prm.data(), pb));
    MG_HIP(up(1, off.data(), off.size() * 8));
    MG_HIP(up(2, old_counts, nt * 8));
    MG_HIP(up(3, n_new.data(), nt * 8));
    MG_HIP(up(4, old_last, nt * 32));
    MG_HIP(up(5, old_paths, nt * path_bytes));
    MG_HIP(hipMemcpyAsync(d.dev(6), d.dev(4), nt * 32, hipMemcpyDeviceToDevice, s)); // the chain starts at the last leaf
    MG_HIP(up(7, leaves, total[0] * 32));
    MG_HIP(up(9, path_trees, k * 8));
    MG_HIP(up(9, refresh_trees, m * 8, k * 8));
    MG_HIP(up(10, path_indices, k * 8));
    MG_HIP(up(10, refresh_indices, m * 8, k * 8));
    MG_HIP(up(11, refresh_paths, m * path_bytes, k * path_bytes)); // refreshed in place
    PoseidonLaunch a{};
    a.prm = d.dev<const u32>(0);
    a.app = MerkleAppend{d.dev<const u64>(2), d.dev<const u64>(3), d.dev<const u32>(4), d.dev<const u32>(5), d.dev<u32>(6),
                         d.dev<u32>(7),       d.dev<const u64>(1), (int)nt,             (int)H};
    a.stream = s;
    for (int l = 0; l < l0; ++l) {
        a.op = PoseidonLaunch::APPEND_LEVEL;
        a.level = l;
        a.n = total[l + 1];
        MG_HIP(launch(h, a));
    }
    a.op = PoseidonLaunch::APPEND_TOP;
    a.level = l0;
    a.roots = d.dev<u32>(8);
    MG_HIP(launch(h, a));
    a.op = PoseidonLaunch::APPEND_GATHER;
    a.n = n_req;
    a.req_trees = d.dev<const u64>(9);
    a.indices = d.dev<const u64>(10);
    a.out = d.dev<u32>(11);
    a.roots = d.dev<u32>(12);
    MG_HIP(launch(h, a));
    const auto down = [&](void *dst, size_t i, size_t bytes, size_t at = 0) {
        return bytes ? hipMemcpyAsync(dst, d.dev(i) + at, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    MG_HIP(down(roots_out, 8, nt * 32));
    MG_HIP(down(paths_out, 11, k * path_bytes));
    MG_HIP(down(refresh_paths, 11, m * path_bytes, k * path_bytes));
    MG_HIP(down(new_paths, 11, nt * path_bytes, n_req * path_bytes));
    MG_HIP(down(new_last, 12, nt * 32));
    MG_HIP(hipStreamSynchronize(s));
    std::memcpy(new_counts, n_new.data(), nt * 8); // last: new_state may be old_state
    return MG_OK;
}

int merkle_forest_roots(const mg_poseidon *h, unsigned height, const u64 *leaves, const u64 *offsets, size_t n_trees,
                        u64 *roots_out) {
    if (!tree_args_ok(h, height) || (n_trees && (!offsets || !roots_out))) return MG_ERR_ARG;
    if (n_trees == 0) return MG_OK;
    if (offsets[0] != 0) return MG_ERR_ARG;
    std::vector<u64> cnt(n_trees);
    for (size_t i = 0; i < n_trees; ++i) {
        if (offsets[i + 1] < offsets[i]) return MG_ERR_ARG;
        cnt[i] = offsets[i + 1] - offsets[i];
        if (cnt[i] > (u64(1) << (height - 1))) return MG_ERR_ARG;
    }
    if (offsets[n_trees] && !leaves) return MG_ERR_ARG;
    return merkle_run(h, height, leaves, cnt, false, roots_out, nullptr, 0, nullptr);
}

} // namespace mg
