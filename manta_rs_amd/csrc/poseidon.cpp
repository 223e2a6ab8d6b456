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
