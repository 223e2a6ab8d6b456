// Host layer of batched Poseidon and the Merkle-tree hashing (mantagpu.h mg_poseidon_* / mg_merkle_*): parameter decoding,
// argument checks (all before any device work), chunking, and the one schedule of every tree call: an append, which a build is
// from the empty state. Kernels and their launch functions in poseidon.h.
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

// f(the launch functions of the hasher's field); they are compiled in poseidon_<curve>.hip only
template <class F> hipError_t on_field(const mg_poseidon *h, F f) {
    return h->curve == 0 ? f(PoseidonKernels<Bn254FrCfg>{}) : f(PoseidonKernels<Bls381FrCfg>{});
}

size_t prm_bytes(const mg_poseidon *h) { return h->prm.size() * 8; }
PoseidonDev on_device(const mg_poseidon *h, const void *d_prm) {
    return PoseidonDev{(const u32 *)d_prm, h->width, h->full / 2, h->partial};
}

// a permute (in place: one device array, 2^19 x 192 B at width 6) or hash launch over n items from host memory, POSEIDON_CHUNK
// at a time, pageable: copies go straight from and to the caller's arrays
template <class Launch> int run(const mg_poseidon *h, const std::vector<Span> &arrays, size_t n, Launch launch) {
    return run_chunks(Staging{POSEIDON_CHUNK, false}, n, h->prm.data(), prm_bytes(h), arrays, 0,
                      [&](const Chunk &c) { return launch(c, on_device(h, c.consts)); });
}

bool tree_args_ok(const mg_poseidon *h, unsigned height) { return h && h->width == 3 && height >= 2 && height <= 32; }

// One pass over a forest in the caller's memory, already checked. A null pointer is something the call does without: no old
// state = every tree starts empty (a build), no request trees = every request is on tree 0, an output that is not wanted.
struct MerkleWork {
    const u64 *old_counts = nullptr, *old_last = nullptr, *old_paths = nullptr; // the state before, all three or none
    const u64 *n_new = nullptr;  // [n_trees] leaf counts after
    const u64 *leaves = nullptr; // the appended leaves of the trees, back to back
    u64 *roots_out = nullptr, *new_last = nullptr, *new_paths = nullptr;
    const u64 *path_trees = nullptr, *path_indices = nullptr; // k Paths of new leaves -> paths_out
    size_t k = 0;
    u64 *paths_out = nullptr;
    const u64 *refresh_trees = nullptr, *refresh_indices = nullptr; // m Paths of older leaves, refreshed in refresh_paths
    size_t m = 0;
    u64 *refresh_paths = nullptr;
};

// Appends to every tree of a forest the leaves that take it from its old count to n_new, gathers the k requested Paths of new
// leaves and refreshes the m Paths of older ones. Device memory follows the work: the recomputed nodes of every level (level 0 =
// the new leaves; at most 2 B + n_trees x height for B leaves), the states and the requests. Levels below l0 -- the first with at
// most MERKLE_TOP recomputed nodes per tree -- take one launch each over all trees, the top kernel finishes every tree in LDS,
// one gather launch writes paths, current paths and last leaves; it is left out when neither paths nor the new state are wanted.
int merkle_grow(const mg_poseidon *h, unsigned height, size_t nt, const MerkleWork &w) {
    if (nt == 0) return MG_OK;
    const size_t T1 = nt + 1, H = height, len = H - 1;
    // the table of the recomputed ranges: level l of tree i holds nodes n_old >> l .. ceil(n_new / 2^l) - 1
    std::vector<u64> off(H * T1), total(H);
    u64 base = 0;
    int l0 = -1;
    for (size_t l = 0; l < H; ++l) {
        u64 mx = 0;
        for (size_t i = 0; i < nt; ++i) {
            const u64 c = ((w.n_new[i] + (u64(1) << l) - 1) >> l) - (w.old_counts ? w.old_counts[i] >> l : 0);
            off[l * T1 + i] = base;
            base += c;
            mx = c > mx ? c : mx;
        }
        off[l * T1 + nt] = base;
        total[l] = base - off[l * T1];
        if (l0 < 0 && (mx <= (u64)MERKLE_TOP || l == H - 1)) l0 = (int)l;
    }
    const size_t pb = prm_bytes(h), n_req = w.k + w.m, path_bytes = len * 32;
    const bool gather = n_req || w.new_last || w.new_paths;
    // parameters | table | counts old, new | last leaves | current paths | chain | nodes | roots | requests | paths | new last
    DevCall d;
    if (const int rc = d.begin({pb, off.size() * 8, nt * 8, nt * 8, nt * 32, nt * path_bytes, nt * 32, base * 32, nt * 32, n_req * 8,
                                n_req * 8, gather ? (n_req + nt) * path_bytes : 0, gather ? nt * 32 : 0},
                               "hipMalloc(merkle)"))
        return rc;
    hipStream_t s = d.stream();
    d.up(0, h->prm.data(), pb);
    d.up(1, off.data(), off.size() * 8);
    if (w.old_counts) {
        d.up(2, w.old_counts, nt * 8);
        d.up(4, w.old_last, nt * 32);
        d.up(5, w.old_paths, nt * path_bytes);
        d.copy(6, 4, nt * 32); // the chain starts at the last leaf
    } else // the empty state, filled in on the device: a tree that stays empty has it copied through
        for (const size_t i : {2, 4, 5, 6}) d.zero(i);
    d.up(3, w.n_new, nt * 8);
    d.up(7, w.leaves, total[0] * 32);
    w.path_trees ? d.up(9, w.path_trees, w.k * 8) : d.zero(9);
    d.up(9, w.refresh_trees, w.m * 8, w.k * 8);
    d.up(10, w.path_indices, w.k * 8);
    d.up(10, w.refresh_indices, w.m * 8, w.k * 8);
    d.up(11, w.refresh_paths, w.m * path_bytes, w.k * path_bytes); // refreshed in place
    const PoseidonDev hd = on_device(h, d.dev(0));
    const MerkleForest t{d.dev<const u64>(2), d.dev<const u64>(3), d.dev<const u32>(4), d.dev<const u32>(5), d.dev<u32>(6),
                         d.dev<u32>(7),       d.dev<const u64>(1), (int)nt,             (int)H};
    const auto launch = [&](auto f) { d.run([&] { return on_field(h, f); }); };
    for (int l = 0; l < l0; ++l) launch([&](auto K) { return K.merkle_level(s, hd, t, l, total[l + 1]); });
    launch([&](auto K) { return K.merkle_top(s, hd, t, l0, d.dev<u32>(8)); });
    if (gather)
        launch([&](auto K) { return K.merkle_gather(s, t, d.dev<const u64>(9), d.dev<const u64>(10), n_req, d.dev<u32>(11), d.dev<u32>(12)); });
    d.down(w.roots_out, 8, nt * 32); // what the caller wants back: not null, not empty
    d.down(w.paths_out, 11, w.k * path_bytes);
    d.down(w.refresh_paths, 11, w.m * path_bytes, w.k * path_bytes);
    d.down(w.new_paths, 11, nt * path_bytes, n_req * path_bytes);
    d.down(w.new_last, 12, nt * 32);
    return d.finish();
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
    return run(h, {Span::inout(states, (size_t)h->width * 32)}, n, [&](const Chunk &c, const PoseidonDev &hd) {
        return on_field(h, [&](auto K) { return K.permute(c.stream, hd, (u32 *)c.a[0], c.n); });
    });
}

int poseidon_hash(const mg_poseidon *h, const u64 *inputs, size_t n, u64 *out) {
    if (!h || (n && (!inputs || !out))) return MG_ERR_ARG;
    return run(h, {Span::in(inputs, (size_t)(h->width - 1) * 32), Span::out(out, 32)}, n, [&](const Chunk &c, const PoseidonDev &hd) {
        return on_field(h, [&](auto K) { return K.hash(c.stream, hd, (const u32 *)c.a[0], c.n, (u32 *)c.a[1]); });
    });
}

int poseidon_hash_device(const mg_poseidon *h, const u64 *d_in, size_t n, u64 *d_out) {
    if (!h || (n && (!d_in || !d_out))) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    DevCall m;
    if (const int rc = m.begin({prm_bytes(h)}, "hipMalloc(poseidon parameters)")) return rc;
    m.up(0, h->prm.data(), prm_bytes(h));
    const PoseidonDev hd = on_device(h, m.dev(0));
    m.run([&] { return on_field(h, [&](auto K) { return K.hash(m.stream(), hd, (const u32 *)d_in, n, (u32 *)d_out); }); });
    return m.finish();
}

// one tree built from its leaves: the append to one empty tree, the k indices as requests on it
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
    const u64 n_new = n;
    MerkleWork w;
    w.n_new = &n_new, w.leaves = leaves, w.roots_out = root_out;
    w.path_indices = indices, w.k = k, w.paths_out = paths_out;
    return merkle_grow(h, height, 1, w);
}

// appends leaves offsets[i] .. offsets[i + 1] - 1 to tree i of a forest known by its state (count, last leaf, current path per
// tree)
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
    const size_t nt = n_trees, len = height - 1;
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
    MerkleWork w;
    w.old_counts = old_counts, w.old_last = old_last, w.old_paths = old_paths;
    w.n_new = n_new.data(), w.leaves = leaves;
    w.roots_out = roots_out, w.new_last = new_last, w.new_paths = new_paths;
    w.path_trees = path_trees, w.path_indices = path_indices, w.k = k, w.paths_out = paths_out;
    w.refresh_trees = refresh_trees, w.refresh_indices = refresh_indices, w.m = m, w.refresh_paths = refresh_paths;
    if (const int rc = merkle_grow(h, height, nt, w)) return rc;
    if (nt) std::memcpy(new_counts, n_new.data(), nt * 8); // last: new_state may be old_state
    return MG_OK;
}

// the roots of trees built from their leaves: the append to empty trees, nothing gathered
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
    MerkleWork w;
    w.n_new = cnt.data(), w.leaves = leaves, w.roots_out = roots_out;
    return merkle_grow(h, height, n_trees, w);
}

} // namespace mg
