// Batched Poseidon over the BN254 / BLS12-381 scalar fields on gfx950, and the hashing inside manta's Merkle trees: the
// permutation and `Hasher::hash` with one state per lane (width t = 3..6 a template parameter, round counts and constants
// runtime data), and the three tree kernels: one level of every tree of a forest, the top levels of each tree in LDS, and path
// gathering. One typed launch function per kernel (PoseidonKernels), instantiated per scalar field in poseidon_<curve>.hip;
// the host layer and the C ABI (mg_poseidon_*, mg_merkle_*) are in poseidon.cpp.
//
// Semantics (manta-pay/src/crypto/poseidon/mod.rs:383-439, hash.rs:111-153): round r adds keys[r t + i] to word i, applies
// x^5 to every word (full round) or to word 0 only (partial round), then new[i] = sum_j mds[t i + j] st[j]; FULL/2 full rounds,
// PARTIAL partial rounds, FULL/2 full rounds. hash(in) = word 0 of the permutation of (domain tag, in_0 .. in_{t-2}).
//
// Arithmetic: the canonical, always fully reduced Fp<Fr> of fp_dev.h (direct form: 3 t + t^2 products per full round, 3 + t^2
// per partial round). The constants are the same for every lane: they sit in one device buffer, keys | mds | tag, read with
// wave-uniform addresses (scalar loads), never copied per lane.
//
// Merkle trees (manta-crypto/src/merkle_tree/{full,inner_tree}.rs): leaves are level 0; node j of level l + 1 is
// hash(node 2j, node 2j + 1) with an absent right child taken as 0; level l holds ceil(n / 2^l) nodes, the rest are the
// sentinel 0. A forest is a table of per-tree segment offsets per level (off[l (n_trees + 1) + k]): tree k's nodes of level l
// are entries off[l][k] .. off[l][k + 1] of the node buffer.
//
// Every tree pass is an append (merkle_tree/{single_path,partial}.rs, tree.rs:351-406, path.rs:416): a tree is known by its leaf
// count n_old, its last leaf and that leaf's Path. Appending b leaves (n_new = n_old + b) computes on level l the nodes
// s_l = n_old >> l .. ceil(n_new / 2^l) - 1; only those are stored (the table's segments hold them, segment entry i = node
// s_l + i). The one older node that work reads is node(l, s_l - 1) for odd s_l, the level's seed: the old path's entry l when
// n_old mod 2^l != 0, else (l = ctz(n_old)) the last leaf's ancestor a_l, a_0 = last leaf, a_{j+1} = hash(path[j], a_j). That
// chain is one extra lane per tree in each level pass (pass l -> l + 1 computes a_{l+1} while l < ctz(n_old)), never a fold of
// its own. Building a tree from its leaves is the append to the empty state: n_old = 0, so s_l = 0, every node of the tree is
// computed, no level has a seed and no chain runs; the old state is then read only for a tree that stays empty (its current path
// and last leaf are copied through), so it must be device memory all the same.
#pragma once
#include "engine.h"
#include "fp_dev.h"
#include "params_gen.h"

namespace mg {

// the device side of one pass over a forest: the state it starts from, the nodes it computes and their table
struct MerkleForest {
    const u64 *n_old, *n_new; // [n_trees] leaf counts before and after (a build: n_old = 0)
    const u32 *last, *cur;    // the old state: last leaves [n_trees], current paths [n_trees][height - 1]
    u32 *anc;                 // [n_trees] the ancestor chain: starts as a copy of `last`, ends as a_ctz(n_old); the top kernel
                              // carries it through LDS for every tree, whether its chain runs or not
    u32 *nodes;               // every recomputed node, level after level
    const u64 *off;           // [height][n_trees + 1] absolute segment offsets into `nodes`
    int n_trees, height;
};

// a hasher on the device: keys | mds | tag in Montgomery words of 8 x u32 per element, and its shape
struct PoseidonDev {
    const u32 *prm;
    int width, half_full, partial;
};

// One launch function per kernel: device pointers, on `s`; nothing is launched for no lanes. Defined below, compiled only where
// they are instantiated (poseidon_bn254.hip, poseidon_bls381.hip): every other unit sees the declarations alone.
template <class C> struct PoseidonKernels {
    static hipError_t permute(hipStream_t s, const PoseidonDev &h, u32 *states, size_t n); // in place; width 3..6
    static hipError_t hash(hipStream_t s, const PoseidonDev &h, const u32 *in, size_t n, u32 *digests);
    // level l -> l + 1 of every tree: n_parents = all nodes of level l + 1 in the table
    static hipError_t merkle_level(hipStream_t s, const PoseidonDev &h, const MerkleForest &t, int l, size_t n_parents);
    // levels l0 .. height - 1 of every tree, each with at most MERKLE_TOP nodes on level l0; roots [n_trees]
    static hipError_t merkle_top(hipStream_t s, const PoseidonDev &h, const MerkleForest &t, int l0, u32 *roots);
    // paths [n_req + n_trees][height - 1]: the requests' (tree, leaf index), refreshed in place, then the new current paths
    static hipError_t merkle_gather(hipStream_t s, const MerkleForest &t, const u64 *req_trees, const u64 *req_idx, size_t n_req,
                                    u32 *paths, u32 *new_last);
};
extern template struct PoseidonKernels<Bn254FrCfg>;
extern template struct PoseidonKernels<Bls381FrCfg>;

constexpr int MERKLE_TOP = 1024; // a level of at most this many nodes per tree is finished in LDS by pos::merkle_top
constexpr int POSEIDON_BLOCK = 256;

namespace pos {

template <class C> MG_DEV Fp<C> sbox(const Fp<C> &x) { // x^5
    const Fp<C> x2 = Fp<C>::sqr(x);
    return Fp<C>::mul(Fp<C>::sqr(x2), x);
}

// The matrix words are loop-invariant: the compiler holds part of them in SGPRs across the rounds and spills the rest into
// VGPR lanes (kernel-resource-usage, BN254: width 3 133 VGPRs / 3 waves per SIMD, width 4 184 / 2, width 5 256 / 1, width 6
// 187 / 2). Making each row's address opaque per use (empty asm) moved the loads but raised width 3 to 180 VGPRs; not kept.
template <class C, int T> MG_DEV void mds_mul(Fp<C> (&st)[T], const u32 *__restrict__ mds) {
    typedef Fp<C> F;
    F nx[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        F acc = F::mul(F::load(mds + (i * T) * 8), st[0]);
#pragma unroll
        for (int j = 1; j < T; ++j) acc = F::add(acc, F::mul(F::load(mds + (i * T + j) * 8), st[j]));
        nx[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < T; ++i) st[i] = nx[i];
}

template <class C, int T> MG_DEV void full_round(Fp<C> (&st)[T], const u32 *__restrict__ keys, const u32 *__restrict__ mds) {
#pragma unroll
    for (int i = 0; i < T; ++i) st[i] = sbox<C>(Fp<C>::add(st[i], Fp<C>::load(keys + i * 8)));
    mds_mul<C, T>(st, mds);
}

template <class C, int T> MG_DEV void partial_round(Fp<C> (&st)[T], const u32 *__restrict__ keys, const u32 *__restrict__ mds) {
#pragma unroll
    for (int i = 0; i < T; ++i) st[i] = Fp<C>::add(st[i], Fp<C>::load(keys + i * 8));
    st[0] = sbox<C>(st[0]);
    mds_mul<C, T>(st, mds);
}

// prm = keys[(2 hf + partial) t] | mds[t t] | tag; the round index is wave-uniform, so every constant is a uniform load
template <class C, int T> MG_DEV void permute(Fp<C> (&st)[T], const u32 *__restrict__ prm, int hf, int partial) {
    const u32 *mds = prm + (size_t)(2 * hf + partial) * T * 8;
    int r = 0;
#pragma unroll 1
    for (; r < hf; ++r) full_round<C, T>(st, prm + r * T * 8, mds);
#pragma unroll 1
    for (; r < hf + partial; ++r) partial_round<C, T>(st, prm + r * T * 8, mds);
#pragma unroll 1
    for (; r < 2 * hf + partial; ++r) full_round<C, T>(st, prm + r * T * 8, mds);
}

template <class C> MG_DEV Fp<C> tag_of(const u32 *__restrict__ prm, int t, int hf, int partial) {
    return Fp<C>::load(prm + (size_t)((2 * hf + partial) * t + t * t) * 8);
}

// the inner hash of the trees: Hasher<Poseidon2>::hash(left, right) = word 0 of permute(tag, left, right)
template <class C> MG_DEV Fp<C> hash2(const Fp<C> &l, const Fp<C> &r, const u32 *__restrict__ prm, int hf, int partial) {
    Fp<C> st[3] = {tag_of<C>(prm, 3, hf, partial), l, r};
    permute<C, 3>(st, prm, hf, partial);
    return st[0];
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
template <class C, int T>
__global__ __launch_bounds__(POSEIDON_BLOCK) void permute_kernel(const u32 *__restrict__ prm, int hf, int partial,
                                                                 u32 *__restrict__ st, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp<C> s[T];
#pragma unroll
    for (int j = 0; j < T; ++j) s[j] = Fp<C>::load(st + (i * T + j) * 8);
    permute<C, T>(s, prm, hf, partial);
#pragma unroll
    for (int j = 0; j < T; ++j) s[j].store(st + (i * T + j) * 8);
}

template <class C, int T>
__global__ __launch_bounds__(POSEIDON_BLOCK) void hash_kernel(const u32 *__restrict__ prm, int hf, int partial,
                                                              const u32 *__restrict__ in, size_t n, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp<C> s[T];
    s[0] = tag_of<C>(prm, T, hf, partial);
#pragma unroll
    for (int j = 1; j < T; ++j) s[j] = Fp<C>::load(in + (i * (T - 1) + j - 1) * 8);
    permute<C, T>(s, prm, hf, partial);
    s[0].store(out + i * 8);
}

// the tree k whose segment of a level holds entry e: off[k] <= e < off[k + 1] (binary search over the n_trees + 1 offsets)
MG_DEV int tree_of(const u64 *__restrict__ off, int n_trees, u64 e) {
    int lo = 0, hi = n_trees; // off[lo] <= e < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- the trees: level passes, the finish in LDS, the gather -- all over the recomputed ranges (a build: the whole tree) -------
MG_DEV u64 nodes_end(u64 n, int l) { return (n + ((u64)1 << l) - 1) >> l; } // ceil(n / 2^l)
// does pass l -> l + 1 advance tree's ancestor chain: l < ctz(n_old); never for n_old = 0
MG_DEV bool chain_runs(u64 n_old, int l) { return n_old && !(n_old & (((u64)2 << l) - 1)); }
// node(l, s_l - 1) of tree k for odd s_l; `anc` is where the chain stands (t.anc, or the top kernel's copy in LDS)
template <class C> MG_DEV Fp<C> seed_of(const MerkleForest &t, int k, int l, u64 n_old, const u32 *anc) {
    return Fp<C>::load(n_old & (((u64)1 << l) - 1) ? t.cur + ((size_t)k * (t.height - 1) + l) * 8 : anc);
}

// level l -> l + 1 of every tree's recomputed range, one lane per parent: parent = hash(left child, right child or 0 past the
// level's end), a left child one below the segment start being the level's seed (n_old = 0: s_l = 0, the left child is always in
// the segment); after the parents one lane per tree hashes the next link of its chain
template <class C>
__global__ __launch_bounds__(POSEIDON_BLOCK) void merkle_level(const u32 *__restrict__ prm, int hf, int partial, MerkleForest t,
                                                               int l, size_t n_parents) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parents + t.n_trees) return;
    Fp<C> a, b;
    u32 *dst;
    if (i < n_parents) {
        const u64 *src_off = t.off + (size_t)l * (t.n_trees + 1), *dst_off = src_off + t.n_trees + 1;
        const u64 e = dst_off[0] + i;
        const int k = tree_of(dst_off, t.n_trees, e);
        const u64 n_old = t.n_old[k], s = n_old >> l, c = src_off[k + 1] - src_off[k];
        const u64 j = (n_old >> (l + 1)) + (e - dst_off[k]);
        const u64 r = 2 * j + 1 - s; // the right child's place in the segment; the left child is one before it, or the seed
        const u32 *ch = t.nodes + (src_off[k] + r) * 8;
        a = r ? Fp<C>::load(ch - 8) : seed_of<C>(t, k, l, n_old, t.anc + (size_t)k * 8);
        b = r < c ? Fp<C>::load(ch) : Fp<C>::zero();
        dst = t.nodes + e * 8;
    } else {
        const size_t k = i - n_parents;
        if (!chain_runs(t.n_old[k], l)) return;
        dst = t.anc + k * 8;
        a = Fp<C>::load(t.cur + (k * (t.height - 1) + l) * 8);
        b = Fp<C>::load(dst);
    }
    hash2<C>(a, b, prm, hf, partial).store(dst);
}

// the finish of each tree in LDS, one block per tree, from level `l0` (at most MERKLE_TOP recomputed nodes per tree) to the
// root, instead of up to 19 tiny launches: levels alternate between two LDS buffers, every level is also written to its segment
// (the gather reads it), and the chain is one more item of a level while it runs
constexpr int TOP_LDS_B = MERKLE_TOP, TOP_LDS_ANC = MERKLE_TOP + MERKLE_TOP / 2 + 8; // a level above l0 has <= TOP / 2 + 1
template <class C>
__global__ __launch_bounds__(POSEIDON_BLOCK) void merkle_top(const u32 *__restrict__ prm, int hf, int partial, MerkleForest t,
                                                             int l0, u32 *__restrict__ roots) {
    __shared__ u32 lds[(TOP_LDS_ANC + 1) * 8];
    const int k = blockIdx.x, tid = threadIdx.x;
    const size_t stride = (size_t)t.n_trees + 1;
    const u64 n_old = t.n_old[k], n_new = t.n_new[k];
    u32 *const anc = lds + TOP_LDS_ANC * 8;
    u32 src = 0, dst = TOP_LDS_B * 8; // word offsets of the level read and the level written
    const u64 base = t.off[l0 * stride + k];
    u32 c = (u32)(t.off[l0 * stride + k + 1] - base);
#pragma unroll 1
    for (u32 j = tid; j < c; j += POSEIDON_BLOCK) Fp<C>::load(t.nodes + (base + j) * 8).store(lds + j * 8);
    if (tid == 0) Fp<C>::load(t.anc + (size_t)k * 8).store(anc);
    __syncthreads();
#pragma unroll 1
    for (int l = l0; l < t.height - 1; ++l) {
        const u64 s = n_old >> l, sp = n_old >> (l + 1), up = t.off[(l + 1) * stride + k];
        const u32 cp = (u32)(nodes_end(n_new, l + 1) - sp), items = cp + (chain_runs(n_old, l) ? 1 : 0);
#pragma unroll 1
        for (u32 it = tid; it < items; it += POSEIDON_BLOCK) {
            Fp<C> a, b;
            if (it < cp) {
                const u64 j = sp + it;
                const u32 r = (u32)(2 * j + 1 - s); // the right child's place in the level; the left child is one before it
                const u32 *ch = lds + src + r * 8;
                a = r ? Fp<C>::load(ch - 8) : seed_of<C>(t, k, l, n_old, anc);
                b = r < c ? Fp<C>::load(ch) : Fp<C>::zero();
            } else {
                a = Fp<C>::load(t.cur + ((size_t)k * (t.height - 1) + l) * 8);
                b = Fp<C>::load(anc);
            }
            const Fp<C> hsh = hash2<C>(a, b, prm, hf, partial);
            if (it < cp) {
                hsh.store(lds + dst + it * 8);
                hsh.store(t.nodes + (up + it) * 8);
            } else
                hsh.store(anc); // read above by this lane only: a level reads the chain as its seed only once it has ended
        }
        __syncthreads();
        const u32 x = src;
        src = dst, dst = x, c = cp;
    }
    if (tid == 0) { // a full tree appends nothing and recomputes nothing: its root is the end of the chain
        (n_new == 0 ? Fp<C>::zero() : Fp<C>::load(c ? lds + src : anc)).store(roots + (size_t)k * 8);
        Fp<C>::load(anc).store(t.anc + (size_t)k * 8);
    }
}

// manta's Path of leaf idx: the sibling of its ancestor on levels 0 .. height - 2. One lane per (request, level): entry l in the
// new tree is 0 past the level's last node, a recomputed node from s_l on (n_old = 0: every node), the level's seed for a new
// leaf, and otherwise -- an older leaf's older sibling -- left as it is in `out`. Requests n_req .. n_req + n_trees - 1 are the
// trees' new current paths (the old one when nothing was appended); the last n_trees lanes write the new last leaves.
template <class C>
__global__ __launch_bounds__(POSEIDON_BLOCK) void merkle_gather(MerkleForest t, const u64 *__restrict__ req_trees,
                                                                const u64 *__restrict__ req_idx, size_t n_req,
                                                                u32 *__restrict__ out, u32 *__restrict__ new_last) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int len = t.height - 1;
    const size_t entries = (n_req + t.n_trees) * (size_t)len;
    if (g >= entries + t.n_trees) return;
    if (g >= entries) {
        const size_t k = g - entries;
        const u64 b = t.n_new[k] - t.n_old[k];
        Fp<C>::load(b ? t.nodes + (t.off[k] + b - 1) * 8 : t.last + k * 8).store(new_last + k * 8);
        return;
    }
    const size_t q = g / len;
    const int l = (int)(g % len);
    const int k = (int)(q < n_req ? req_trees[q] : q - n_req);
    const u64 n_old = t.n_old[k], n_new = t.n_new[k];
    u64 idx;
    if (q < n_req) idx = req_idx[q];
    else if (n_new == n_old) {
        Fp<C>::load(t.cur + ((size_t)k * len + l) * 8).store(out + g * 8);
        return;
    } else idx = n_new - 1;
    const u64 s = n_old >> l, sib = (idx >> l) ^ 1;
    if (sib >= nodes_end(n_new, l)) Fp<C>::zero().store(out + g * 8);
    else if (sib >= s) Fp<C>::load(t.nodes + (t.off[(size_t)l * (t.n_trees + 1) + k] + sib - s) * 8).store(out + g * 8);
    else if (idx >= n_old) seed_of<C>(t, k, l, n_old, t.anc + (size_t)k * 8).store(out + g * 8);
}

} // namespace pos

// ---- the launch functions --------------------------------------------------------------------------------------------------
// `kernel` over `lanes` lanes in blocks of POSEIDON_BLOCK; nothing is launched for none
template <class Kernel, class... Args> hipError_t poseidon_lanes(Kernel kernel, hipStream_t s, size_t lanes, Args... args) {
    if (lanes == 0) return hipSuccess;
    kernel<<<dim3((unsigned)((lanes + POSEIDON_BLOCK - 1) / POSEIDON_BLOCK)), dim3(POSEIDON_BLOCK), 0, s>>>(args...);
    return hipGetLastError();
}

template <class C> hipError_t PoseidonKernels<C>::permute(hipStream_t s, const PoseidonDev &h, u32 *states, size_t n) {
    switch (h.width) {
    case 3: return poseidon_lanes(pos::permute_kernel<C, 3>, s, n, h.prm, h.half_full, h.partial, states, n);
    case 4: return poseidon_lanes(pos::permute_kernel<C, 4>, s, n, h.prm, h.half_full, h.partial, states, n);
    case 5: return poseidon_lanes(pos::permute_kernel<C, 5>, s, n, h.prm, h.half_full, h.partial, states, n);
    case 6: return poseidon_lanes(pos::permute_kernel<C, 6>, s, n, h.prm, h.half_full, h.partial, states, n);
    default: return hipErrorInvalidValue;
    }
}

template <class C>
hipError_t PoseidonKernels<C>::hash(hipStream_t s, const PoseidonDev &h, const u32 *in, size_t n, u32 *digests) {
    switch (h.width) {
    case 3: return poseidon_lanes(pos::hash_kernel<C, 3>, s, n, h.prm, h.half_full, h.partial, in, n, digests);
    case 4: return poseidon_lanes(pos::hash_kernel<C, 4>, s, n, h.prm, h.half_full, h.partial, in, n, digests);
    case 5: return poseidon_lanes(pos::hash_kernel<C, 5>, s, n, h.prm, h.half_full, h.partial, in, n, digests);
    case 6: return poseidon_lanes(pos::hash_kernel<C, 6>, s, n, h.prm, h.half_full, h.partial, in, n, digests);
    default: return hipErrorInvalidValue;
    }
}

template <class C>
hipError_t PoseidonKernels<C>::merkle_level(hipStream_t s, const PoseidonDev &h, const MerkleForest &t, int l, size_t n_parents) {
    return poseidon_lanes(pos::merkle_level<C>, s, n_parents + t.n_trees, h.prm, h.half_full, h.partial, t, l, n_parents);
}

template <class C>
hipError_t PoseidonKernels<C>::merkle_top(hipStream_t s, const PoseidonDev &h, const MerkleForest &t, int l0, u32 *roots) {
    if (t.n_trees == 0) return hipSuccess;
    pos::merkle_top<C><<<dim3((unsigned)t.n_trees), dim3(POSEIDON_BLOCK), 0, s>>>(h.prm, h.half_full, h.partial, t, l0, roots);
    return hipGetLastError();
}

template <class C>
hipError_t PoseidonKernels<C>::merkle_gather(hipStream_t s, const MerkleForest &t, const u64 *req_trees, const u64 *req_idx,
                                             size_t n_req, u32 *paths, u32 *new_last) {
    const size_t lanes = (n_req + t.n_trees) * (size_t)(t.height - 1) + t.n_trees;
    return poseidon_lanes(pos::merkle_gather<C>, s, lanes, t, req_trees, req_idx, n_req, paths, new_last);
}

} // namespace mg
