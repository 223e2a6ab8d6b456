// Batched Poseidon over the BN254 / BLS12-381 scalar fields on gfx950, and the hashing inside manta's Merkle trees: the
// permutation and `Hasher::hash` with one state per lane (width t = 3..6 a template parameter, round counts and constants
// runtime data), one kernel per tree level over every tree of a forest, the top levels of each tree in LDS, and path gathering.
// Instantiated per scalar field in poseidon_<curve>.hip; the host layer and the C ABI (mg_poseidon_*, mg_merkle_*) are in
// poseidon.cpp.
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
// are entries off[l][k] .. off[l][k + 1] of that level's buffer.
#pragma once
#include "engine.h"
#include "fp_dev.h"
#include "params_gen.h"

namespace mg {

// keys | mds | tag in Montgomery words of 8 x u32 per element
struct PoseidonLaunch {
    enum Op { PERMUTE = 0, HASH = 1, LEVEL = 2, TOP = 3, PATHS = 4 };
    int op, width, half_full, partial;
    const u32 *prm;      // device parameters
    const u32 *in;       // PERMUTE: n states (in place, = out); HASH: n x (t - 1) inputs; LEVEL / TOP: the source level
    u32 *out;            // PERMUTE: states; HASH: n digests; LEVEL: the next level; PATHS: k x (height - 1) digests
    size_t n;            // states / digests / parents of the level / paths
    const u64 *src_off;  // LEVEL: offsets of the source level; TOP / PATHS: the whole table
    const u64 *dst_off;  // LEVEL: offsets of the destination level
    int n_trees, level, height;
    u32 *keep;           // TOP: where the levels above `level` are written (the table's absolute offsets), or null
    u32 *roots;          // TOP: n_trees roots
    const u64 *indices;  // PATHS: leaf indices
    hipStream_t stream;
};
hipError_t poseidon_launch_bn254(const PoseidonLaunch &a);
hipError_t poseidon_launch_bls381(const PoseidonLaunch &a);

constexpr int MERKLE_TOP = 1024; // a level of at most this many nodes per tree is finished in LDS by merkle_top_kernel
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

// one level of every tree: parent j of tree k = hash(child 2j, child 2j + 1 or 0 when absent); one lane per parent
template <class C>
__global__ __launch_bounds__(POSEIDON_BLOCK) void level_kernel(const u32 *__restrict__ prm, int hf, int partial,
                                                               const u32 *__restrict__ src, const u64 *__restrict__ src_off,
                                                               u32 *__restrict__ dst, const u64 *__restrict__ dst_off, int n_trees,
                                                               size_t n_parents) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parents) return;
    const u64 e = dst_off[0] + i;
    const int k = tree_of(dst_off, n_trees, e);
    const u64 j = e - dst_off[k], c = src_off[k + 1] - src_off[k];
    const u32 *ch = src + (src_off[k] + 2 * j) * 8;
    const Fp<C> l = Fp<C>::load(ch);
    const Fp<C> r = 2 * j + 1 < c ? Fp<C>::load(ch + 8) : Fp<C>::zero();
    hash2<C>(l, r, prm, hf, partial).store(dst + e * 8);
}

// the top of each tree, one block per tree: level `l0` (at most MERKLE_TOP nodes per tree) is loaded into LDS and reduced
// level by level to the root, two parents per lane; with `keep` every level above l0 is also written to its place in the table
template <class C>
__global__ __launch_bounds__(POSEIDON_BLOCK) void top_kernel(const u32 *__restrict__ prm, int hf, int partial,
                                                             const u32 *__restrict__ src, const u64 *__restrict__ off, int n_trees,
                                                             int l0, int height, u32 *__restrict__ keep, u32 *__restrict__ roots) {
    __shared__ u32 lds[MERKLE_TOP * 8];
    const int k = blockIdx.x, tid = threadIdx.x;
    const size_t stride = (size_t)n_trees + 1;
    const u64 base = off[l0 * stride + k];
    u32 c = (u32)(off[l0 * stride + k + 1] - base);
#pragma unroll 1
    for (u32 j = tid; j < c; j += POSEIDON_BLOCK) Fp<C>::load(src + (base + j) * 8).store(lds + j * 8);
    __syncthreads();
#pragma unroll 1
    for (int l = l0; l < height - 1; ++l) {
        const u32 cp = (c + 1) >> 1;
        Fp<C> h[MERKLE_TOP / 2 / POSEIDON_BLOCK];
#pragma unroll 1
        for (int q = 0; q < MERKLE_TOP / 2 / POSEIDON_BLOCK; ++q) {
            const u32 j = tid + q * POSEIDON_BLOCK;
            if (j < cp) {
                const Fp<C> a = Fp<C>::load(lds + 2 * j * 8);
                const Fp<C> b = 2 * j + 1 < c ? Fp<C>::load(lds + (2 * j + 1) * 8) : Fp<C>::zero();
                h[q] = hash2<C>(a, b, prm, hf, partial);
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MERKLE_TOP / 2 / POSEIDON_BLOCK; ++q) {
            const u32 j = tid + q * POSEIDON_BLOCK;
            if (j < cp) {
                h[q].store(lds + j * 8);
                if (keep) h[q].store(keep + (off[(l + 1) * stride + k] + j) * 8);
            }
        }
        __syncthreads();
        c = cp;
    }
    if (tid == 0) (c ? Fp<C>::load(lds) : Fp<C>::zero()).store(roots + (size_t)k * 8);
}

// manta's Path of leaf idx: sibling of its ancestor on levels 0 .. height - 2, 0 where absent; one lane per (path, level)
template <class C>
__global__ __launch_bounds__(POSEIDON_BLOCK) void paths_kernel(const u32 *__restrict__ levels, const u64 *__restrict__ off,
                                                               int height, const u64 *__restrict__ idx, size_t k,
                                                               u32 *__restrict__ out) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int len = height - 1;
    if (g >= k * (size_t)len) return;
    const size_t q = g / len;
    const int l = (int)(g % len);
    const u64 s = (idx[q] >> l) ^ 1, lo = off[2 * l], c = off[2 * l + 1] - lo;
    (s < c ? Fp<C>::load(levels + (lo + s) * 8) : Fp<C>::zero()).store(out + g * 8);
}

} // namespace pos

template <class C> hipError_t poseidon_launch(const PoseidonLaunch &a) {
    const auto grid = [](size_t n) { return dim3((unsigned)((n + POSEIDON_BLOCK - 1) / POSEIDON_BLOCK)); };
    const dim3 blk(POSEIDON_BLOCK);
    switch (a.op) {
    case PoseidonLaunch::PERMUTE:
    case PoseidonLaunch::HASH: {
        if (a.n == 0) return hipSuccess;
#define MG_POSEIDON_WIDTH(T)                                                                                                     \
    case T:                                                                                                                      \
        if (a.op == PoseidonLaunch::PERMUTE)                                                                                     \
            hipLaunchKernelGGL((pos::permute_kernel<C, T>), grid(a.n), blk, 0, a.stream, a.prm, a.half_full, a.partial, a.out,   \
                               a.n);                                                                                             \
        else                                                                                                                     \
            hipLaunchKernelGGL((pos::hash_kernel<C, T>), grid(a.n), blk, 0, a.stream, a.prm, a.half_full, a.partial, a.in, a.n,  \
                               a.out);                                                                                           \
        break;
        switch (a.width) {
            MG_POSEIDON_WIDTH(3)
            MG_POSEIDON_WIDTH(4)
            MG_POSEIDON_WIDTH(5)
            MG_POSEIDON_WIDTH(6)
        default: return hipErrorInvalidValue;
        }
#undef MG_POSEIDON_WIDTH
        break;
    }
    case PoseidonLaunch::LEVEL:
        if (a.n == 0) return hipSuccess;
        hipLaunchKernelGGL((pos::level_kernel<C>), grid(a.n), blk, 0, a.stream, a.prm, a.half_full, a.partial, a.in, a.src_off,
                           a.out, a.dst_off, a.n_trees, a.n);
        break;
    case PoseidonLaunch::TOP:
        if (a.n_trees == 0) return hipSuccess;
        hipLaunchKernelGGL((pos::top_kernel<C>), dim3((unsigned)a.n_trees), blk, 0, a.stream, a.prm, a.half_full, a.partial, a.in,
                           a.src_off, a.n_trees, a.level, a.height, a.keep, a.roots);
        break;
    case PoseidonLaunch::PATHS:
        if (a.n == 0) return hipSuccess;
        hipLaunchKernelGGL((pos::paths_kernel<C>), grid(a.n * (size_t)(a.height - 1)), blk, 0, a.stream, a.in, a.src_off,
                           a.height, a.indices, a.n, a.out);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace mg
