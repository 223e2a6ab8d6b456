// Column sums of scaled group elements -- the sparse half of `mpc::initialize` (manta-trusted-setup/src/groth16/mpc.rs:251-294
// `specialize_to_phase_2`): out[j] = sum over the stored entries (i, j) of a set of sparse matrices of [M[i][j]] basis[i].
// The reference runs one 254-bit `mul` per non-zero in sequence; here it is a sparse matrix-transpose product over the group,
// built from the MSM's own pieces. Part of msm_impl.h; host side: GroupEngineT::qap_columns (msm_engine.h).
//
//   host        one (key = column, value = entry id) pair per stored entry; per entry the basis row it multiplies (`src`, an
//               index into ONE device array holding every basis of the call) and its Montgomery coefficient
//   sort        sort_pairs by column (sort.hip; stable, so the entries of a column keep the caller's order)
//   qap_entry   one lane per SORTED entry: [k] P as an XYZZ point, written at the entry's sorted position
//   qap_segsum  every lane owns L consecutive sorted products and adds them by column with XYZZ::add (projective addends;
//               P + P and P + (-P) exact): runs that start and end inside the lane go straight to out[col], the lane's first
//               and last run leave as partials -- the layout accumulate_chunks leaves
//   merge       merge_partials (msm_reduce.h) folds the partials of one column, 64 G -> 2 per wave and level
//   normalise   XYZZ -> arkworks-format XYZZ (group_scale_store_kernel, group_ops.h) -> affine with one inversion per 16 points
//               (xyzz_to_affine_launch, msm_tables.h)
//
// Launches per call: 1 zero-fill + 4 per radix pass (at most 4 passes) + 2 + the merge levels (log_64 of the lane count) + 2;
// copies: 4 uploads (basis rows, coefficients, columns, entry ids), 1 download -- and in front of it mg_qap_columns uploads the
// basis of each of its terms, mg_mpc_initialize its four power vectors. Neither depends on the number of columns; no
// global atomics on points; every column is written exactly once, so the result is deterministic.
//
// Device memory of a call with N entries, C columns and L entries per lane, T = ceil(N / L) (XW = words of an XYZZ point in the
// kernels' field representation, XS / AS = words of an arkworks-format XYZZ / affine point), besides the bases themselves:
//   4 N (src) + 32 N (coefficients) + 16 N (pairs in and out) + sort_pairs_temp_bytes(N) ~ 8.3 N + 4 XW N (products)
//   + 2 T (4 + 4 XW) (1 + 1/32) (partials of two merge levels) + 4 XW (C + 1) (column sums) + 4 (XS + AS) C (normalisation)
// BN254 G1 (XW = 36): ~245 B per entry + 340 B per column at L = 8; BLS12-381 G2 (XW = 112): ~625 B per entry + 1 KB per column.
#pragma once
#include "msm_common.h"

namespace mg {

// [k] P for one sorted entry. R1CS coefficients are mostly 1, -1 and small powers of two: 0, 1 and r - 1 take no ladder at all,
// everything else is a double-and-add from the top set bit of the shorter of k and r - k (the point negated for r - k), so a
// coefficient 2^s costs s doublings and -3 two doublings and an addition where the plain ladder walks 254 bits.
template <class F, class FrC>
__global__ __launch_bounds__(256) void qap_entry_kernel(const u32 *__restrict__ sorted_ids, u32 N, const u32 *__restrict__ src,
                                                        const u32 *__restrict__ val_mont, const u32 *__restrict__ bases_aff,
                                                        u32 *__restrict__ prods) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    typedef typename F::Std S;
    typedef Fp<FrC> K;
    const u32 e = sorted_ids[t];
    const Affine<S> s = Affine<S>::load(bases_aff + (size_t)src[e] * Affine<S>::WORDS);
    K k = K::from_mont(K::load(val_mont + (size_t)e * 8)); // `coeff.into_repr()`
    XYZZ<F> acc = XYZZ<F>::inf();
    if (!s.is_inf() && !k.is_zero()) {
        const Affine<F> p{F::from_std(s.x), F::from_std(s.y)};
        const K nk = K::neg(k); // r - k
        // the shorter of the two: compare from the top limb down
        bool negate = false, decided = false;
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            if (!decided && k.v[i] != nk.v[i]) negate = nk.v[i] < k.v[i], decided = true;
        }
        if (negate) k = nk;
        int top = 0; // index of the top set bit (k != 0)
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (k.v[i]) top = 32 * i + 31 - __clz((int)k.v[i]);
        acc.madd(p, negate); // the top bit: acc = +-P
        for (int b = top - 1; b >= 0; --b) {
            u32 w = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) w = (q == (b >> 5)) ? k.v[q] : w;
            acc = XYZZ<F>::dbl(acc);
            if ((w >> (b & 31)) & 1) acc.madd(p, negate);
        }
    }
    acc.store(prods + (size_t)t * XYZZ<F>::WORDS);
}

// Segmented sum of the sorted products by column, L entries per lane: accumulate_chunks (msm_accumulate.h) over projective
// addends. A run that starts and ends inside the lane is complete -- no other lane holds a part of it -- and is stored to
// out[col]; the first and the last run may continue in the neighbouring lanes and leave as the partials (2 t, 2 t + 1) for
// merge_partials; a lane that is one run emits (col, sum), (col, infinity). `invalid` (= the number of columns) marks the slots
// of lanes past the last entry.
template <class F>
__global__ __launch_bounds__(256) void qap_segsum_kernel(const u32 *__restrict__ keys, const u32 *__restrict__ prods, u32 N, u32 L,
                                                         u32 invalid, u32 *__restrict__ out, u32 *__restrict__ pkeys,
                                                         u32 *__restrict__ ppts, u32 T) {
    MG_PRIO_FOR(F);
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    constexpr size_t XW = XYZZ<F>::WORDS;
    const size_t begin = (size_t)t * L;
    size_t end = begin + L;
    if (end > N) end = N;
    if (begin >= N) {
        pkeys[2 * t] = invalid;
        pkeys[2 * t + 1] = invalid;
        return;
    }
    u32 cur = keys[begin];
    XYZZ<F> acc = XYZZ<F>::inf();
    bool first = true;
    for (size_t j = begin; j < end; ++j) {
        const u32 k = keys[j];
        if (k != cur) {
            if (first) {
                pkeys[2 * t] = cur;
                acc.store(ppts + (size_t)(2 * t) * XW);
                first = false;
            } else {
                acc.store(out + (size_t)cur * XW);
            }
            acc = XYZZ<F>::inf();
            cur = k;
        }
        const XYZZ<F> p = XYZZ<F>::load(prods + j * XW);
        if (!p.is_inf()) acc.add(p);
    }
    if (first) { // the whole lane is one run
        pkeys[2 * t] = cur;
        acc.store(ppts + (size_t)(2 * t) * XW);
        pkeys[2 * t + 1] = cur;
        XYZZ<F>::inf().store(ppts + (size_t)(2 * t + 1) * XW);
    } else {
        pkeys[2 * t + 1] = cur;
        acc.store(ppts + (size_t)(2 * t + 1) * XW);
    }
}

} // namespace mg
