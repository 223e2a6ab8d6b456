// Kernels that build base tables: base conversion, window / full tables, and the batched affine conversion that every producer of
// XYZZ points ends with (xyzz_to_affine_batch and its one launch site). Part of msm_impl.h.
#pragma once
#include "msm_common.h"

namespace mg {

// an affine point in arkworks format (zeros = infinity) -> the internal field representation
template <class F> static __device__ __forceinline__ Affine<F> load_affine_std(const u32 *p) {
    typedef typename F::Std S;
    const Affine<S> s = Affine<S>::load(p);
    Affine<F> r;
    if (s.is_inf()) {
        r.x = F::zero();
        r.y = F::zero();
    } else {
        r.x = F::from_std(s.x);
        r.y = F::from_std(s.y);
    }
    return r;
}

// arkworks-format affine bases -> internal representation (identity copy when the two coincide)
template <class F>
__global__ __launch_bounds__(256) void bases_to_internal(const u32 *__restrict__ in, size_t n, u32 *__restrict__ out,
                                                         u32 astride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    load_affine_std<F>(in + i * Affine<typename F::Std>::WORDS).store(out + i * astride);
}

// --------------------------------------------------------------------------------------------
// precompute: table[w*n + i] = 2^(c w) * P_i (affine). Two kernels: doubling chains into XYZZ, then
// batched conversion to affine with Montgomery's trick (one Fermat inversion per KB points).
// --------------------------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(256) void precompute_chain(const u32 *__restrict__ base, u32 astride, u32 n, int c, int W,
                                                        u32 *__restrict__ xyzz_out /* (W-1)*n */) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XYZZ<F> p = XYZZ<F>::from_affine(Affine<F>::load(base + (size_t)i * astride));
    for (int w = 1; w < W; ++w) {
        for (int k = 0; k < c; ++k) p = XYZZ<F>::dbl(p);
        p.store(xyzz_out + ((size_t)(w - 1) * n + i) * XYZZ<F>::WORDS);
    }
}
// full tables: the multiples m Q, m = 1 .. B, of `cnt` window bases Q = 2^(c w) P (affine, from entry j0 on) as XYZZ points,
// entry (t B + m - 1) -- B - 1 mixed additions per lane (the first is the doubling Q + Q: madd's exact exceptional cases)
template <class F>
__global__ __launch_bounds__(256) void full_table_chain(const u32 *__restrict__ win, u32 astride, size_t j0, u32 cnt, u32 B,
                                                        u32 *__restrict__ xyzz_out) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt) return;
    const Affine<F> q = Affine<F>::load(win + (j0 + t) * astride);
    XYZZ<F> acc = XYZZ<F>::from_affine(q);
    for (u32 m = 0; m < B; ++m) {
        if (m) acc.madd(q, false);
        acc.store(xyzz_out + ((size_t)t * B + m) * XYZZ<F>::WORDS);
    }
}
template <class F> struct FieldInv; // Fermat inversion on the device (slow, one-off use only)
template <class C> struct FieldInv<Fp<C>> {
    static __device__ Fp<C> inv(const Fp<C> &a) { return Fp<C>::inv(a); }
};
template <class C> struct FieldInv<FpR<C>> {
    static __device__ FpR<C> inv(const FpR<C> &a) { return FpR<C>::inv(a); }
};
template <class C> struct FieldInv<Fp2R<C>> {
    static __device__ Fp2R<C> inv(const Fp2R<C> &a) { return Fp2R<C>::inv(a); }
};
template <class C> struct FieldInv<Fp2<C>> {
    static __device__ Fp2<C> inv(const Fp2<C> &a) {
        typedef Fp<C> B;
        B n = B::inv(B::add(B::sqr(a.c0), B::sqr(a.c1)));
        return Fp2<C>{B::mul(a.c0, n), B::neg(B::mul(a.c1, n))};
    }
};
template <class F, int KB>
__global__ __launch_bounds__(256) void xyzz_to_affine_batch(const u32 *__restrict__ xyzz, size_t n,
                                                            u32 *__restrict__ aff, u32 astride) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t b0 = t * KB;
    if (b0 >= n) return;
    // prefix products of d_k = zz*zzz (1 for infinity) are parked at the front of the affine output record (F::N limb words: a
    // record is 2 F::AFF_N >= F::N words in either format), then replaced by the record itself
    static_assert(Affine<F>::WORDS >= F::N, "record too small to park a field element");
    F run = F::one();
    for (int k = 0; k < KB && b0 + k < n; ++k) {
        const u32 *src = xyzz + (b0 + k) * XYZZ<F>::WORDS;
        F zz = F::load(src + 2 * F::N), zzz = F::load(src + 3 * F::N);
        F d = zz.is_zero_exact() ? F::one() : F::mul(zz, zzz);
        run.store(aff + (b0 + k) * astride); // prefix before k
        run = F::mul(run, d);
    }
    F inv = FieldInv<F>::inv(run);
    int last = KB - 1;
    if (b0 + KB > n) last = (int)(n - b0) - 1;
    for (int k = last; k >= 0; --k) {
        const u32 *src = xyzz + (b0 + k) * XYZZ<F>::WORDS;
        u32 *dst = aff + (b0 + k) * astride;
        F zz = F::load(src + 2 * F::N), zzz = F::load(src + 3 * F::N);
        if (zz.is_zero_exact()) {
            Affine<F>{F::zero(), F::zero()}.store(dst);
            continue;
        }
        F pre = F::load(dst);
        F dinv = F::mul(inv, pre); // 1/(zz*zzz)
        inv = F::mul(inv, F::mul(zz, zzz));
        F x = F::load(src), y = F::load(src + F::N);
        F izz = F::mul(dinv, zzz), izzz = F::mul(dinv, zz);
        Affine<F>{F::mul(x, izz), F::mul(y, izzz)}.store(dst); // products: < 2p, normalised -- what the packed format needs
    }
}
// n XYZZ points at src -> affine records `stride` words apart at dst, KB points per lane and inversion (64 for full tables)
template <class F, int KB = 16> static void xyzz_to_affine_launch(hipStream_t st, const u32 *src, size_t n, u32 *dst, u32 stride) {
    hipLaunchKernelGGL((xyzz_to_affine_batch<F, KB>), dim3(cdiv(cdiv(n, KB), 256)), dim3(256), 0, st, src, n, dst, stride);
}

} // namespace mg
