// Batched arkworks 0.3 point codec on gfx950: decode (bytes -> checked affine Montgomery points), check (points already in
// memory) and encode (affine Montgomery -> canonical bytes) for short-Weierstrass G1 / G2 of BN254 and BLS12-381, one point
// per lane. Instantiated per curve in point_codec_<curve>.hip; the C ABI (mg_points_*) is in point_codec.cpp.
// The same kernel bodies read and write a second record format, that of the Perpetual Powers of Tau files (BN254 only, C ABI
// mg_ppot_points_*): the bodies take a format policy (`Arkworks`, `Ppot` below) that turns a record into x, y and flags, and back.
//
// Replaces, in bulk, the per-point host code of
//   ark-ec 0.3 `GroupAffine<P>: CanonicalDeserialize` (compressed: x + SWFlags, y = sqrt(x^3 + b) picked by the flag;
//   uncompressed: x, y + SWFlags) followed by `is_in_correct_subgroup_assuming_on_curve` -- what `Proof::deserialize`
//   (verify.cpp g1_decompress / g2_decompress), `kzg::Accumulator`'s CanonicalDeserialize (C::check on every power,
//   manta-trusted-setup/src/groth16/kzg.rs:607-690) and `mpc::State::check` (groth16/mpc.rs:79-100) run per point --
//   and `CanonicalSerialize` of the same points (host_ec.h HPoint::serialize).
//
// Arithmetic: the saturated, always fully reduced Fp<Fq> / Fp2<Fq> of fp_dev.h with the XYZZ group law of ec_dev.h. Every
// value is canonical, so the equality tests (r^2 == a, y^2 == x^3 + b), the sign test and the final [r]P == O test compare
// exact representations; the subgroup check is a security test and keeps to the plainest arithmetic the library has.
//
// Control flow: the square-root exponent (q + 1) / 4 and the group order r are compile-time constants, so every lane of a
// wavefront runs the same squarings, multiplications, doublings and additions. A lane whose encoding failed keeps computing
// on whatever its bytes gave and is masked when its status is written; lanes differ only in selects (and in the exact
// exceptional branches of the group law, taken by points of small order only).
#pragma once
#include "ec_dev.h"
#include "params_gen.h"
#include "staging.h"
#include <cstring>
#include <vector>

namespace mg {

enum { PT_OK = 0, PT_BAD_ENCODING = 1, PT_NOT_ON_CURVE = 2, PT_NOT_IN_SUBGROUP = 3 }; // = MG_POINT_* of mantagpu.h

namespace codec {

// ---- base field Fq (canonical Montgomery Fp<C>) ---------------------------------------------------------------------
template <class C> MG_DEV bool geq_p(const Fp<C> &a) { // the plain integer a >= p
    u32 bw = 0;
#pragma unroll
    for (int i = 0; i < C::N; ++i) {
        const u64 d = (u64)a.v[i] - C::P[i] - bw;
        bw = (u32)(d >> 63);
    }
    return bw == 0;
}
// a^((q + 1) / 4): the square root of a when there is one (q = 3 mod 4 on both curves); fixed exponent, square-and-multiply
template <class C> MG_DEV Fp<C> pow_sqrt_exp(const Fp<C> &a) {
    static_assert((C::P[0] & 3) == 3, "q = 3 mod 4");
    constexpr int N = C::N;
    u32 t[N], e[N];
    u32 cy = 1;
#pragma unroll
    for (int i = 0; i < N; ++i) { // q + 1 (no carry out of the top limb: q < 2^(32 N - 2))
        const u64 s = (u64)C::P[i] + cy;
        t[i] = (u32)s;
        cy = (u32)(s >> 32);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = (t[i] >> 2) | (i + 1 < N ? t[i + 1] << 30 : 0u);
    Fp<C> acc = Fp<C>::one();
    for (int i = 32 * N - 1; i >= 0; --i) {
        acc = Fp<C>::sqr(acc);
        u32 w = 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j == (i >> 5)) w = e[j];
        if ((w >> (i & 31)) & 1) acc = Fp<C>::mul(acc, a);
    }
    return acc;
}
template <class C> MG_DEV Fp<C> half(const Fp<C> &a) { // a / 2 (mod p), linear: valid on Montgomery forms
    const u32 m = 0u - (a.v[0] & 1u);
    u32 t[C::N];
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < C::N; ++i) {
        const u64 s = (u64)a.v[i] + (C::P[i] & m) + c;
        t[i] = (u32)s;
        c = (u32)(s >> 32);
    }
    Fp<C> r;
#pragma unroll
    for (int i = 0; i < C::N; ++i) r.v[i] = (t[i] >> 1) | ((i + 1 < C::N ? t[i + 1] : c) << 31);
    return r;
}
template <class C> MG_DEV bool fsqrt(const Fp<C> &a, Fp<C> &r) {
    r = pow_sqrt_exp<C>(a);
    return Fp<C>::sqr(r) == a;
}
// arkworks "lexicographically largest": canonical(a) > (q - 1) / 2  <=>  2 canonical(a) > q  (host_ec.h HFp::is_high)
template <class C> MG_DEV bool is_high(const Fp<C> &a) {
    const Fp<C> c = Fp<C>::from_mont(a);
    u32 bw = 0, top = 0;
#pragma unroll
    for (int i = 0; i < C::N; ++i) {
        const u32 d = (c.v[i] << 1) | top;
        top = c.v[i] >> 31;
        const u64 s = (u64)d - C::P[i] - bw;
        bw = (u32)(s >> 63);
    }
    return top != 0 || bw == 0;
}
template <class C> MG_DEV void clear_flags(Fp<C> &a) { a.v[C::N - 1] &= 0x3fffffffu; }
template <class C> MG_DEV void set_flags(Fp<C> &a, u32 f) { a.v[C::N - 1] |= f << 24; }
template <class C> MG_DEV Fp<C> to_mont(const Fp<C> &a) { return Fp<C>::to_mont(a); }
template <class C> MG_DEV Fp<C> from_mont(const Fp<C> &a) { return Fp<C>::from_mont(a); }
template <class C> MG_DEV bool any_geq_p(const Fp<C> &a) { return geq_p<C>(a); }

// ---- Fq2 = Fq[u] / (u^2 + 1) ----------------------------------------------------------------------------------------
// Square root with uniform control flow (three fixed exponentiations; no branch on the data):
//   n = a0^2 + a1^2 is a square in Fq iff a is a square in Fq2 (the existence answer of verify.cpp hsqrt2);
//   s = sqrt(n);  t = (a0 + s) / 2  (t = a0 when a1 = 0);  x0 = t^((q+1)/4).
//   If x0^2 = t:   root = x0 + (a1 / 2x0) u.
//   Otherwise x0^2 = -t (t is a non-square; -1 is one too), and (a0 - s) / 2 = -a1^2 / 4t = (a1 / 2x0)^2, so
//                  root = (a1 / 2x0) + x0 u.   (a1 = 0: root = x0 u with x0^2 = -a0.)
// a1 != 0 makes t != 0 (t (a0 - s) / 2 = -a1^2 / 4), so 1 / 2x0 exists wherever it is used; the result is checked by
// squaring, which decides existence.
template <class C> MG_DEV bool fsqrt(const Fp2<C> &a, Fp2<C> &r) {
    typedef Fp<C> B;
    const B n = B::add(B::sqr(a.c0), B::sqr(a.c1));
    const B s = pow_sqrt_exp<C>(n);
    const B t = B::select(a.c1.is_zero(), a.c0, half<C>(B::add(a.c0, s)));
    const B x0 = pow_sqrt_exp<C>(t);
    const bool sq = B::sqr(x0) == t;
    const B y = B::mul(a.c1, B::inv(B::dbl(x0))); // inv(0) = 0: a1 = 0 gives y = 0
    r = Fp2<C>{B::select(sq, x0, y), B::select(sq, y, x0)};
    return Fp2<C>::sqr(r) == a;
}
template <class C> MG_DEV bool is_high(const Fp2<C> &a) { // c1 first, then c0 (host_ec.h HFp2::is_high)
    const bool h0 = is_high<C>(a.c0), h1 = is_high<C>(a.c1);
    return a.c1.is_zero() ? h0 : h1;
}
template <class C> MG_DEV void clear_flags(Fp2<C> &a) { clear_flags<C>(a.c1); }
template <class C> MG_DEV void set_flags(Fp2<C> &a, u32 f) { set_flags<C>(a.c1, f); }
template <class C> MG_DEV Fp2<C> to_mont(const Fp2<C> &a) { return Fp2<C>{Fp<C>::to_mont(a.c0), Fp<C>::to_mont(a.c1)}; }
template <class C> MG_DEV Fp2<C> from_mont(const Fp2<C> &a) { return Fp2<C>{Fp<C>::from_mont(a.c0), Fp<C>::from_mont(a.c1)}; }
template <class C> MG_DEV bool any_geq_p(const Fp2<C> &a) { return geq_p<C>(a.c0) || geq_p<C>(a.c1); }

// ---- the group: coordinate field and b of y^2 = x^3 + b -------------------------------------------------------------
template <class Curve, int G> struct Group;
template <class Curve> struct Group<Curve, 1> {
    typedef Fp<typename Curve::Fq> F;
    static MG_DEV F b() {
        F r;
#pragma unroll
        for (int i = 0; i < F::N; ++i) r.v[i] = Curve::G1_B[i];
        return r;
    }
};
template <class Curve> struct Group<Curve, 2> {
    typedef Fp2<typename Curve::Fq> F;
    static MG_DEV F b() {
        F r;
#pragma unroll
        for (int i = 0; i < Curve::Fq::N; ++i) r.c0.v[i] = Curve::G2_B0[i], r.c1.v[i] = Curve::G2_B1[i];
        return r;
    }
};

template <class F> MG_DEV F curve_rhs(const F &x, const F &b) { return F::add(F::mul(F::sqr(x), x), b); } // x^3 + b

constexpr int top_bit(const uint32_t *w, int n) {
    for (int i = 32 * n - 1; i >= 0; --i)
        if ((w[i >> 5] >> (i & 31)) & 1) return i;
    return -1;
}
// [r] p == O, r = the prime order of G1 / G2 (arkworks `is_in_correct_subgroup_assuming_on_curve`: mul_by_cofactor-free
// `self.mul(Fr::characteristic()).is_zero()`): double-and-add over r's fixed bits, from its top bit down
template <class Curve, class F> MG_DEV bool times_r_is_zero(const Affine<F> &p) {
    typedef typename Curve::Fr R;
    constexpr int TOP = top_bit(R::P, R::N);
    XYZZ<F> acc = XYZZ<F>::from_affine(p);
    for (int i = TOP - 1; i >= 0; --i) {
        acc = XYZZ<F>::dbl(acc);
        u32 w = 0;
#pragma unroll
        for (int j = 0; j < R::N; ++j)
            if (j == (i >> 5)) w = R::P[j];
        if ((w >> (i & 31)) & 1) acc.madd(p, false);
    }
    return acc.is_inf();
}

// ---- record formats ---------------------------------------------------------------------------------------------------
// A format reads a record of W words (W = F::N compressed, 2 F::N uncompressed; word k = bytes 4k..4k+3 of the record) into
// x, y as plain integers (not yet Montgomery; y = 0 when compressed), flags (bit 7 = 0x80, bit 6 = 0x40: infinity) and its verdict
// on the encoding (true = rejected), and writes canonical x, y with the flags back. Everything after that -- the curve equation,
// the root and its sign, the subgroup test, the order of the statuses -- is the kernels' and the same for every format.
template <class C> MG_DEV u32 top_flags(const Fp<C> &a) { return (a.v[C::N - 1] >> 24) & 0xc0u; }
template <class C> MG_DEV u32 top_flags(const Fp2<C> &a) { return top_flags<C>(a.c1); }

// arkworks 0.3 `CanonicalSerialize`: little-endian, Fq2 as c0 | c1, the flags in the last byte of the record
struct Arkworks {
    template <class Q, class F> static MG_DEV bool read(const u32 *rec, bool compressed, F &x, F &y, u32 &flags) {
        x = F::load(rec), y = F::zero();
        if (compressed) {
            flags = top_flags<Q>(x);
            clear_flags<Q>(x);
        } else {
            y = F::load(rec + F::N);
            flags = top_flags<Q>(y);
            clear_flags<Q>(y);
        }
        // SWFlags::from_u8 has no value for both bits; every coordinate read must be canonical, infinity included
        return flags == 0xc0u || any_geq_p<Q>(x) || any_geq_p<Q>(y);
    }
    template <class Q, class F> static MG_DEV void write(u32 *o, bool compressed, F x, F y, u32 flags) {
        if (compressed) {
            set_flags<Q>(x, flags);
            x.store(o);
        } else {
            set_flags<Q>(y, flags);
            x.store(o);
            y.store(o + F::N);
        }
    }
};

// Big-endian base-field elements: limb j of the element at words p[0 .. N) is the byte-swapped word N - 1 - j
template <class C> MG_DEV void load_be(const u32 *p, Fp<C> &a) {
#pragma unroll
    for (int j = 0; j < C::N; ++j) a.v[j] = __builtin_bswap32(p[C::N - 1 - j]);
}
template <class C> MG_DEV void load_be(const u32 *p, Fp2<C> &a) { // c1 first
    load_be<C>(p, a.c1);
    load_be<C>(p + C::N, a.c0);
}
template <class C> MG_DEV void store_be(u32 *p, const Fp<C> &a) {
#pragma unroll
    for (int j = 0; j < C::N; ++j) p[C::N - 1 - j] = __builtin_bswap32(a.v[j]);
}
template <class C> MG_DEV void store_be(u32 *p, const Fp2<C> &a) {
    store_be<C>(p, a.c1);
    store_be<C>(p + C::N, a.c0);
}
// The serializer of the Perpetual Powers of Tau files (manta-trusted-setup/src/groth16/ppot/serialization.rs:52-379):
// big-endian elements x | y (Fq2 as c1 | c0), the flags in bits 7 and 6 of byte 0 -- the top byte of the first element, which
// is x's (x.c1's) whatever the form. Bit 7 on an uncompressed record is `ExpectedUncompressed`; bit 6 with any other bit of the
// record set (byte 0 masked with 0x3f) is `PointAtInfinity`; bit 7 beside bit 6 on a compressed record is ignored (:116-126).
// Coordinates are `from_be_bytes_mod_order`: never rejected. x and y leave here UNREDUCED (the first element < 2^254, the
// others any 256-bit value) and the kernel's to_mont reduces them: Fp::mul(a, R2) computes t = (a R2 + m q) / R with a < R = 2^256,
// R2 < q and m < R, so t < (R q + R q) / R = 2q < 2^255 and its final conditional subtraction leaves a R mod q < q for EVERY
// 256-bit a; each column of the product holds at most 2 N terms < 2^64 in 96 bits whatever a is. No subtraction chain is needed.
struct Ppot {
    template <class Q, class F> static MG_DEV bool read(const u32 *rec, bool compressed, F &x, F &y, u32 &flags) {
        load_be<Q>(rec, x);
        y = F::zero();
        if (!compressed) load_be<Q>(rec + F::N, y);
        flags = top_flags<Q>(x);
        clear_flags<Q>(x);
        const bool inf_dirty = (flags & 0x40u) != 0 && !(x.is_zero() && y.is_zero());
        return (!compressed && (flags & 0x80u) != 0) || inf_dirty;
    }
    template <class Q, class F> static MG_DEV void write(u32 *o, bool compressed, F x, F y, u32 flags) {
        set_flags<Q>(x, flags);
        store_be<Q>(o, x);
        if (!compressed) store_be<Q>(o + F::N, y);
    }
};

// ---- kernels ----------------------------------------------------------------------------------------------------------
// n records of W words each in format Fmt -> affine Montgomery x || y (zeros for infinity and for every rejected point) and
// one status byte per point.
template <class Curve, int G, class Fmt>
__global__ __launch_bounds__(256) void point_decode_kernel(const u32 *__restrict__ in, size_t n, int compressed, int checked,
                                                           u32 *__restrict__ out, uint8_t *__restrict__ status) {
    typedef typename Group<Curve, G>::F F;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 *rec = in + i * (size_t)(compressed ? F::N : 2 * F::N);
    F x, y;
    u32 flags;
    const bool bad = Fmt::template read<typename Curve::Fq, F>(rec, compressed != 0, x, y, flags);
    const bool inf = (flags & 0x40u) != 0;
    x = to_mont<typename Curve::Fq>(x);
    const F rhs = curve_rhs(x, Group<Curve, G>::b());
    bool on = true;
    if (compressed) {
        F r;
        on = fsqrt<typename Curve::Fq>(rhs, r);
        const bool greatest = (flags & 0x80u) != 0;
        y = F::select(is_high<typename Curve::Fq>(r) != greatest, F::neg(r), r);
    } else {
        y = to_mont<typename Curve::Fq>(y);
        if (checked) on = F::sqr(y) == rhs;
    }
    bool in_group = true;
    if (checked) in_group = times_r_is_zero<Curve, F>(Affine<F>{x, y});
    const uint8_t st = bad ? PT_BAD_ENCODING : inf ? PT_OK : !on ? PT_NOT_ON_CURVE : !in_group ? PT_NOT_IN_SUBGROUP : PT_OK;
    const bool keep = st == PT_OK && !inf;
    const F z = F::zero();
    u32 *o = out + i * (size_t)(2 * F::N);
    F::select(keep, x, z).store(o);
    F::select(keep, y, z).store(o + F::N);
    status[i] = st;
}

// points already in memory (affine Montgomery, zeros = infinity): coordinates must be reduced (< q), on the curve and in
// the subgroup of order r -- `State::check` / `C::check`
template <class Curve, int G>
__global__ __launch_bounds__(256) void point_check_kernel(const u32 *__restrict__ aff, size_t n, uint8_t *__restrict__ status) {
    typedef typename Group<Curve, G>::F F;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> p = Affine<F>::load(aff + i * (size_t)(2 * F::N));
    const bool inf = p.x.is_zero() && p.y.is_zero();
    const bool bad = any_geq_p<typename Curve::Fq>(p.x) || any_geq_p<typename Curve::Fq>(p.y);
    const bool on = F::sqr(p.y) == curve_rhs(p.x, Group<Curve, G>::b());
    const bool in_group = times_r_is_zero<Curve, F>(p);
    status[i] = bad ? PT_BAD_ENCODING : inf ? PT_OK : !on ? PT_NOT_ON_CURVE : !in_group ? PT_NOT_IN_SUBGROUP : PT_OK;
}

// affine Montgomery -> records of format Fmt: canonical x (flags: bit 7 = y is the larger root) or x, y; infinity = zeros
// with bit 6 -- for Arkworks byte for byte HPoint::serialize
template <class Curve, int G, class Fmt>
__global__ __launch_bounds__(256) void point_encode_kernel(const u32 *__restrict__ aff, size_t n, int compressed,
                                                           u32 *__restrict__ out) {
    typedef typename Group<Curve, G>::F F;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> p = Affine<F>::load(aff + i * (size_t)(2 * F::N));
    const bool inf = p.x.is_zero() && p.y.is_zero();
    const F z = F::zero();
    const F x = F::select(inf, z, from_mont<typename Curve::Fq>(p.x));
    u32 *o = out + i * (size_t)(compressed ? F::N : 2 * F::N);
    if (compressed) {
        Fmt::template write<typename Curve::Fq, F>(o, true, x, z, inf ? 0x40u : is_high<typename Curve::Fq>(p.y) ? 0x80u : 0u);
    } else {
        const F y = F::select(inf, z, from_mont<typename Curve::Fq>(p.y));
        Fmt::template write<typename Curve::Fq, F>(o, false, x, y, inf ? 0x40u : 0u);
    }
}

} // namespace codec

// ---- host side: run_chunks (staging.h) through a pinned block on the calling thread's setup stream --------------------
// At most POINT_CODEC_CHUNK points are on the device at a time: device memory and pinned host memory of a call are each
// bounded by POINT_CODEC_CHUNK x (input + output record) -- < 26 MB for uncompressed BLS12-381 G2, the largest record.
constexpr size_t POINT_CODEC_CHUNK = size_t(1) << 16;
constexpr Staging POINT_CODEC_STAGING{POINT_CODEC_CHUNK, true};

template <class Curve, int G, class Fmt> struct PointCodecT {
    typedef typename codec::Group<Curve, G>::F F;
    static constexpr size_t COORD = (size_t)F::N * 4; // bytes of one coordinate = words of F x 4
    static unsigned blocks(size_t cnt) { return (unsigned)((cnt + 255) / 256); }
    static int decode(const uint8_t *bytes, size_t n, bool compressed, bool checked, u64 *out, uint8_t *status) {
        const int cf = compressed, ck = checked;
        return run_chunks(POINT_CODEC_STAGING, n, nullptr, 0,
                          {Span::in(bytes, (compressed ? 1 : 2) * COORD), Span::out(out, 2 * COORD), Span::out(status, 1)}, 0,
                          [&](const Chunk &c) {
                              hipLaunchKernelGGL((codec::point_decode_kernel<Curve, G, Fmt>), dim3(blocks(c.n)), dim3(256), 0, c.stream,
                                                 (const u32 *)c.a[0], c.n, cf, ck, (u32 *)c.a[1], c.a[2]);
                              return hipGetLastError();
                          });
    }
    static int check(const u64 *aff, size_t n, uint8_t *status) {
        return run_chunks(POINT_CODEC_STAGING, n, nullptr, 0, {Span::in(aff, 2 * COORD), Span::out(status, 1)}, 0, [&](const Chunk &c) {
            hipLaunchKernelGGL((codec::point_check_kernel<Curve, G>), dim3(blocks(c.n)), dim3(256), 0, c.stream, (const u32 *)c.a[0],
                               c.n, c.a[1]);
            return hipGetLastError();
        });
    }
    static int encode(const u64 *aff, size_t n, bool compressed, uint8_t *out) {
        const int cf = compressed;
        return run_chunks(POINT_CODEC_STAGING, n, nullptr, 0, {Span::in(aff, 2 * COORD), Span::out(out, (compressed ? 1 : 2) * COORD)}, 0,
                          [&](const Chunk &c) {
                              hipLaunchKernelGGL((codec::point_encode_kernel<Curve, G, Fmt>), dim3(blocks(c.n)), dim3(256), 0, c.stream,
                                                 (const u32 *)c.a[0], c.n, cf, (u32 *)c.a[1]);
                              return hipGetLastError();
                          });
    }
};

// per-curve entry points (point_codec_<curve>.hip): op 0 decode, 1 check, 2 encode; format 0 arkworks, 1 PPoT (Bn254 only)
struct PointCodecArgs {
    int group, op, compressed, checked;
    const void *in;
    size_t n;
    void *out;
    uint8_t *status;
    int format = 0;
};
template <class Curve, class Fmt> int point_codec_dispatch(const PointCodecArgs &a) {
    if (a.group != 1 && a.group != 2) return MG_ERR_ARG;
    if (a.group == 1) {
        typedef PointCodecT<Curve, 1, Fmt> P;
        if (a.op == 0) return P::decode((const uint8_t *)a.in, a.n, a.compressed, a.checked, (u64 *)a.out, a.status);
        if (a.op == 1) return P::check((const u64 *)a.in, a.n, a.status);
        return P::encode((const u64 *)a.in, a.n, a.compressed, (uint8_t *)a.out);
    }
    typedef PointCodecT<Curve, 2, Fmt> P;
    if (a.op == 0) return P::decode((const uint8_t *)a.in, a.n, a.compressed, a.checked, (u64 *)a.out, a.status);
    if (a.op == 1) return P::check((const u64 *)a.in, a.n, a.status);
    return P::encode((const u64 *)a.in, a.n, a.compressed, (uint8_t *)a.out);
}
int point_codec_bn254(const PointCodecArgs &a);
int point_codec_bls381(const PointCodecArgs &a);

} // namespace mg
