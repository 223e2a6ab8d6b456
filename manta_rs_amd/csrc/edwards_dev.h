// Device arithmetic of manta-pay's embedded curve on gfx950: ed_on_bn254 (`Group = ed_on_bn254::EdwardsProjective`,
// manta-pay/src/config/mod.rs), the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over BN254 Fr with a = 1,
// d = 168696 / 168700, cofactor 8 and a subgroup of prime order l (251 bits). Replaces, per lane, ark-ec 0.3
// `twisted_edwards_extended::{GroupAffine, GroupProjective}` (add, double, mul, `get_point_from_x`,
// `is_in_correct_subgroup_assuming_on_curve`).
//
// Extended coordinates (X : Y : Z : T), x = X / Z, y = Y / Z, T = X Y / Z, over the canonical, always fully reduced Fp<Fr> of
// fp_dev.h: every equality test below compares exact representations. d is a non-square and a = 1 a square mod p, so the
// unified addition law (Hisil-Wong-Carter-Dawson 2008, "add-2008-hwcd") is complete: no pair of curve points, small-order ones
// included, needs a branch, and the group law has no data-dependent control flow at all. Doubling is "dbl-2008-hwcd" (4 products
// and 4 squarings, T of the input unused); a general addition is 9 products and one by d, an addition of an affine point with
// d x y precomputed (AffineNiels) 8.
//
// Below the group law: the per-lane pieces that more than one kernel file runs (encoder, the two per-lane scalar products, the
// point and value predicates), and the launch shape all of these kernels share.
#pragma once
#include "fp_dev.h"
#include "params_gen.h"
#include "point_codec.h"

namespace mg {

// fixed-base table: entry [j][m] = m 16^j B as x | y | d x y (affine, Montgomery), j < 63, m < 16: a scalar below 2^252 is 63
// four-bit digits, its product 63 additions of gathered entries and no doubling
constexpr int ED_WINDOW_BITS = 4, ED_WINDOWS = 63, ED_TABLE_ENTRIES = ED_WINDOWS << ED_WINDOW_BITS;
constexpr int ED_TABLE_WORDS = ED_TABLE_ENTRIES * 24;

// One point, note, UTXO or signature per lane: n lanes in blocks of LANE_BLOCK. Nothing is launched for n == 0.
constexpr int LANE_BLOCK = 256;
template <class Kernel, class... Args> hipError_t launch_lanes(Kernel kernel, hipStream_t stream, size_t n, Args... args) {
    if (n == 0) return hipSuccess;
    kernel<<<dim3((unsigned)((n + LANE_BLOCK - 1) / LANE_BLOCK)), dim3(LANE_BLOCK), 0, stream>>>(args...);
    return hipGetLastError();
}

struct EdBn254 {
    typedef Bn254FrCfg Fq; // the base field of the embedded curve = the scalar field of BN254
    // d in Montgomery form; a = 1
    static constexpr u32 D[8] = {0x9fb08e74u, 0xe7a66d1du, 0xe17629dcu, 0xd775bbd5u, 0x286ef1e7u, 0x70ccd097u, 0x398fdf98u, 0x00045809u};
    // the order of the prime subgroup, a plain integer
    static constexpr u32 L[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu};
    static constexpr int L_BITS = 251;
    // ((p - 1) / 2^28 - 1) / 2, the exponent of the Tonelli-Shanks start value (225 bits)
    static constexpr u32 SQRT_EXP[8] = {0x1f0fac9fu, 0xcdcb848au, 0x419f4243u, 0x0c0ac2e9u, 0xc2822db4u, 0x098d014du, 0x83227397u, 0x00000001u};
    static constexpr int SQRT_EXP_BITS = 225;
};

namespace ed {

template <class E> struct Curve {
    typedef Fp<typename E::Fq> F;
    static MG_DEV F d() {
        F r;
#pragma unroll
        for (int i = 0; i < F::N; ++i) r.v[i] = E::D[i];
        return r;
    }
};

template <class F> struct Aff { // x | y in memory, identity = (0, 1)
    F x, y;
    static MG_DEV Aff load(const u32 *p) { return Aff{F::load(p), F::load(p + F::N)}; }
    MG_DEV void store(u32 *p) const {
        x.store(p);
        y.store(p + F::N);
    }
};

template <class F> struct Niels { // an affine addend with its product term ready: x, y, d x y
    F x, y, dt;
    static MG_DEV Niels load(const u32 *p) { return Niels{F::load(p), F::load(p + F::N), F::load(p + 2 * F::N)}; }
};

template <class E> struct Ext {
    typedef Fp<typename E::Fq> F;
    F X, Y, Z, T;

    static MG_DEV Ext identity() { return Ext{F::zero(), F::one(), F::one(), F::zero()}; }
    static MG_DEV Ext from_affine(const Aff<F> &p) { return Ext{p.x, p.y, F::one(), F::mul(p.x, p.y)}; }
    static MG_DEV Niels<F> niels(const Aff<F> &p) { return Niels<F>{p.x, p.y, F::mul(Curve<E>::d(), F::mul(p.x, p.y))}; }
    // (0 : 1 : 1 : 0) up to scaling; the point of order two is (0 : -1 : 1 : 0)
    MG_DEV bool is_identity() const { return X.is_zero() && Y == Z; }

    static MG_DEV Ext dbl(const Ext &p) {
        const F A = F::sqr(p.X), B = F::sqr(p.Y), C = F::dbl(F::sqr(p.Z));
        const F E_ = F::sub(F::sub(F::sqr(F::add(p.X, p.Y)), A), B);
        const F G = F::add(A, B), Fv = F::sub(G, C), H = F::sub(A, B); // a = 1: D = A
        return Ext{F::mul(E_, Fv), F::mul(G, H), F::mul(Fv, G), F::mul(E_, H)};
    }
    static MG_DEV Ext add(const Ext &p, const Ext &q) {
        const F A = F::mul(p.X, q.X), B = F::mul(p.Y, q.Y), C = F::mul(F::mul(p.T, q.T), Curve<E>::d()), D = F::mul(p.Z, q.Z);
        const F E_ = F::sub(F::sub(F::mul(F::add(p.X, p.Y), F::add(q.X, q.Y)), A), B);
        const F Fv = F::sub(D, C), G = F::add(D, C), H = F::sub(B, A);
        return Ext{F::mul(E_, Fv), F::mul(G, H), F::mul(Fv, G), F::mul(E_, H)};
    }
    static MG_DEV Ext madd(const Ext &p, const Niels<F> &q) { // q affine: Z2 = 1
        const F A = F::mul(p.X, q.x), B = F::mul(p.Y, q.y), C = F::mul(p.T, q.dt);
        const F E_ = F::sub(F::sub(F::mul(F::add(p.X, p.Y), F::add(q.x, q.y)), A), B);
        const F Fv = F::sub(p.Z, C), G = F::add(p.Z, C), H = F::sub(B, A);
        return Ext{F::mul(E_, Fv), F::mul(G, H), F::mul(Fv, G), F::mul(E_, H)};
    }
    static MG_DEV Ext select(bool c, const Ext &a, const Ext &b) {
        return Ext{F::select(c, a.X, b.X), F::select(c, a.Y, b.Y), F::select(c, a.Z, b.Z), F::select(c, a.T, b.T)};
    }
    // one Fermat inversion per lane; Z != 0 for every point the complete law produces from curve points
    MG_DEV Aff<F> to_affine() const {
        const F zi = F::inv(Z);
        return Aff<F>{F::mul(X, zi), F::mul(Y, zi)};
    }
};

// bit i of a little-endian word array whose index is not a compile-time constant, without indexing registers dynamically
template <int N> MG_DEV u32 bit_of(const u32 (&w)[N], int i) {
    u32 x = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (j == (i >> 5)) x = w[j];
    return (x >> (i & 31)) & 1u;
}

// [l] p == O (`is_in_correct_subgroup_assuming_on_curve`): double-and-add over the fixed bits of l, same path in every lane
template <class E> MG_DEV bool times_l_is_identity(const Aff<Fp<typename E::Fq>> &p) {
    const Niels<Fp<typename E::Fq>> q = Ext<E>::niels(p);
    Ext<E> acc = Ext<E>::from_affine(p);
    for (int i = E::L_BITS - 2; i >= 0; --i) {
        acc = Ext<E>::dbl(acc);
        u32 w = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j == (i >> 5)) w = E::L[j];
        if ((w >> (i & 31)) & 1) acc = Ext<E>::madd(acc, q);
    }
    return acc.is_identity();
}

// a x^2 + y^2 == 1 + d x^2 y^2
template <class E> MG_DEV bool on_curve(const Aff<Fp<typename E::Fq>> &p) {
    typedef Fp<typename E::Fq> F;
    const F x2 = F::sqr(p.x), y2 = F::sqr(p.y);
    return F::add(x2, y2) == F::add(F::one(), F::mul(Curve<E>::d(), F::mul(x2, y2)));
}

// PT_OK for a point with both coordinates canonical and on the curve, else the PT_* of the first of the two that fails
template <class E> MG_DEV uint8_t point_status(const Aff<Fp<typename E::Fq>> &p) {
    const bool bad = codec::geq_p<typename E::Fq>(p.x) || codec::geq_p<typename E::Fq>(p.y);
    const bool on = on_curve<E>(p);
    return bad ? PT_BAD_ENCODING : !on ? PT_NOT_ON_CURVE : PT_OK;
}

// ark-ec 0.3 `GroupAffine: CanonicalSerialize`: the identity (0, 1) is 32 zero bytes; any other point is x, canonical, with
// bit 255 = (y > -y)
template <class E> MG_DEV Fp<typename E::Fq> encode(const Aff<Fp<typename E::Fq>> &p) {
    typedef Fp<typename E::Fq> F;
    const bool ident = p.x.is_zero() && p.y == F::one();
    F x = F::from_mont(p.x);
    if (!ident && codec::is_high<typename E::Fq>(p.y)) x.v[7] |= 0x80000000u;
    return x;
}

// k B for k < 2^252 from the table of B (layout above): 63 gathered additions, no doubling
template <class E> MG_DEV Ext<E> mul_fixed(const u32 *table, const u32 (&k)[8]) {
    Ext<E> acc = Ext<E>::identity();
#pragma unroll 1
    for (int w = 0; w < ED_WINDOWS; ++w) {
        u32 word = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j == (w >> 3)) word = k[j];
        const u32 m = (word >> ((w & 7) * 4)) & 15u;
        acc = Ext<E>::madd(acc, Niels<Fp<typename E::Fq>>::load(table + (size_t)(w * 16 + m) * 24));
    }
    return acc;
}

// k q for k < 2^L_BITS, k different in every lane: double, add always, keep the sum where the lane's bit is set
template <class E> MG_DEV Ext<E> mul_select(const u32 (&k)[8], const Niels<Fp<typename E::Fq>> &q) {
    Ext<E> acc = Ext<E>::identity();
#pragma unroll 1
    for (int b = E::L_BITS - 1; b >= 0; --b) {
        acc = Ext<E>::dbl(acc);
        acc = Ext<E>::select(bit_of(k, b) != 0, Ext<E>::madd(acc, q), acc);
    }
    return acc;
}

// a^SQRT_EXP: a fixed exponent, square-and-multiply from the top
template <class E> MG_DEV Fp<typename E::Fq> pow_sqrt_exp(const Fp<typename E::Fq> &a) {
    typedef Fp<typename E::Fq> F;
    F acc = F::one();
    for (int i = E::SQRT_EXP_BITS - 1; i >= 0; --i) {
        acc = F::sqr(acc);
        u32 w = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j == (i >> 5)) w = E::SQRT_EXP[j];
        if ((w >> (i & 31)) & 1) acc = F::mul(acc, a);
    }
    return acc;
}

// Square root in a field with p - 1 = 2^S t, S = 28: Tonelli-Shanks with the iteration count fixed. x = a^((t + 1) / 2),
// b = a^t, z = a root of unity of order 2^S; with x^2 = a b kept, step k = S .. 2 tests b^(2^(k - 2)): if it is not 1 (then it is
// -1 and b has order 2^(k - 1)), x <- x z and b <- b z^2 make the order of b divide 2^(k - 2); z <- z^2. For a square a the
// loop ends with b = 1 and x^2 = a; for a non-square it cannot, and the final squaring decides. 351 + 225 squarings, every lane
// the same sequence, selects instead of branches.
template <class E> MG_DEV bool fsqrt(const Fp<typename E::Fq> &a, Fp<typename E::Fq> &r) {
    typedef typename E::Fq C;
    typedef Fp<C> F;
    static_assert(C::TWO_ADICITY == 28, "exponent constants are those of BN254 Fr");
    const F w = pow_sqrt_exp<E>(a);
    F x = F::mul(a, w), b = F::mul(x, w), z;
#pragma unroll
    for (int i = 0; i < F::N; ++i) z.v[i] = C::ROOT[i];
    const F one = F::one();
#pragma unroll 1
    for (int k = C::TWO_ADICITY; k >= 2; --k) {
        F bb = b;
#pragma unroll 1
        for (int j = 0; j < k - 2; ++j) bb = F::sqr(bb);
        const bool fix = !(bb == one);
        const F z2 = F::sqr(z);
        x = F::select(fix, F::mul(x, z), x);
        b = F::select(fix, F::mul(b, z2), b);
        z = z2;
    }
    r = x;
    return F::sqr(x) == a;
}

// manta-pay's `AssetValue` is a u128 (`try_into_u128`, config/utxo.rs:716-731): a value word (Montgomery) whose integer is
// 2^128 or more is no asset value
template <class F> MG_DEV bool fits_u128(const F &mont) {
    const F v = F::from_mont(mont);
    return (v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0;
}

// v -= 2^S l where v >= 2^S l, on plain integers
template <int S, class E = EdBn254> MG_DEV void sub_shifted_l_if_geq(u32 (&v)[8]) {
    u32 t[8], bw = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32 m = (E::L[i] << S) | (S && i ? E::L[i ? i - 1 : 0] >> ((32 - S) & 31) : 0u);
        const u64 d = (u64)v[i] - m - bw;
        t[i] = (u32)d;
        bw = (u32)(d >> 63);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bw ? v[i] : t[i];
}

} // namespace ed
} // namespace mg
