// Host side of the embedded curve (ed_on_bn254) shared by edwards.cpp and utxo.cpp: the group law of edwards_dev.h on the
// host, the fixed-base table, the argument checks on points and scalars, and the staging choice of the embedded-curve calls.
// Host-only; no kernel lives here.
#pragma once
#include "edwards.h"
#include "edwards_dev.h"
#include "host_ec.h"
#include "staging.h"
#include <cstring>
#include <vector>

namespace mg {
namespace edh {

typedef host::HFp<Bn254FrCfg> H;

inline H h_const(const u32 *w) {
    H r;
    r.load_words(w);
    return r;
}

// the group law of edwards_dev.h on the host, for the 1 008 entries of a fixed-base table
struct HExt {
    H X, Y, Z, T;
    static HExt identity() { return HExt{H::zero(), H::one(), H::one(), H::zero()}; }
    static HExt from_affine(const H &x, const H &y) { return HExt{x, y, H::one(), H::mul(x, y)}; }
    static HExt dbl(const HExt &p) {
        const H A = H::sqr(p.X), B = H::sqr(p.Y), C = H::dbl(H::sqr(p.Z));
        const H E = H::sub(H::sub(H::sqr(H::add(p.X, p.Y)), A), B), G = H::add(A, B), F = H::sub(G, C), Hh = H::sub(A, B);
        return HExt{H::mul(E, F), H::mul(G, Hh), H::mul(F, G), H::mul(E, Hh)};
    }
    static HExt add(const HExt &p, const HExt &q) {
        const H A = H::mul(p.X, q.X), B = H::mul(p.Y, q.Y), C = H::mul(H::mul(p.T, q.T), h_const(EdBn254::D)), D = H::mul(p.Z, q.Z);
        const H E = H::sub(H::sub(H::mul(H::add(p.X, p.Y), H::add(q.X, q.Y)), A), B);
        const H F = H::sub(D, C), G = H::add(D, C), Hh = H::sub(B, A);
        return HExt{H::mul(E, F), H::mul(G, Hh), H::mul(F, G), H::mul(E, Hh)};
    }
    bool is_identity() const { return X.is_zero() && Y == Z; }
};

inline bool coords_reduced(const u64 *p) { return !H::geq_p(p) && !H::geq_p(p + 4); }
inline bool h_on_curve(const H &x, const H &y) {
    const H x2 = H::sqr(x), y2 = H::sqr(y);
    return H::add(x2, y2) == H::add(H::one(), H::mul(h_const(EdBn254::D), H::mul(x2, y2)));
}
// an affine Montgomery point x | y with both coordinates reduced and on the curve
inline bool point_ok(const u64 *p) {
    if (!coords_reduced(p)) return false;
    H x, y;
    std::memcpy(x.v, p, 32);
    std::memcpy(y.v, p + 4, 32);
    return h_on_curve(x, y);
}

// entry [j][m] = m 16^j B as x | y | d x y; one inversion for the whole table (Montgomery's trick)
inline void build_table(const u64 *base, std::vector<u32> &out) {
    H bx, by;
    std::memcpy(bx.v, base, 32);
    std::memcpy(by.v, base + 4, 32);
    std::vector<HExt> e(ED_TABLE_ENTRIES);
    HExt w = HExt::from_affine(bx, by);
    const HExt id = HExt::identity();
    for (int j = 0; j < ED_WINDOWS; ++j) {
        e[j * 16] = id;
        e[j * 16 + 1] = w;
        for (int m = 2; m < 16; ++m) e[j * 16 + m] = HExt::add(e[j * 16 + m - 1], w);
        for (int k = 0; k < ED_WINDOW_BITS; ++k) w = HExt::dbl(w);
    }
    std::vector<H> pre(ED_TABLE_ENTRIES);
    H acc = H::one();
    for (int i = 0; i < ED_TABLE_ENTRIES; ++i) {
        pre[i] = acc;
        acc = H::mul(acc, e[i].Z);
    }
    H inv = H::inv(acc);
    const H d = h_const(EdBn254::D);
    out.resize(ED_TABLE_WORDS);
    for (int i = ED_TABLE_ENTRIES - 1; i >= 0; --i) {
        const H zi = H::mul(inv, pre[i]);
        inv = H::mul(inv, e[i].Z);
        const H x = H::mul(e[i].X, zi), y = H::mul(e[i].Y, zi);
        x.store_words(&out[(size_t)i * 24]);
        y.store_words(&out[(size_t)i * 24 + 8]);
        H::mul(d, H::mul(x, y)).store_words(&out[(size_t)i * 24 + 16]);
    }
}

// k B for k < 2^252 from the table of B (63 entries, one per digit), affine Montgomery x | y
inline void fixed_base_mul(const u32 *table, const u64 *k, u32 *out) {
    HExt acc = HExt::identity();
    for (int w = 0; w < ED_WINDOWS; ++w) {
        const u32 m = (u32)(k[w >> 4] >> ((w & 15) * 4)) & 15u;
        const u32 *e = &table[(size_t)(w * 16 + m) * 24];
        acc = HExt::add(acc, HExt::from_affine(h_const(e), h_const(e + 8)));
    }
    const H zi = H::inv(acc.Z);
    H::mul(acc.X, zi).store_words(out);
    H::mul(acc.Y, zi).store_words(out + 8);
}

inline bool scalar_ok(const u64 *k) { // < l
    for (int i = 3; i >= 0; --i) {
        const u64 li = (u64)EdBn254::L[2 * i] | ((u64)EdBn254::L[2 * i + 1] << 32);
        if (k[i] != li) return k[i] < li;
    }
    return false;
}
inline bool scalars_ok(const u64 *k, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!scalar_ok(k + 4 * i)) return false;
    return true;
}
inline int top_bit(const u64 *k) {
    for (int i = 255; i >= 0; --i)
        if ((k[i >> 6] >> (i & 63)) & 1) return i;
    return -1;
}

constexpr Staging EDWARDS_STAGING{EDWARDS_CHUNK, false}; // pageable: copies go straight from and to the caller's arrays

} // namespace edh
} // namespace mg
