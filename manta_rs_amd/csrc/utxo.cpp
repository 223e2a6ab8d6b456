// Host layer of the batched UTXO derivation (mantagpu.h mg_utxo_model_* / mg_utxos_* / mg_viewing_keys): parameter decoding,
// argument checks (all before any device work), the address of an opening call, chunking. Kernels in utxo_bn254.hip; the
// fixed-base multiplication of the receiving keys is the kernel of edwards_bn254.hip.
#include "utxo.h"
#include "edwards_host.h"
#include <cstring>
#include <vector>

// Host memory only. The constants are uploaded once per CALL, with the call's other constants, into the call's DevBlock: a
// model that owned device memory would need one copy per device, a lock around their creation and an owner for their release
// beside other threads' stream captures (staging.h); 40 KB per call (134 KB with the table) is below a chunk's own copies.
struct mg_utxo_model {
    std::vector<mg::u32> prm;   // H5 | H4 | H3 | H2 as utxo.h lays them out, Montgomery words
    std::vector<mg::u32> table; // fixed-base table of the generator
};

namespace mg {
namespace {

using namespace edh;

H hpow(const H &a, const u32 *e, int bits) {
    H acc = H::one();
    for (int i = bits - 1; i >= 0; --i) {
        acc = H::sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = H::mul(acc, a);
    }
    return acc;
}

// Tonelli-Shanks as edwards_dev.h fsqrt runs it (p - 1 = 2^28 t); false: a is not a square
bool hsqrt(const H &a, H &r) {
    const H w = hpow(a, EdBn254::SQRT_EXP, EdBn254::SQRT_EXP_BITS);
    H x = H::mul(a, w), b = H::mul(x, w), z = h_const(Bn254FrCfg::ROOT);
    for (int k = Bn254FrCfg::TWO_ADICITY; k >= 2; --k) {
        H bb = b;
        for (int j = 0; j < k - 2; ++j) bb = H::sqr(bb);
        const H z2 = H::sqr(z);
        if (!(bb == H::one())) {
            x = H::mul(x, z);
            b = H::mul(b, z2);
        }
        z = z2;
    }
    r = x;
    return H::sqr(x) == a;
}

bool in_subgroup(const H &x, const H &y) { // [l] P == O
    const HExt p = HExt::from_affine(x, y);
    HExt acc = p;
    for (int i = EdBn254::L_BITS - 2; i >= 0; --i) {
        acc = HExt::dbl(acc);
        if ((EdBn254::L[i >> 5] >> (i & 31)) & 1) acc = HExt::add(acc, p);
    }
    return acc.is_identity();
}

// group-generator.dat: the ark-ec 0.3 encoding mg_edwards_decode reads (x little-endian, bit 255 = y is the larger root),
// checked: x < p, on the curve, of order l (so not the identity). out = x | y Montgomery.
bool decode_generator(const uint8_t *bytes, u64 *out) {
    H x;
    std::memcpy(x.v, bytes, 32);
    const bool greatest = (x.v[3] >> 63) != 0;
    x.v[3] &= ~(u64(1) << 63);
    if (H::geq_p(x.v) || x.is_zero()) return false;
    x = H::to_mont(x);
    const H x2 = H::sqr(x), one = H::one();
    H y;
    if (!hsqrt(H::mul(H::sub(x2, one), H::inv(H::sub(H::mul(h_const(EdBn254::D), x2), one))), y)) return false;
    if (y.is_high() != greatest) y = H::neg(y);
    if (!h_on_curve(x, y) || !in_subgroup(x, y)) return false;
    std::memcpy(out, x.v, 32);
    std::memcpy(out + 4, y.v, 32);
    return true;
}

} // namespace

// spans = the four `Hasher` files in the order of utxo.h, then the generator
int utxo_model_create(int curve, const uint8_t *const *bytes, const size_t *len, mg_utxo_model **out) {
    if (out) *out = nullptr;
    if (curve != 0 || !bytes || !len || !out) return MG_ERR_ARG;
    static const int off[5] = {UTXO_H5_OFF, UTXO_H4_OFF, UTXO_H3_OFF, UTXO_H2_OFF, UTXO_PRM_WORDS};
    for (int i = 0; i < 5; ++i)
        if (!bytes[i]) return MG_ERR_ARG;
    std::vector<u32> prm(UTXO_PRM_WORDS);
    for (int i = 0; i < 4; ++i) {
        const size_t count = (size_t)(off[i + 1] - off[i]) / 8;
        if (len[i] != count * 32 || !decode_canonical_elements<Bn254FrCfg>(bytes[i], count, &prm[off[i]])) return MG_ERR_ARG;
    }
    u64 g[8];
    if (len[4] != 32 || !decode_generator(bytes[4], g)) return MG_ERR_ARG;
    mg_utxo_model *h = new mg_utxo_model;
    h->prm = std::move(prm);
    build_table(g, h->table);
    *out = h;
    return MG_OK;
}

void utxo_model_destroy(mg_utxo_model *h) { delete h; }
const u32 *utxo_model_table(const mg_utxo_model *h) { return h->table.data(); }

int utxos_mint(const mg_utxo_model *h, const u64 *recv_keys, const u64 *plaintexts, const uint8_t *flags, size_t n, u64 *utxos_out,
               u64 *items_out, uint8_t *status) {
    if (!h || (n && (!recv_keys || !plaintexts || !flags || !utxos_out || !items_out || !status))) return MG_ERR_ARG;
    return run_chunks(EDWARDS_STAGING, n, h->prm.data(), h->prm.size() * 4,
                      {Span::in(recv_keys, 64), Span::in(plaintexts, 96), Span::in(flags, 1), Span::out(utxos_out, 128),
                       Span::out(items_out, 32), Span::out(status, 1)},
                      0, [&](const Chunk &c) {
                          return utxo_mint(c.stream, (const u32 *)c.consts, (const u32 *)c.a[0], (const u32 *)c.a[1], c.a[2], c.n,
                                           (u32 *)c.a[3], (u32 *)c.a[4], c.a[5]);
                      });
}

// consts of an opening call: the four hashers | address x | y | authorization key x | y
int utxos_open(const mg_utxo_model *h, const u64 *viewing_key, const u64 *pak, const u64 *plaintexts, const u64 *utxos, size_t n,
               uint8_t *status, u64 *items_out, u64 *nullifiers_out, size_t *n_ok) {
    if (!h || !viewing_key || (n && (!plaintexts || !utxos || !status || !items_out))) return MG_ERR_ARG;
    if ((pak != nullptr) != (nullifiers_out != nullptr)) return MG_ERR_ARG;
    if (!scalar_ok(viewing_key) || (pak && !point_ok(pak))) return MG_ERR_ARG;
    if (n_ok) *n_ok = 0;
    if (n == 0) return MG_OK;
    std::vector<u32> consts(h->prm);
    consts.resize(UTXO_PRM_WORDS + 32);
    fixed_base_mul(h->table.data(), viewing_key, &consts[UTXO_PRM_WORDS]); // `derive_address`, once per call
    if (pak) std::memcpy(&consts[UTXO_PRM_WORDS + 16], pak, 64);
    std::vector<Span> arrays = {Span::in(plaintexts, 96), Span::in(utxos, 128), Span::out(status, 1), Span::out(items_out, 32)};
    if (pak) arrays.push_back(Span::out(nullifiers_out, 32));
    const int rc = run_chunks(EDWARDS_STAGING, n, consts.data(), consts.size() * 4, arrays, 0, [&](const Chunk &c) {
        const u32 *prm = (const u32 *)c.consts;
        return utxo_open(c.stream, prm, prm + UTXO_PRM_WORDS, (const u32 *)c.a[0], (const u32 *)c.a[1], c.n, (u32 *)c.a[3],
                         pak ? (u32 *)c.a[4] : nullptr, c.a[2]);
    });
    if (rc == MG_OK && n_ok) *n_ok = n - count_bad(status, n);
    return rc;
}

// consts of a key call: the four hashers | the generator's table
int viewing_keys(const mg_utxo_model *h, const u64 *paks, size_t n, u64 *viewing_keys_out, u64 *recv_keys_out) {
    if (!h || (n && (!paks || !viewing_keys_out))) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    std::vector<u32> consts(h->prm);
    if (recv_keys_out) consts.insert(consts.end(), h->table.begin(), h->table.end());
    std::vector<Span> arrays = {Span::in(paks, 64), Span::out(viewing_keys_out, 32)};
    if (recv_keys_out) arrays.push_back(Span::out(recv_keys_out, 64));
    return run_chunks(EDWARDS_STAGING, n, consts.data(), consts.size() * 4, arrays, 0, [&](const Chunk &c) {
        const u32 *prm = (const u32 *)c.consts;
        u32 *scalars = (u32 *)c.a[1];
        const hipError_t e = utxo_viewing_keys(c.stream, prm, (const u32 *)c.a[0], c.n, scalars);
        if (e != hipSuccess || !recv_keys_out) return e;
        // receiving key = G * viewing key, from the scalars the kernel above left on the device
        return ed_mul_fixed(c.stream, prm + UTXO_PRM_WORDS, scalars, c.n, (u32 *)c.a[2]);
    });
}

} // namespace mg
