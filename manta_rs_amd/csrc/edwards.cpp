// Host layer of the embedded-curve operations and the Poseidon note encryption (mantagpu.h mg_edwards_* / mg_note_cipher_* /
// mg_notes_*): argument checks (all before any device work), chunking. Kernels in edwards_bn254.hip; the host group law and
// the fixed-base table in edwards_host.h.
#include "edwards.h"
#include "edwards_dev.h"
#include "edwards_host.h"
#include <cstring>
#include <vector>

struct mg_note_cipher {
    std::vector<mg::u32> prm;   // round keys | MDS | initial state, Montgomery words
    std::vector<mg::u32> table; // fixed-base table of the generator
};

namespace mg {

using namespace edh; // the host group law, the fixed-base table and the point / scalar checks, shared with utxo.cpp

int edwards_decode(int curve, const uint8_t *bytes, size_t n, int checked, u64 *out, uint8_t *status, size_t *n_bad) {
    if (curve != 0 || (n && (!bytes || !out))) return MG_ERR_ARG;
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    const int rc = run_chunks(EDWARDS_STAGING, n, nullptr, 0, {Span::in(bytes, 32), Span::out(out, 64), Span::out(status, 1)}, 0,
                              [&](const Chunk &c) {
                                  return ed_decode(c.stream, (const u32 *)c.a[0], c.n, checked != 0, (u32 *)c.a[1], c.a[2]);
                              });
    if (rc == MG_OK && n_bad) *n_bad = count_bad(status, n);
    return rc;
}

int edwards_check(int curve, const u64 *affine, size_t n, uint8_t *status, size_t *n_bad) {
    if (curve != 0 || (n && !affine)) return MG_ERR_ARG;
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    const int rc = run_chunks(EDWARDS_STAGING, n, nullptr, 0, {Span::in(affine, 64), Span::out(status, 1)}, 0, [&](const Chunk &c) {
        return ed_check(c.stream, (const u32 *)c.a[0], c.n, c.a[1]);
    });
    if (rc == MG_OK && n_bad) *n_bad = count_bad(status, n);
    return rc;
}

int edwards_encode(int curve, const u64 *affine, size_t n, uint8_t *out) {
    if (curve != 0 || (n && (!affine || !out))) return MG_ERR_ARG;
    return run_chunks(EDWARDS_STAGING, n, nullptr, 0, {Span::in(affine, 64), Span::out(out, 32)}, 0, [&](const Chunk &c) {
        return ed_encode(c.stream, (const u32 *)c.a[0], c.n, (u32 *)c.a[1]);
    });
}

int edwards_mul(int curve, int mode, const u64 *points, size_t n_points, const u64 *scalars, size_t n_scalars, u64 *out) {
    if (curve != 0 || mode < 0 || mode > 2) return MG_ERR_ARG;
    if ((n_points && !points) || (n_scalars && !scalars)) return MG_ERR_ARG;
    if (mode == 0 && n_scalars != 1) return MG_ERR_ARG;
    if (mode == 1 && n_points != 1) return MG_ERR_ARG;
    if (mode == 2 && n_points != n_scalars) return MG_ERR_ARG;
    const size_t n = mode == 0 ? n_points : n_scalars;
    if (n && !out) return MG_ERR_ARG;
    if (!scalars_ok(scalars, n_scalars)) return MG_ERR_ARG;
    if (mode == 1 && !coords_reduced(points)) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    if (mode == 0) {
        const int top = top_bit(scalars);
        return run_chunks(EDWARDS_STAGING, n, scalars, 32, {Span::in(points, 64), Span::out(out, 64)}, 0, [&](const Chunk &c) {
            return ed_mul_shared(c.stream, (const u32 *)c.a[0], c.n, (const u32 *)c.consts, top, (u32 *)c.a[1]);
        });
    }
    if (mode == 1) {
        std::vector<u32> table;
        build_table(points, table);
        return run_chunks(EDWARDS_STAGING, n, table.data(), table.size() * 4, {Span::in(scalars, 32), Span::out(out, 64)}, 0,
                          [&](const Chunk &c) {
                              return ed_mul_fixed(c.stream, (const u32 *)c.consts, (const u32 *)c.a[0], c.n, (u32 *)c.a[1]);
                          });
    }
    return run_chunks(EDWARDS_STAGING, n, nullptr, 0, {Span::in(points, 64), Span::in(scalars, 32), Span::out(out, 64)}, 0,
                      [&](const Chunk &c) {
                          return ed_mul_pairwise(c.stream, (const u32 *)c.a[0], (const u32 *)c.a[1], c.n, (u32 *)c.a[2]);
                      });
}

int edwards_add(int curve, const u64 *a_pts, const u64 *b_pts, size_t n, u64 *out) {
    if (curve != 0 || (n && (!a_pts || !b_pts || !out))) return MG_ERR_ARG;
    return run_chunks(EDWARDS_STAGING, n, nullptr, 0, {Span::in(a_pts, 64), Span::in(b_pts, 64), Span::out(out, 64)}, 0,
                      [&](const Chunk &c) {
                          return ed_add(c.stream, (const u32 *)c.a[0], (const u32 *)c.a[1], c.n, (u32 *)c.a[2]);
                      });
}

// bytes = `IncomingBaseEncryptionScheme` in the manta codec: the width-4 permutation (63 x 4 round keys | 4 x 4 MDS), then
// `FixedEncryption::initial_state` as a u64 length (4) and four elements
int note_cipher_create(int curve, const uint8_t *bytes, size_t len, const u64 *generator, mg_note_cipher **out) {
    if (out) *out = nullptr;
    if (curve != 0 || !bytes || !generator || !out) return MG_ERR_ARG;
    constexpr size_t NP = (size_t)(ED_CIPHER_FULL + ED_CIPHER_PARTIAL) * 4 + 16;
    if (len != NP * 32 + 8 + 4 * 32) return MG_ERR_ARG;
    u64 state_len;
    std::memcpy(&state_len, bytes + NP * 32, 8);
    if (state_len != 4) return MG_ERR_ARG;
    std::vector<u32> prm((size_t)ED_CIPHER_ELEMS * 8); // the permutation, then (behind the length) the initial state
    if (!decode_canonical_elements<Bn254FrCfg>(bytes, NP, prm.data()) ||
        !decode_canonical_elements<Bn254FrCfg>(bytes + NP * 32 + 8, ED_CIPHER_ELEMS - NP, &prm[NP * 8]))
        return MG_ERR_ARG;
    if (!coords_reduced(generator)) return MG_ERR_ARG;
    H gx, gy;
    std::memcpy(gx.v, generator, 32);
    std::memcpy(gy.v, generator + 4, 32);
    if (!h_on_curve(gx, gy)) return MG_ERR_ARG;
    mg_note_cipher *h = new mg_note_cipher;
    h->prm = std::move(prm);
    build_table(generator, h->table);
    *out = h;
    return MG_OK;
}

void note_cipher_destroy(mg_note_cipher *h) { delete h; }

// consts of a notes call: cipher parameters | fixed-base table | the shared scalar (decrypt)
int notes_encrypt(const mg_note_cipher *h, const u64 *recv_keys, const u64 *randomness, const u64 *plaintexts, size_t n,
                  u64 *epk_out, u64 *ciphertext_out, u64 *tag_out) {
    if (!h || (n && (!recv_keys || !randomness || !plaintexts || !epk_out || !ciphertext_out || !tag_out))) return MG_ERR_ARG;
    if (!scalars_ok(randomness, n)) return MG_ERR_ARG;
    std::vector<u32> consts(h->prm);
    consts.insert(consts.end(), h->table.begin(), h->table.end());
    const size_t prm_words = h->prm.size();
    return run_chunks(EDWARDS_STAGING, n, consts.data(), consts.size() * 4,
                      {Span::in(recv_keys, 64), Span::in(randomness, 32), Span::in(plaintexts, 96), Span::out(epk_out, 64),
                       Span::out(ciphertext_out, 96), Span::out(tag_out, 32)},
                      64, [&](const Chunk &c) {
                          const u32 *prm = (const u32 *)c.consts, *table = prm + prm_words, *rand = (const u32 *)c.a[1];
                          u32 *key = (u32 *)c.scratch;
                          hipError_t e = ed_mul_fixed(c.stream, table, rand, c.n, (u32 *)c.a[3]); // epk = G * randomness
                          if (e != hipSuccess) return e;
                          e = ed_mul_pairwise(c.stream, (const u32 *)c.a[0], rand, c.n, key); // key = recv_key * randomness
                          if (e != hipSuccess) return e;
                          return ed_encrypt(c.stream, prm, key, (const u32 *)c.a[2], c.n, (u32 *)c.a[4], (u32 *)c.a[5]);
                      });
}

int notes_decrypt(const mg_note_cipher *h, const u64 *viewing_key, const u64 *epks, const u64 *ciphertexts, const u64 *tags,
                  size_t n, u64 *plaintext_out, uint8_t *ok, uint8_t *status) {
    if (!h || !viewing_key || (n && (!epks || !ciphertexts || !tags || !plaintext_out || !ok))) return MG_ERR_ARG;
    if (!scalar_ok(viewing_key)) return MG_ERR_ARG;
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    std::vector<u32> consts(h->prm);
    const size_t prm_words = consts.size();
    consts.resize(prm_words + 8);
    std::memcpy(&consts[prm_words], viewing_key, 32);
    const int top = top_bit(viewing_key);
    const int rc = run_chunks(EDWARDS_STAGING, n, consts.data(), consts.size() * 4,
                              {Span::in(epks, 64), Span::in(ciphertexts, 96), Span::in(tags, 32), Span::out(plaintext_out, 96),
                               Span::out(status, 1)},
                              64, [&](const Chunk &c) {
                                  const u32 *prm = (const u32 *)c.consts;
                                  u32 *key = (u32 *)c.scratch; // key = epk * viewing key
                                  const hipError_t e = ed_mul_shared(c.stream, (const u32 *)c.a[0], c.n, prm + prm_words, top, key);
                                  if (e != hipSuccess) return e;
                                  return ed_decrypt(c.stream, prm, key, (const u32 *)c.a[1], (const u32 *)c.a[2], c.n,
                                                    (u32 *)c.a[3], c.a[4]);
                              });
    if (rc == MG_OK)
        for (size_t i = 0; i < n; ++i) ok[i] = status[i] == NOTE_OK;
    return rc;
}

} // namespace mg
