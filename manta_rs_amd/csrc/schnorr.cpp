// Host layer of the batched Schnorr authorization signatures (mantagpu.h mg_schnorr_challenges / mg_signatures_verify /
// mg_signatures_sign, mg_blake2s256): argument checks (all before any device work), chunking. Kernels in schnorr_bn254.hip;
// the fixed-base multiplications of a signing call are the kernel of edwards_bn254.hip on the model's table (utxo.h).
#include "schnorr.h"
#include "blake2s.h"
#include "edwards_host.h"
#include "utxo.h"
#include <vector>

namespace mg {
namespace {

using namespace edh;

// What the three calls share: the message rows cross as n rows of `stride` bytes with optional lengths. false: refused.
bool messages_ok(const uint8_t *messages, size_t stride, const uint32_t *lengths, size_t n) {
    if (!schnorr_sizes_ok(n, stride)) return false;
    if (n && stride && !messages) return false;
    for (size_t i = 0; lengths && i < n; ++i)
        if (lengths[i] > stride) return false;
    return true;
}

// the spans of the message rows and their lengths, where present; their positions in the chunk's arrays (-1: absent)
struct MessageSpans {
    int rows = -1, lengths = -1;
    void add(std::vector<Span> &arrays, const uint8_t *messages, size_t stride, const uint32_t *lens) {
        if (stride) rows = (int)arrays.size(), arrays.push_back(Span::in(messages, stride));
        if (lens) lengths = (int)arrays.size(), arrays.push_back(Span::in(lens, 4));
    }
    // the challenges of a chunk: its message rows hashed behind `pks` and `nonce_pts`
    hipError_t challenge(const Chunk &c, const u32 *pks, const u32 *nonce_pts, size_t stride, u32 *out) const {
        return schnorr_challenge(c.stream, pks, nonce_pts, rows < 0 ? nullptr : (const u32 *)c.a[rows],
                                 lengths < 0 ? nullptr : (const u32 *)c.a[lengths], (u32)stride, c.n, out);
    }
};

} // namespace

void blake2s256(const uint8_t *data, size_t len, uint8_t out[32]) { blake2s::hash(data, len, out); }

int schnorr_challenges(const mg_utxo_model *h, const u64 *pks, const u64 *nonce_points, const uint8_t *messages, size_t stride,
                       const uint32_t *lengths, size_t n, u64 *challenges_out) {
    if (!h || (n && (!pks || !nonce_points || !challenges_out)) || !messages_ok(messages, stride, lengths, n)) return MG_ERR_ARG;
    std::vector<Span> arrays = {Span::in(pks, 64), Span::in(nonce_points, 64), Span::out(challenges_out, 32)};
    MessageSpans ms;
    ms.add(arrays, messages, stride, lengths);
    return run_chunks(Staging{schnorr_lanes_per_pass(stride), false}, n, nullptr, 0, arrays, 0, [&](const Chunk &c) {
        return ms.challenge(c, (const u32 *)c.a[0], (const u32 *)c.a[1], stride, (u32 *)c.a[2]);
    });
}

// consts of a verifying call: the generator's table; scratch: the challenges
int signatures_verify(const mg_utxo_model *h, const u64 *pks, const u64 *nonce_points, const u64 *scalars, const uint8_t *messages,
                      size_t stride, const uint32_t *lengths, size_t n, uint8_t *status, size_t *n_ok) {
    if (!h || (n && (!pks || !nonce_points || !scalars)) || !messages_ok(messages, stride, lengths, n)) return MG_ERR_ARG;
    if (n_ok) *n_ok = 0;
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    std::vector<Span> arrays = {Span::in(pks, 64), Span::in(nonce_points, 64), Span::in(scalars, 32), Span::out(status, 1)};
    MessageSpans ms;
    ms.add(arrays, messages, stride, lengths);
    const int rc = run_chunks(Staging{schnorr_lanes_per_pass(stride), false}, n, utxo_model_table(h), (size_t)ED_TABLE_WORDS * 4,
                              arrays, 32, [&](const Chunk &c) {
                                  const u32 *pks = (const u32 *)c.a[0], *nonce_pts = (const u32 *)c.a[1];
                                  u32 *challenges = (u32 *)c.scratch;
                                  const hipError_t e = ms.challenge(c, pks, nonce_pts, stride, challenges);
                                  if (e != hipSuccess) return e;
                                  return schnorr_verify(c.stream, (const u32 *)c.consts, pks, nonce_pts, (const u32 *)c.a[2],
                                                        challenges, c.n, c.a[3]);
                              });
    if (rc == MG_OK && n_ok) *n_ok = n - count_bad(status, n);
    return rc;
}

// consts of a signing call: the generator's table; scratch: the challenges, then the verifying keys
int signatures_sign(const mg_utxo_model *h, const u64 *signing_keys, const u64 *nonces, const uint8_t *messages, size_t stride,
                    const uint32_t *lengths, size_t n, u64 *scalars_out, u64 *nonce_points_out, u64 *pks_out) {
    if (!h || (n && (!signing_keys || !nonces || !scalars_out || !nonce_points_out)) || !messages_ok(messages, stride, lengths, n))
        return MG_ERR_ARG;
    if (!scalars_ok(signing_keys, n) || !scalars_ok(nonces, n)) return MG_ERR_ARG;
    std::vector<Span> arrays = {Span::in(signing_keys, 32), Span::in(nonces, 32), Span::out(scalars_out, 32),
                                Span::out(nonce_points_out, 64)};
    const int pk_at = pks_out ? (int)arrays.size() : -1;
    if (pks_out) arrays.push_back(Span::out(pks_out, 64));
    MessageSpans ms;
    ms.add(arrays, messages, stride, lengths);
    return run_chunks(Staging{schnorr_lanes_per_pass(stride), false}, n, utxo_model_table(h), (size_t)ED_TABLE_WORDS * 4, arrays,
                      pks_out ? 32 : 96, [&](const Chunk &c) {
                          const u32 *table = (const u32 *)c.consts, *sk = (const u32 *)c.a[0], *k = (const u32 *)c.a[1];
                          u32 *nonce_pts = (u32 *)c.a[3], *challenges = (u32 *)c.scratch;
                          u32 *pk = pk_at < 0 ? (u32 *)(c.scratch + c.n * 32) : (u32 *)c.a[pk_at];
                          hipError_t e = ed_mul_fixed(c.stream, table, k, c.n, nonce_pts); // R = k G
                          if (e != hipSuccess) return e;
                          if ((e = ed_mul_fixed(c.stream, table, sk, c.n, pk)) != hipSuccess) return e; // pk = sk G
                          if ((e = ms.challenge(c, pk, nonce_pts, stride, challenges)) != hipSuccess) return e;
                          return schnorr_sign_finish(c.stream, sk, k, challenges, c.n, (u32 *)c.a[2]);
                      });
}

} // namespace mg
