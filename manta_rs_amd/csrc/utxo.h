// Batched UTXO derivation of manta-pay (commitments, accumulator items, nullifier commitments, viewing keys): the host layer
// behind the C ABI mg_utxo_model_* / mg_utxos_* / mg_viewing_keys (utxo.cpp) and one launch function per kernel
// (utxo_bn254.hip). One UTXO or one key per lane.
#pragma once
#include "engine.h"
#include "fp_dev.h"

struct mg_utxo_model;

namespace mg {

enum { UTXO_OK = 0, UTXO_BAD_ENCODING = 1, UTXO_MISMATCH = 2 }; // = MG_UTXO_* of mantagpu.h

// The four hashers of the model in one device buffer, each as poseidon.h lays a hasher out (keys | mds | tag, 8 words per
// element), in the order of the chain: H5 (width 6), H4 (width 5), H3 (width 4), H2 (width 3). Offsets in words.
constexpr int UTXO_FULL = 8;
constexpr int utxo_prm_words(int t, int partial) { return ((UTXO_FULL + partial) * t + t * t + 1) * 8; }
constexpr int UTXO_H5_PARTIAL = 56, UTXO_H4_PARTIAL = 56, UTXO_H3_PARTIAL = 55, UTXO_H2_PARTIAL = 55;
constexpr int UTXO_H5_OFF = 0;
constexpr int UTXO_H4_OFF = UTXO_H5_OFF + utxo_prm_words(6, UTXO_H5_PARTIAL);
constexpr int UTXO_H3_OFF = UTXO_H4_OFF + utxo_prm_words(5, UTXO_H4_PARTIAL);
constexpr int UTXO_H2_OFF = UTXO_H3_OFF + utxo_prm_words(4, UTXO_H3_PARTIAL);
constexpr int UTXO_PRM_WORDS = UTXO_H2_OFF + utxo_prm_words(3, UTXO_H2_PARTIAL);

// ---- the kernels: device pointers, n lanes on `s`. prm: the four hashers; plain: blocks randomness | asset id | asset value
// (24 words each); a record is flag | public id | public value | commitment (32 words); status: UTXO_*
// flags: 0 opaque, 1 transparent
hipError_t utxo_mint(hipStream_t s, const u32 *prm, const u32 *recv_keys, const u32 *plain, const uint8_t *flags, size_t n,
                     u32 *utxos_out, u32 *items, uint8_t *status);
// shared: the address's receiving key x | y, then (with nullifiers) the authorization key x | y
hipError_t utxo_open(hipStream_t s, const u32 *prm, const u32 *shared, const u32 *plain, const u32 *utxos, size_t n, u32 *items,
                     u32 *nullifiers /* or null */, uint8_t *status);
// paks: proof authorization keys (affine, 16 words each); scalars: canonical limbs below l (8 words each)
hipError_t utxo_viewing_keys(hipStream_t s, const u32 *prm, const u32 *paks, size_t n, u32 *scalars);

// ---- the host layer (utxo.cpp): arrays in the caller's memory, the library's status
int utxo_model_create(int curve, const uint8_t *const *bytes, const size_t *len, mg_utxo_model **out);
void utxo_model_destroy(mg_utxo_model *h);
// the model's fixed-base table of the generator (edwards_dev.h, ED_TABLE_WORDS words), for the modules that share the handle
const u32 *utxo_model_table(const mg_utxo_model *h);
int utxos_mint(const mg_utxo_model *h, const u64 *recv_keys, const u64 *plaintexts, const uint8_t *flags, size_t n, u64 *utxos_out,
               u64 *items_out, uint8_t *status);
int utxos_open(const mg_utxo_model *h, const u64 *viewing_key, const u64 *pak, const u64 *plaintexts, const u64 *utxos, size_t n,
               uint8_t *status, u64 *items_out, u64 *nullifiers_out, size_t *n_ok);
int viewing_keys(const mg_utxo_model *h, const u64 *paks, size_t n, u64 *viewing_keys_out, u64 *recv_keys_out);

} // namespace mg
