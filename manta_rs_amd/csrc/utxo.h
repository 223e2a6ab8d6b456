// Batched UTXO derivation of manta-pay (commitments, accumulator items, nullifier commitments, viewing keys): the launch
// interface between the host layer (utxo.cpp, the C ABI mg_utxo_model_* / mg_utxos_* / mg_viewing_keys) and the kernels
// (utxo_bn254.hip). One UTXO or one key per lane.
#pragma once
#include "engine.h"
#include "fp_dev.h"

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

struct UtxoLaunch {
    enum Op { MINT, OPEN, VIEWING_KEYS };
    int op;
    const u32 *prm;       // the four hashers
    const u32 *shared;    // OPEN: the address's receiving key x | y, then (with nullifiers) the authorization key x | y
    const u32 *keys;      // MINT: receiving keys; VIEWING_KEYS: proof authorization keys (affine, 16 words each)
    const u32 *plain;     // MINT / OPEN: plaintext blocks randomness | asset id | asset value (24 words each)
    const uint8_t *flags; // MINT: 0 opaque, 1 transparent
    const u32 *utxos_in;  // OPEN: the ledger's records flag | public id | public value | commitment (32 words each)
    u32 *utxos_out;       // MINT: the records
    u32 *items;           // MINT / OPEN: accumulator items
    u32 *nullifiers;      // OPEN: nullifier commitments, or null
    u32 *scalars;         // VIEWING_KEYS: canonical limbs below l (8 words each)
    uint8_t *status;      // MINT / OPEN: UTXO_*
    size_t n;
    hipStream_t stream;
};
hipError_t utxo_launch_bn254(const UtxoLaunch &a);

} // namespace mg

struct mg_utxo_model;
namespace mg {
// the model's fixed-base table of the generator (edwards.h, ED_TABLE_WORDS words), for the modules that share the handle
const u32 *utxo_model_table(const mg_utxo_model *h);
} // namespace mg
