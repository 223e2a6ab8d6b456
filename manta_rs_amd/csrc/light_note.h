// Batched AES-GCM notes of manta-pay (manta-pay/src/config/utxo.rs `IncomingBaseAES` 760-1031, `OutgoingBaseAES` 1511-1777,
// `AddressPartitionFunction` 1810-1831, the Merkle shard function 1319-1337; manta-pay/src/crypto/encryption/aes.rs): the host
// layer behind the C ABI mg_light_notes_* / mg_outgoing_notes_* / mg_address_partitions / mg_merkle_shard_indices /
// mg_aes256_gcm / mg_blake2s (light_note.cpp) and one launch function per kernel (light_note_bn254.hip). One note, key or leaf
// per lane; the key agreements are the kernels of edwards_bn254.hip.
#pragma once
#include "engine.h"
#include "fp_dev.h"

struct mg_utxo_model;

namespace mg {

enum { NOTE_OTHER_PARTITION = 3 }; // = MG_NOTE_OTHER_PARTITION of mantagpu.h; NOTE_OK / BAD_TAG / BAD_VALUE: edwards.h
constexpr int LIGHT_NOTE_BYTES = 96, OUTGOING_NOTE_BYTES = 64; // ciphertext | tag

// ---- the kernels: device pointers, n lanes on `s`. keys: the agreed points, affine Montgomery (16 words each), which stay on
// the device; a light plaintext is randomness | asset id | asset value (24 Montgomery words), an outgoing one asset id | asset
// value (16); a sealed note is ciphertext | tag (24 or 16 words); status: NOTE_*
// epks: null, or the ephemeral keys of the lanes, which a lane that is not NOTE_OK overwrites with zeros
hipError_t light_note_seal(hipStream_t s, const u32 *keys, const u32 *plain, size_t n, u32 *epks, u32 *sealed, uint8_t *status);
hipError_t outgoing_note_seal(hipStream_t s, const u32 *keys, const u32 *plain, size_t n, u32 *epks, u32 *sealed, uint8_t *status);
hipError_t light_note_open(hipStream_t s, const u32 *keys, const u32 *sealed, size_t n, u32 *plain, uint8_t *status);
hipError_t outgoing_note_open(hipStream_t s, const u32 *keys, const u32 *sealed, size_t n, u32 *plain, uint8_t *status);
// one byte per lane: the address partition of a point x | y (16 words), the shard index of a leaf (8 words)
hipError_t address_partition(hipStream_t s, const u32 *points, size_t n, uint8_t *out);
hipError_t merkle_shard_index(hipStream_t s, const u32 *leaves, size_t n, uint8_t *out);

// ---- the host layer (light_note.cpp): arrays in the caller's memory, the library's status
int blake2s_var(const uint8_t *data, size_t len, size_t out_len, uint8_t *out);
int aes256_gcm(const uint8_t *key, const uint8_t *nonce, const uint8_t *in, size_t len, int decrypt, uint8_t *out, int *ok);
int address_partitions(const mg_utxo_model *h, const u64 *recv_keys, size_t n, uint8_t *out);
int merkle_shard_indices(int curve, const u64 *leaves, size_t n, uint8_t *out);
int light_notes_encrypt(const mg_utxo_model *h, const u64 *recv_keys, const u64 *randomness, const u64 *plaintexts, size_t n,
                        u64 *epk_out, uint8_t *ciphertexts_out, uint8_t *status);
int light_notes_open(const mg_utxo_model *h, const u64 *viewing_key, const u64 *epks, const uint8_t *ciphertexts,
                     const uint8_t *partitions, size_t n, u64 *plaintext_out, uint8_t *ok, uint8_t *status, size_t *n_tried);
int outgoing_notes_encrypt(const mg_utxo_model *h, const u64 *recv_key, const u64 *randomness, const u64 *assets, size_t n,
                           u64 *epk_out, uint8_t *ciphertexts_out, uint8_t *status);
int outgoing_notes_open(const mg_utxo_model *h, const u64 *viewing_key, const u64 *epks, const uint8_t *ciphertexts, size_t n,
                        u64 *assets_out, uint8_t *ok, uint8_t *status);

} // namespace mg
