// Batched Schnorr authorization signatures of manta-pay (manta-crypto/src/signature/mod.rs `schnorr`, manta-pay/src/config/
// utxo.rs `SchnorrHashFunction`, manta-accounting/src/transfer/utxo/protocol.rs `auth::VerifySignature`): the host layer behind
// the C ABI mg_schnorr_challenges / mg_signatures_verify / mg_signatures_sign / mg_blake2s256 (schnorr.cpp) and one launch function
// per kernel (schnorr_bn254.hip). One signature per lane.
#pragma once
#include "engine.h"
#include "fp_dev.h"

struct mg_utxo_model;

namespace mg {

enum { SIG_OK = 0, SIG_BAD_ENCODING = 1, SIG_DEGENERATE = 2, SIG_MISMATCH = 3 }; // = MG_SIG_* of mantagpu.h
constexpr size_t SIGNATURE_MAX_MESSAGE = size_t(1) << 16;                          // = MG_SIGNATURE_MAX_MESSAGE

// Lanes per device pass of a call whose message rows are `stride` bytes: 16 MiB of message rows, between 64 and 2^16 lanes.
// With stride <= SIGNATURE_MAX_MESSAGE a pass holds at most max(16 MiB, 64 x 64 KiB = 4 MiB) = 16 MiB of messages and at
// most 2^16 x 260 bytes = 16.25 MiB of everything else (sign: two scalars and a length in; a scalar, two points and the
// challenge out), beside the 94.5 KB table: the device memory of a call stays below 33 MiB whatever n and stride.
constexpr size_t schnorr_lanes_per_pass(size_t stride) {
    const size_t by_bytes = (size_t(16) << 20) / (stride < 4 ? 4 : stride);
    const size_t lanes = by_bytes < 64 ? 64 : by_bytes;
    return lanes < (size_t(1) << 16) ? lanes : size_t(1) << 16;
}
// the sizes a call multiplies: n rows of `stride` bytes and n records of up to 64 bytes must not wrap a size_t
constexpr bool schnorr_sizes_ok(size_t n, size_t stride) {
    return stride % 4 == 0 && stride <= SIGNATURE_MAX_MESSAGE && n <= SIZE_MAX / (stride < 64 ? 64 : stride);
}

// ---- the kernels: device pointers, n lanes on `s`. Points are affine Montgomery (16 words each); scalars and challenges are 8
// canonical words each, below l
// messages: rows of `stride` bytes (stride a multiple of 4; null when stride is 0); lengths: the bytes of each row that are the
// message, or null: all of `stride`
hipError_t schnorr_challenge(hipStream_t s, const u32 *pks, const u32 *nonce_pts, const u32 *messages, const u32 *lengths,
                             u32 stride, size_t n, u32 *challenges);
// table: the fixed-base table of the generator (edwards_dev.h); scalars: s; status: SIG_*
hipError_t schnorr_verify(hipStream_t s, const u32 *table, const u32 *pks, const u32 *nonce_pts, const u32 *scalars,
                          const u32 *challenges, size_t n, uint8_t *status);
hipError_t schnorr_sign_finish(hipStream_t s, const u32 *signing_keys, const u32 *nonces, const u32 *challenges, size_t n,
                               u32 *scalars_out);

// ---- the host layer (schnorr.cpp): arrays in the caller's memory, the library's status
void blake2s256(const uint8_t *data, size_t len, uint8_t out[32]);
int schnorr_challenges(const mg_utxo_model *h, const u64 *pks, const u64 *nonce_points, const uint8_t *messages, size_t stride,
                       const uint32_t *lengths, size_t n, u64 *challenges_out);
int signatures_verify(const mg_utxo_model *h, const u64 *pks, const u64 *nonce_points, const u64 *scalars, const uint8_t *messages,
                      size_t stride, const uint32_t *lengths, size_t n, uint8_t *status, size_t *n_ok);
int signatures_sign(const mg_utxo_model *h, const u64 *signing_keys, const u64 *nonces, const uint8_t *messages, size_t stride,
                    const uint32_t *lengths, size_t n, u64 *scalars_out, u64 *nonce_points_out, u64 *pks_out);

} // namespace mg
