// Batched Schnorr authorization signatures of manta-pay (manta-crypto/src/signature/mod.rs `schnorr`, manta-pay/src/config/
// utxo.rs `SchnorrHashFunction`, manta-accounting/src/transfer/utxo/protocol.rs `auth::VerifySignature`): the launch interface
// between the host layer (schnorr.cpp, the C ABI mg_schnorr_challenges / mg_signatures_verify / mg_signatures_sign) and the
// kernels (schnorr_bn254.hip). One signature per lane.
#pragma once
#include "engine.h"
#include "fp_dev.h"

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

struct SchnorrLaunch {
    enum Op { CHALLENGE, VERIFY, SIGN_FINISH };
    int op;
    const u32 *table;    // VERIFY: the fixed-base table of the generator (edwards.h)
    const u32 *pks;      // CHALLENGE / VERIFY: verifying keys, affine Montgomery (16 words each)
    const u32 *nonce_pts; // CHALLENGE / VERIFY: nonce points R
    const u32 *scalars;  // VERIFY: s; SIGN_FINISH: the nonces k (8 words each, canonical)
    const u32 *keys;     // SIGN_FINISH: the signing keys
    const u32 *messages; // CHALLENGE: rows of `stride` bytes (stride a multiple of 4; null when stride is 0)
    const u32 *lengths;  // CHALLENGE: bytes of each row that are the message, or null: all of `stride`
    u32 stride;
    u32 *challenges;     // CHALLENGE: out; VERIFY / SIGN_FINISH: in (8 words each, canonical, below l)
    u32 *out;            // SIGN_FINISH: s
    uint8_t *status;     // VERIFY: SIG_*
    size_t n;
    hipStream_t stream;
};
hipError_t schnorr_launch_bn254(const SchnorrLaunch &a);

} // namespace mg
