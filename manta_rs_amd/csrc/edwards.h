// Batched operations on manta-pay's embedded curve (ed_on_bn254) and its Poseidon note encryption: the host layer behind the C
// ABI mg_edwards_* / mg_note_cipher_* / mg_notes_* (edwards.cpp) and one launch function per kernel (edwards_bn254.hip; the group
// law and the fixed-base table are in edwards_dev.h). One point, scalar or note per lane.
#pragma once
#include "engine.h"
#include "fp_dev.h"

struct mg_note_cipher;

namespace mg {

constexpr size_t EDWARDS_CHUNK = size_t(1) << 16; // = MG_EDWARDS_CHUNK of mantagpu.h: lanes per device pass
// cipher parameters on the device: round keys[63 x 4] | MDS[16] | initial state[4], 8 words each
constexpr int ED_CIPHER_FULL = 8, ED_CIPHER_PARTIAL = 55, ED_CIPHER_ELEMS = (ED_CIPHER_FULL + ED_CIPHER_PARTIAL) * 4 + 16 + 4;

enum { NOTE_OK = 0, NOTE_BAD_TAG = 1, NOTE_BAD_VALUE = 2 }; // = MG_NOTE_* of mantagpu.h

// ---- the kernels: device pointers, n lanes on `s`. Points are affine Montgomery x | y (16 words), scalars 8 canonical words.
hipError_t ed_decode(hipStream_t s, const u32 *encodings, size_t n, bool checked /* run the subgroup test */, u32 *points,
                     uint8_t *status /* PT_* */);
hipError_t ed_check(hipStream_t s, const u32 *points, size_t n, uint8_t *status /* PT_* */);
hipError_t ed_encode(hipStream_t s, const u32 *points, size_t n, u32 *encodings);
// `scalar`: 8 words on the device, the same for every lane; top = the index of its top set bit, -1 for 0
hipError_t ed_mul_shared(hipStream_t s, const u32 *points, size_t n, const u32 *scalar, int top, u32 *out);
hipError_t ed_mul_fixed(hipStream_t s, const u32 *table, const u32 *scalars, size_t n, u32 *out);
hipError_t ed_mul_pairwise(hipStream_t s, const u32 *points, const u32 *scalars, size_t n, u32 *out);
hipError_t ed_add(hipStream_t s, const u32 *a, const u32 *b, size_t n, u32 *out);
// prm: the cipher parameters; keys: the agreed points; blocks of 3 field elements
hipError_t ed_encrypt(hipStream_t s, const u32 *prm, const u32 *keys, const u32 *plain, size_t n, u32 *cipher_out, u32 *tag_out);
hipError_t ed_decrypt(hipStream_t s, const u32 *prm, const u32 *keys, const u32 *blocks, const u32 *tags, size_t n,
                      u32 *plain_out, uint8_t *status /* NOTE_* */);

// ---- the host layer (edwards.cpp): arrays in the caller's memory, the library's status
int edwards_decode(int curve, const uint8_t *bytes, size_t n, int checked, u64 *out, uint8_t *status, size_t *n_bad);
int edwards_check(int curve, const u64 *affine, size_t n, uint8_t *status, size_t *n_bad);
int edwards_encode(int curve, const u64 *affine, size_t n, uint8_t *out);
int edwards_mul(int curve, int mode, const u64 *points, size_t n_points, const u64 *scalars, size_t n_scalars, u64 *out);
int edwards_add(int curve, const u64 *a_pts, const u64 *b_pts, size_t n, u64 *out);
int note_cipher_create(int curve, const uint8_t *bytes, size_t len, const u64 *generator, mg_note_cipher **out);
void note_cipher_destroy(mg_note_cipher *h);
int notes_encrypt(const mg_note_cipher *h, const u64 *recv_keys, const u64 *randomness, const u64 *plaintexts, size_t n,
                  u64 *epk_out, u64 *ciphertext_out, u64 *tag_out);
int notes_decrypt(const mg_note_cipher *h, const u64 *viewing_key, const u64 *epks, const u64 *ciphertexts, const u64 *tags,
                  size_t n, u64 *plaintext_out, uint8_t *ok, uint8_t *status);

} // namespace mg
