// Batched operations on manta-pay's embedded curve (ed_on_bn254) and its Poseidon note encryption: the launch interface between
// the host layer (edwards.cpp, the C ABI mg_edwards_* / mg_note_cipher_* / mg_notes_*) and the kernels (edwards_bn254.hip; the
// group law is in edwards_dev.h). One point, scalar or note per lane.
#pragma once
#include "engine.h"
#include "fp_dev.h"

namespace mg {

constexpr size_t EDWARDS_CHUNK = size_t(1) << 16; // = MG_EDWARDS_CHUNK of mantagpu.h: lanes per device pass
// fixed-base table: entry [j][m] = m 16^j B as x | y | d x y (affine, Montgomery), j < 63, m < 16: a scalar below 2^252 is 63
// four-bit digits, its product 63 additions of gathered entries and no doubling
constexpr int ED_WINDOW_BITS = 4, ED_WINDOWS = 63, ED_TABLE_ENTRIES = ED_WINDOWS << ED_WINDOW_BITS;
constexpr int ED_TABLE_WORDS = ED_TABLE_ENTRIES * 24;
// cipher parameters on the device: round keys[63 x 4] | MDS[16] | initial state[4], 8 words each
constexpr int ED_CIPHER_FULL = 8, ED_CIPHER_PARTIAL = 55, ED_CIPHER_ELEMS = (ED_CIPHER_FULL + ED_CIPHER_PARTIAL) * 4 + 16 + 4;

enum { NOTE_OK = 0, NOTE_BAD_TAG = 1, NOTE_BAD_VALUE = 2 }; // = MG_NOTE_* of mantagpu.h

struct EdwardsLaunch {
    enum Op { DECODE, CHECK, ENCODE, MUL_SHARED, MUL_FIXED, MUL_PAIRWISE, ADD, ENCRYPT, DECRYPT };
    int op;
    int checked;       // DECODE: run the subgroup test
    int top;           // MUL_SHARED: index of the scalar's top set bit, -1 for 0
    const u32 *consts; // MUL_SHARED: the scalar (8 words); MUL_FIXED: the table; ENCRYPT / DECRYPT: the cipher parameters
    const u32 *a;      // points (DECODE: encodings; MUL_FIXED: unused; ENCRYPT / DECRYPT: the agreed keys)
    const u32 *b;      // MUL_FIXED / MUL_PAIRWISE: scalars; ADD: the second points; ENCRYPT / DECRYPT: the 3-word blocks
    const u32 *c;      // DECRYPT: the tags
    u32 *out;          // points / encodings / the 3-word blocks
    u32 *out2;         // ENCRYPT: the tags
    uint8_t *status;   // DECODE / CHECK: PT_*; DECRYPT: NOTE_*
    size_t n;
    hipStream_t stream;
};
hipError_t edwards_launch_bn254(const EdwardsLaunch &a);

} // namespace mg
