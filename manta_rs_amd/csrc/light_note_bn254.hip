// Kernels of manta-pay's AES-GCM notes over ed_on_bn254 and of its two one-byte hashes: one note, key or leaf per lane, wave64.
// A note is sealed under key = Blake2s-256(enc(K)), K the agreed point that a key-agreement kernel of edwards_bn254.hip left on
// the device (`recv_key * randomness` when sealing, `epk * viewing_key` when opening; utxo.rs:907-949, 1658-1700), with
// AES-256-GCM under the fixed nonce "random nonce" (crypto/encryption/aes.rs). The light incoming note is randomness | asset id
// (32 bytes little-endian canonical each) | asset value (u128, 16 bytes): 80 bytes, five blocks; the outgoing note asset id |
// asset value: 48 bytes, three blocks. Encoder: edwards_dev.h; hash: blake2s.h; cipher: aes_gcm.h. Behind each kernel, its
// launch function (light_note.h).
#include "light_note.h"
#include "aes_gcm.h"
#include "blake2s.h"
#include "edwards.h"
#include "edwards_dev.h"

namespace mg {
namespace lnote {

typedef EdBn254 E;
typedef Bn254FrCfg C;
typedef Fp<C> F;
typedef ed::Aff<F> A;

// a string as little-endian words, zeros behind its last byte
template <int W> struct Words {
    u32 w[W];
};
template <int W, int N> constexpr Words<W> words_of(const char (&s)[N]) {
    Words<W> r{};
    for (int k = 0; k < N - 1; ++k) r.w[k >> 2] |= (u32)(uint8_t)s[k] << (8 * (k & 3));
    return r;
}
constexpr Words<3> NONCE = words_of<3>("random nonce");
// both 39 bytes: the field bytes behind them start three bytes into word 9
constexpr int PREFIX_BYTES = 39, PREFIX_WORDS = 10;
constexpr Words<PREFIX_WORDS> ADDRESS_PARTITION = words_of<PREFIX_WORDS>("manta-v1.0.0/address-partition-function");
constexpr Words<PREFIX_WORDS> MERKLE_SHARD = words_of<PREFIX_WORDS>("manta-v1.0.0/merkle-tree-shard-function");
static_assert(sizeof("manta-v1.0.0/address-partition-function") - 1 == PREFIX_BYTES, "prefix length");
static_assert(sizeof("manta-v1.0.0/merkle-tree-shard-function") - 1 == PREFIX_BYTES, "prefix length");

// The S-box of a block in LDS: the lookups of a lane have key-dependent addresses
struct LdsSbox {
    const uint8_t *t;
    MG_DEV u32 operator()(u32 b) const { return t[b]; }
};
// the 32 bytes of an encoded point as the stream of blake2s::digest: one block
struct PointStream {
    u32 v[8];
    template <int J> MG_DEV u32 word(u64) const { return J < 8 ? v[J < 8 ? J : 0] : 0u; }
};

// One kernel per note kind and direction. ELEMS = the field elements of a plaintext (3 light, 2 outgoing): ELEMS - 1 whole
// elements, then the value's low 16 bytes. The whole chain runs here: encode the agreed point, hash it to the key, expand the key,
// H and AES_K(J0), the counter blocks, GHASH, and the codec between Montgomery words and canonical bytes. No lane branches on
// its data: a lane whose value is 2^128 or more (sealing), whose tag differs or whose elements are not below r (opening)
// computes on and stores zeros.
template <int ELEMS, bool OPEN>
__global__ __launch_bounds__(LANE_BLOCK) void note_kernel(const u32 *__restrict__ keys, const u32 *__restrict__ in, size_t n,
                                                          u32 *__restrict__ epks, u32 *__restrict__ out,
                                                          uint8_t *__restrict__ status) {
    static_assert(LANE_BLOCK == 256, "one S-box entry per thread of the block");
    __shared__ uint8_t sbox[256];
    sbox[threadIdx.x] = (uint8_t)aes::sbox_entry(threadIdx.x);
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int WHOLE = ELEMS - 1, WORDS = 8 * WHOLE + 4, BLOCKS = WORDS / 4, SEALED = WORDS + 4;
    PointStream ps;
    const F enc = ed::encode<E>(A::load(keys + i * 16));
#pragma unroll
    for (int j = 0; j < 8; ++j) ps.v[j] = enc.v[j];
    u32 key[8], data[WORDS], tag[4];
    blake2s::digest(32, ps, key);
    const LdsSbox s{sbox};
    if (!OPEN) {
        const u32 *pt = in + i * (size_t)(8 * ELEMS);
#pragma unroll
        for (int e = 0; e < WHOLE; ++e) {
            const F v = F::from_mont(F::load(pt + e * 8));
#pragma unroll
            for (int j = 0; j < 8; ++j) data[e * 8 + j] = v.v[j];
        }
        const F value = F::from_mont(F::load(pt + WHOLE * 8));
#pragma unroll
        for (int j = 0; j < 4; ++j) data[WHOLE * 8 + j] = value.v[j];
        const bool bad = (value.v[4] | value.v[5] | value.v[6] | value.v[7]) != 0; // `try_into_u128`
        aes::crypt_blocks<BLOCKS, false>(s, key, NONCE.w, data, tag);
        u32 *o = out + i * (size_t)SEALED;
#pragma unroll
        for (int j = 0; j < WORDS; ++j) o[j] = bad ? 0u : data[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[WORDS + j] = bad ? 0u : tag[j];
        status[i] = bad ? NOTE_BAD_VALUE : NOTE_OK;
        if (epks && bad) {
#pragma unroll
            for (int j = 0; j < 16; ++j) epks[i * 16 + j] = 0u;
        }
    } else {
        const u32 *c = in + i * (size_t)SEALED;
#pragma unroll
        for (int j = 0; j < WORDS; ++j) data[j] = c[j];
        aes::crypt_blocks<BLOCKS, true>(s, key, NONCE.w, data, tag);
        u32 diff = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) diff |= tag[j] ^ c[WORDS + j];
        bool big = false; // the reference `.expect()`s canonical elements behind a valid tag; the library reports
        F m[ELEMS];
#pragma unroll
        for (int e = 0; e < WHOLE; ++e) {
#pragma unroll
            for (int j = 0; j < 8; ++j) m[e].v[j] = data[e * 8 + j];
            big = big || codec::geq_p<C>(m[e]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) m[WHOLE].v[j] = j < 4 ? data[WHOLE * 8 + (j < 4 ? j : 0)] : 0u;
        const uint8_t st = diff ? NOTE_BAD_TAG : big ? NOTE_BAD_VALUE : NOTE_OK;
        const F z = F::zero();
#pragma unroll
        for (int e = 0; e < ELEMS; ++e) F::select(st == NOTE_OK, F::to_mont(m[e]), z).store(out + (i * ELEMS + e) * 8);
        status[i] = st;
    }
}

// One byte per lane: Blake2s with digest length 1 over prefix | ELEMS elements as 32 bytes little-endian canonical each. The
// stream is 39 + 32 ELEMS bytes, two blocks, whose words are put together here from the canonical words shifted by three bytes.
template <int ELEMS>
__global__ __launch_bounds__(LANE_BLOCK) void byte_hash_kernel(const u32 *__restrict__ in, size_t n, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int EW = 8 * ELEMS;
    u32 e[EW], m[2][16];
#pragma unroll
    for (int k = 0; k < ELEMS; ++k) {
        const F v = F::from_mont(F::load(in + (i * ELEMS + k) * 8));
#pragma unroll
        for (int j = 0; j < 8; ++j) e[k * 8 + j] = v.v[j];
    }
#pragma unroll
    for (int w = 0; w < 32; ++w) {
        const int j = w - (PREFIX_WORDS - 1); // the element word whose first byte is the top byte of stream word w
        u32 x = 0;
        if (w < PREFIX_WORDS) x = ELEMS == 2 ? ADDRESS_PARTITION.w[w < PREFIX_WORDS ? w : 0] : MERKLE_SHARD.w[w < PREFIX_WORDS ? w : 0];
        if (j >= 1 && j <= EW) x = e[j >= 1 && j <= EW ? j - 1 : 0] >> 8;
        if (j >= 0 && j < EW) x |= e[j >= 0 && j < EW ? j : 0] << 24;
        m[w >> 4][w & 15] = x;
    }
    u32 h[8];
    blake2s::init(h, 1);
    blake2s::compress(h, m[0], 64, false);
    blake2s::compress(h, m[1], PREFIX_BYTES + 32 * ELEMS, true);
    out[i] = (uint8_t)h[0];
}

} // namespace lnote

hipError_t light_note_seal(hipStream_t s, const u32 *keys, const u32 *plain, size_t n, u32 *epks, u32 *sealed, uint8_t *status) {
    return launch_lanes(lnote::note_kernel<3, false>, s, n, keys, plain, n, epks, sealed, status);
}
hipError_t outgoing_note_seal(hipStream_t s, const u32 *keys, const u32 *plain, size_t n, u32 *epks, u32 *sealed, uint8_t *status) {
    return launch_lanes(lnote::note_kernel<2, false>, s, n, keys, plain, n, epks, sealed, status);
}
hipError_t light_note_open(hipStream_t s, const u32 *keys, const u32 *sealed, size_t n, u32 *plain, uint8_t *status) {
    return launch_lanes(lnote::note_kernel<3, true>, s, n, keys, sealed, n, (u32 *)nullptr, plain, status);
}
hipError_t outgoing_note_open(hipStream_t s, const u32 *keys, const u32 *sealed, size_t n, u32 *plain, uint8_t *status) {
    return launch_lanes(lnote::note_kernel<2, true>, s, n, keys, sealed, n, (u32 *)nullptr, plain, status);
}
hipError_t address_partition(hipStream_t s, const u32 *points, size_t n, uint8_t *out) {
    return launch_lanes(lnote::byte_hash_kernel<2>, s, n, points, n, out);
}
hipError_t merkle_shard_index(hipStream_t s, const u32 *leaves, size_t n, uint8_t *out) {
    return launch_lanes(lnote::byte_hash_kernel<1>, s, n, leaves, n, out);
}

} // namespace mg
