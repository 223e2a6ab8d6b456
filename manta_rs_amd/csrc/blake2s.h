// Blake2s (RFC 7693), unkeyed, no salt, no personalisation: with the 32-byte digest the hash of manta-pay's Schnorr challenge
// (manta-pay/src/config/utxo.rs `SchnorrHashFunction`: `Blake2s256::new()`, updates, `finalize`) and of its AES note keys, with a
// one-byte digest (`Blake2sVar::new(1)`) its address partition and Merkle shard functions. The digest length is part of the
// parameter word, so a shorter digest is another hash and not a prefix of the longer one. One source for the kernels
// (schnorr_bn254.hip, light_note_bn254.hip) and for host code (mg_blake2s256, mg_blake2s): plain C++, no HIP header needed on the
// host.
//
// The stream is presented as 32-bit little-endian words: a source `W` answers `w.template word<J>(b)` = word J of block b,
// with the bytes past the end of the stream zero. J is a template argument, so the sixteen message words of a block are
// sixteen named registers, and the ten rounds below index them through the constexpr permutation table only: nothing here
// indexes m[] with a run-time value, which on the device would move the block to scratch memory.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <utility>

#if defined(__HIPCC__)
#define MG_B2S_FN __host__ __device__ __forceinline__
#else
#define MG_B2S_FN inline
#endif

namespace mg {
namespace blake2s {

// h0 of an unkeyed digest of k bytes = IV[0] ^ 0x01010000 ^ k (fanout 1, depth 1, no key, digest length k)
constexpr uint32_t IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
constexpr int SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

MG_B2S_FN uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

MG_B2S_FN void g(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t x, uint32_t y) {
    a = a + b + x;
    d = rotr(d ^ a, 16);
    c = c + d;
    b = rotr(b ^ c, 12);
    a = a + b + y;
    d = rotr(d ^ a, 8);
    c = c + d;
    b = rotr(b ^ c, 7);
}

template <int R> MG_B2S_FN void round(uint32_t (&v)[16], const uint32_t (&m)[16]) {
    g(v[0], v[4], v[8], v[12], m[SIGMA[R][0]], m[SIGMA[R][1]]);
    g(v[1], v[5], v[9], v[13], m[SIGMA[R][2]], m[SIGMA[R][3]]);
    g(v[2], v[6], v[10], v[14], m[SIGMA[R][4]], m[SIGMA[R][5]]);
    g(v[3], v[7], v[11], v[15], m[SIGMA[R][6]], m[SIGMA[R][7]]);
    g(v[0], v[5], v[10], v[15], m[SIGMA[R][8]], m[SIGMA[R][9]]);
    g(v[1], v[6], v[11], v[12], m[SIGMA[R][10]], m[SIGMA[R][11]]);
    g(v[2], v[7], v[8], v[13], m[SIGMA[R][12]], m[SIGMA[R][13]]);
    g(v[3], v[4], v[9], v[14], m[SIGMA[R][14]], m[SIGMA[R][15]]);
}

MG_B2S_FN void init(uint32_t (&h)[8], uint32_t out_len = 32) {
    h[0] = IV[0] ^ 0x01010000u ^ out_len;
    h[1] = IV[1], h[2] = IV[2], h[3] = IV[3], h[4] = IV[4], h[5] = IV[5], h[6] = IV[6], h[7] = IV[7];
}

// F of RFC 7693 3.2: t = the bytes of the stream up to and including this block, last = this is the final block
MG_B2S_FN void compress(uint32_t (&h)[8], const uint32_t (&m)[16], uint64_t t, bool last) {
    uint32_t v[16] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], IV[0], IV[1], IV[2], IV[3],
                      IV[4] ^ (uint32_t)t, IV[5] ^ (uint32_t)(t >> 32), last ? ~IV[6] : IV[6], IV[7]};
    round<0>(v, m), round<1>(v, m), round<2>(v, m), round<3>(v, m), round<4>(v, m);
    round<5>(v, m), round<6>(v, m), round<7>(v, m), round<8>(v, m), round<9>(v, m);
    h[0] ^= v[0] ^ v[8], h[1] ^= v[1] ^ v[9], h[2] ^= v[2] ^ v[10], h[3] ^= v[3] ^ v[11];
    h[4] ^= v[4] ^ v[12], h[5] ^= v[5] ^ v[13], h[6] ^= v[6] ^ v[14], h[7] ^= v[7] ^ v[15];
}

template <class W, int... J> MG_B2S_FN void fill(uint32_t (&m)[16], const W &w, uint64_t b, std::integer_sequence<int, J...>) {
    ((m[J] = w.template word<J>(b)), ...);
}

// The digest of a stream of `total` bytes as eight words (byte 4 i of the digest = the low byte of out[i]; a digest of
// out_len < 32 bytes is the first out_len of these). The final block is
// the last one that holds a byte of the stream -- a stream of a non-zero multiple of 64 bytes finalises its last full block,
// there is no extra empty one -- and the empty stream is one zero block with t = 0.
template <class W> MG_B2S_FN void digest(uint64_t total, const W &w, uint32_t (&out)[8], uint32_t out_len = 32) {
    init(out, out_len);
    const uint64_t blocks = total ? (total + 63) / 64 : 1;
    for (uint64_t b = 0; b < blocks; ++b) {
        uint32_t m[16];
        fill(m, w, b, std::make_integer_sequence<int, 16>());
        const bool last = b + 1 == blocks;
        compress(out, m, last ? total : 64 * (b + 1), last);
    }
}

// a stream that is `len` bytes in memory
struct Bytes {
    const uint8_t *data;
    uint64_t len;
    template <int J> MG_B2S_FN uint32_t word(uint64_t b) const {
        const uint64_t off = 64 * b + 4 * J;
        uint32_t r = 0;
        for (uint64_t k = off; k < off + 4 && k < len; ++k) r |= (uint32_t)data[k] << (8 * (k - off));
        return r;
    }
};

inline void hash(const uint8_t *data, size_t len, uint8_t *out, size_t out_len = 32) { // out_len in 1..32
    uint32_t h[8];
    digest(len, Bytes{data, len}, h, (uint32_t)out_len);
    for (size_t i = 0; i < out_len; ++i) out[i] = (uint8_t)(h[i >> 2] >> (8 * (i & 3)));
}

} // namespace blake2s
} // namespace mg
