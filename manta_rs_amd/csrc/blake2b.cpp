// Blake2b-512 (RFC 7693), unkeyed, no salt, no personalisation, host code: the hash of Perpetual Powers of Tau files -- the
// 64-byte header of a challenge / response is the digest of the file it answers, and a contribution's response is the digest
// of accumulator | challenge | proof (manta-trusted-setup/src/groth16/ppot/kzg.rs:85-118, `BlakeHasher` = `Blake2b::default()`).
// Written from the RFC: 128-byte blocks through 12 rounds of the G function on a 4 x 4 state of 64-bit words (rotations 32, 24,
// 16, 63), message words chosen by the ten SIGMA permutations (rounds 10 and 11 reuse 0 and 1), a 128-bit byte counter of which
// the low 64 bits suffice for any buffer in memory, the last block flagged by inverting v[14]. Little-endian words.
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mg {
namespace {

const uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                        0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
const uint8_t SIGMA[10][16] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
                               {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
                               {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
                               {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
                               {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

inline uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
inline void g(uint64_t *v, int a, int b, int c, int d, uint64_t x, uint64_t y) {
    v[a] = v[a] + v[b] + x;
    v[d] = rotr(v[d] ^ v[a], 32);
    v[c] = v[c] + v[d];
    v[b] = rotr(v[b] ^ v[c], 24);
    v[a] = v[a] + v[b] + y;
    v[d] = rotr(v[d] ^ v[a], 16);
    v[c] = v[c] + v[d];
    v[b] = rotr(v[b] ^ v[c], 63);
}
// h <- F(h, block, t, last): t = bytes hashed so far, this block's included
void compress(uint64_t h[8], const uint8_t block[128], uint64_t t, bool last) {
    uint64_t m[16], v[16];
    for (int i = 0; i < 16; ++i) {
        m[i] = 0;
        for (int j = 7; j >= 0; --j) m[i] = (m[i] << 8) | block[8 * i + j];
    }
    for (int i = 0; i < 8; ++i) v[i] = h[i], v[i + 8] = IV[i];
    v[12] ^= t; // the counter's high word stays 0: no buffer in memory has 2^64 bytes
    if (last) v[14] = ~v[14];
    for (int r = 0; r < 12; ++r) {
        const uint8_t *s = SIGMA[r % 10];
        g(v, 0, 4, 8, 12, m[s[0]], m[s[1]]);
        g(v, 1, 5, 9, 13, m[s[2]], m[s[3]]);
        g(v, 2, 6, 10, 14, m[s[4]], m[s[5]]);
        g(v, 3, 7, 11, 15, m[s[6]], m[s[7]]);
        g(v, 0, 5, 10, 15, m[s[8]], m[s[9]]);
        g(v, 1, 6, 11, 12, m[s[10]], m[s[11]]);
        g(v, 2, 7, 8, 13, m[s[12]], m[s[13]]);
        g(v, 3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}

} // namespace

void blake2b512(const uint8_t *data, size_t len, uint8_t out[64]) {
    uint64_t h[8];
    for (int i = 0; i < 8; ++i) h[i] = IV[i];
    h[0] ^= 0x01010000ull ^ 64; // parameter block: digest length 64, no key, fanout 1, depth 1
    size_t off = 0;
    while (len - off > 128) { // every block but the last; a message that ends on a block boundary keeps that block for last
        compress(h, data + off, (uint64_t)off + 128, false);
        off += 128;
    }
    uint8_t tail[128] = {0};
    if (len - off) std::memcpy(tail, data + off, len - off);
    compress(h, tail, (uint64_t)len, true);
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) out[8 * i + j] = (uint8_t)(h[i] >> (8 * j));
}

} // namespace mg
