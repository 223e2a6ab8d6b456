// AES-256-GCM (FIPS 197, NIST SP 800-38D) with a 12-byte nonce, no associated data and a 16-byte tag: the cipher of manta-pay's
// light incoming note and of its outgoing note (manta-pay/src/crypto/encryption/aes.rs `FixedNonceAesGcm`, the `aes-gcm` crate).
// One source for the kernels (light_note_bn254.hip) and for host code (mg_aes256_gcm): plain C++, no HIP header needed on the
// host. Encryption only of the block cipher: GCM never runs AES backwards.
//
// Nothing here is a table typed in by hand. The S-box is computed (the inverse in GF(2^8) as a^254, then the affine map) by a
// constexpr function; the host keeps its 256 values as a compile-time table, a kernel has each of the 256 threads of a block
// compute one entry into LDS (light_note_bn254.hip). Either is handed in as `S`: s(b) = the S-box of byte b. The round constants
// come from xtime. MixColumns works on a packed column, no T-tables.
//
// Words: the cipher's 16-byte block is four little-endian words, column c = word c, the byte of row r at bits 8 r. GHASH's
// blocks are four BIG-endian words (word 0 holds bytes 0..3), since its field puts the first bit of a block at the top; bswap
// moves between the two. All indices into round keys, state and message words are compile-time constants, so on the device the
// 60 round-key words and the message stay in registers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MG_AES_FN __host__ __device__ __forceinline__
#else
#define MG_AES_FN inline
#endif

namespace mg {
namespace aes {

constexpr uint32_t xtime8(uint32_t a) { return ((a << 1) ^ ((a >> 7) * 0x1bu)) & 0xffu; }
constexpr uint32_t gf_mul(uint32_t a, uint32_t b) { // in GF(2^8) mod x^8 + x^4 + x^3 + x + 1
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i) {
        if (b & 1) r ^= a;
        a = xtime8(a);
        b >>= 1;
    }
    return r;
}
// FIPS 197 5.1.1: the multiplicative inverse (0 -> 0) as a^254, then b ^ rotl(b, 1..4) ^ 0x63
constexpr uint32_t sbox_entry(uint32_t a) {
    const uint32_t a2 = gf_mul(a, a), a3 = gf_mul(a2, a), a6 = gf_mul(a3, a3), a7 = gf_mul(a6, a), a14 = gf_mul(a7, a7);
    const uint32_t a15 = gf_mul(a14, a), a30 = gf_mul(a15, a15), a31 = gf_mul(a30, a), a62 = gf_mul(a31, a31);
    const uint32_t a63 = gf_mul(a62, a), a126 = gf_mul(a63, a63), a127 = gf_mul(a126, a), inv = gf_mul(a127, a127);
    const uint32_t w = inv | (inv << 8);
    return (inv ^ (w >> 7) ^ (w >> 6) ^ (w >> 5) ^ (w >> 4) ^ 0x63u) & 0xffu;
}
struct SboxTable {
    uint8_t v[256];
};
constexpr SboxTable make_sbox() {
    SboxTable t{};
    for (int i = 0; i < 256; ++i) t.v[i] = (uint8_t)sbox_entry((uint32_t)i);
    return t;
}
// the host's S-box: the table above, built by the compiler
struct HostSbox {
    static constexpr SboxTable T = make_sbox();
    uint32_t operator()(uint32_t b) const { return T.v[b]; }
};
constexpr uint32_t rcon(int i) { // x^(i - 1), i = 1..7
    uint32_t r = 1;
    for (int k = 1; k < i; ++k) r = xtime8(r);
    return r;
}

MG_AES_FN uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
MG_AES_FN uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }
template <class S> MG_AES_FN uint32_t sub_word(const S &s, uint32_t w) {
    return s(w & 0xffu) | (s((w >> 8) & 0xffu) << 8) | (s((w >> 16) & 0xffu) << 16) | (s(w >> 24) << 24);
}
// one column through MixColumns: 2 b0 + 3 b1 + b2 + b3 in every byte position, on the four bytes at once
MG_AES_FN uint32_t mix_column(uint32_t w) {
    const uint32_t x = ((w & 0x7f7f7f7fu) << 1) ^ (((w >> 7) & 0x01010101u) * 0x1bu); // xtime of each byte
    const uint32_t r = rotr32(w, 8);
    return x ^ r ^ rotr32(x, 8) ^ rotr32(w, 16) ^ rotr32(w, 24);
}

constexpr int ROUNDS = 14, RK_WORDS = 4 * (ROUNDS + 1);

// FIPS 197 5.2 for Nk = 8; key = the 32 key bytes as eight little-endian words
template <int I, class S> MG_AES_FN void expand_step(const S &s, uint32_t (&rk)[RK_WORDS]) {
    uint32_t t = rk[I - 1];
    if (I % 8 == 0) t = sub_word(s, rotr32(t, 8)) ^ rcon(I / 8);
    if (I % 8 == 4) t = sub_word(s, t);
    rk[I] = rk[I - 8] ^ t;
    if constexpr (I + 1 < RK_WORDS) expand_step<I + 1>(s, rk);
}
template <class S> MG_AES_FN void expand_key(const S &s, const uint32_t (&key)[8], uint32_t (&rk)[RK_WORDS]) {
    rk[0] = key[0], rk[1] = key[1], rk[2] = key[2], rk[3] = key[3], rk[4] = key[4], rk[5] = key[5], rk[6] = key[6], rk[7] = key[7];
    expand_step<8>(s, rk);
}

// SubBytes and ShiftRows of the whole state: column c of the result takes row r from column c + r
template <class S> MG_AES_FN void sub_shift(const S &s, const uint32_t (&a)[4], uint32_t (&t)[4]) {
    t[0] = s(a[0] & 0xffu) | (s((a[1] >> 8) & 0xffu) << 8) | (s((a[2] >> 16) & 0xffu) << 16) | (s(a[3] >> 24) << 24);
    t[1] = s(a[1] & 0xffu) | (s((a[2] >> 8) & 0xffu) << 8) | (s((a[3] >> 16) & 0xffu) << 16) | (s(a[0] >> 24) << 24);
    t[2] = s(a[2] & 0xffu) | (s((a[3] >> 8) & 0xffu) << 8) | (s((a[0] >> 16) & 0xffu) << 16) | (s(a[1] >> 24) << 24);
    t[3] = s(a[3] & 0xffu) | (s((a[0] >> 8) & 0xffu) << 8) | (s((a[1] >> 16) & 0xffu) << 16) | (s(a[2] >> 24) << 24);
}
template <int R, class S> MG_AES_FN void rounds_from(const S &s, const uint32_t (&rk)[RK_WORDS], uint32_t (&a)[4]) {
    uint32_t t[4];
    sub_shift(s, a, t);
    if constexpr (R < ROUNDS) {
        a[0] = mix_column(t[0]) ^ rk[4 * R], a[1] = mix_column(t[1]) ^ rk[4 * R + 1];
        a[2] = mix_column(t[2]) ^ rk[4 * R + 2], a[3] = mix_column(t[3]) ^ rk[4 * R + 3];
        rounds_from<R + 1>(s, rk, a);
    } else {
        a[0] = t[0] ^ rk[4 * R], a[1] = t[1] ^ rk[4 * R + 1], a[2] = t[2] ^ rk[4 * R + 2], a[3] = t[3] ^ rk[4 * R + 3];
    }
}
// a <- AES_K(a)
template <class S> MG_AES_FN void encrypt_block(const S &s, const uint32_t (&rk)[RK_WORDS], uint32_t (&a)[4]) {
    a[0] ^= rk[0], a[1] ^= rk[1], a[2] ^= rk[2], a[3] ^= rk[3];
    rounds_from<1>(s, rk, a);
}

// ---- GHASH: y <- y * h in GF(2^128) as SP 800-38D 6.3 states it, shift and xor. Big-endian words: the bit of x^0 is the top bit
// of word 0, and "multiply by x" moves the block one bit to the RIGHT, folding the bit that falls off into R = 0xe1 || 0^120.
// The shift count of the inner loop is a run-time value; no array is indexed by one.
MG_AES_FN void ghash_mul(uint32_t (&y)[4], const uint32_t (&h)[4]) {
    uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0, v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
    const uint32_t x[4] = {y[0], y[1], y[2], y[3]};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const uint32_t take = 0u - ((x[w] >> b) & 1u), fold = 0u - (v3 & 1u);
            z0 ^= v0 & take, z1 ^= v1 & take, z2 ^= v2 & take, z3 ^= v3 & take;
            v3 = (v3 >> 1) | (v2 << 31), v2 = (v2 >> 1) | (v1 << 31), v1 = (v1 >> 1) | (v0 << 31);
            v0 = (v0 >> 1) ^ (0xe1000000u & fold);
        }
    }
    y[0] = z0, y[1] = z1, y[2] = z2, y[3] = z3;
}

// What one key makes: the round keys, the hash key H = AES_K(0^128) and AES_K(J0), J0 = nonce | 00 00 00 01
struct Gcm {
    uint32_t rk[RK_WORDS];
    uint32_t h[4];     // big-endian words
    uint32_t ej0[4];   // big-endian words
    uint32_t nonce[3]; // little-endian words, as the cipher reads them
    uint32_t y[4];     // the running GHASH
};
template <class S> MG_AES_FN void gcm_init(const S &s, const uint32_t (&key)[8], const uint32_t (&nonce)[3], Gcm &g) {
    expand_key(s, key, g.rk);
    uint32_t a[4] = {0, 0, 0, 0};
    encrypt_block(s, g.rk, a);
    g.h[0] = bswap(a[0]), g.h[1] = bswap(a[1]), g.h[2] = bswap(a[2]), g.h[3] = bswap(a[3]);
    g.nonce[0] = nonce[0], g.nonce[1] = nonce[1], g.nonce[2] = nonce[2];
    a[0] = nonce[0], a[1] = nonce[1], a[2] = nonce[2], a[3] = bswap(1u);
    encrypt_block(s, g.rk, a);
    g.ej0[0] = bswap(a[0]), g.ej0[1] = bswap(a[1]), g.ej0[2] = bswap(a[2]), g.ej0[3] = bswap(a[3]);
    g.y[0] = g.y[1] = g.y[2] = g.y[3] = 0;
}
// AES_K(nonce | be32(counter)) as little-endian words: block b of the message uses counter b + 2
template <class S> MG_AES_FN void keystream(const S &s, const Gcm &g, uint32_t counter, uint32_t (&ks)[4]) {
    ks[0] = g.nonce[0], ks[1] = g.nonce[1], ks[2] = g.nonce[2], ks[3] = bswap(counter);
    encrypt_block(s, g.rk, ks);
}
// one 16-byte block of CIPHERTEXT (little-endian words; a short last block padded with zeros) into the hash
MG_AES_FN void absorb(Gcm &g, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    g.y[0] ^= bswap(c0), g.y[1] ^= bswap(c1), g.y[2] ^= bswap(c2), g.y[3] ^= bswap(c3);
    ghash_mul(g.y, g.h);
}
// the length block 0^64 | be64(8 len), then the tag as little-endian words (= its 16 bytes in memory order)
MG_AES_FN void finish(Gcm &g, uint64_t len, uint32_t (&tag)[4]) {
    g.y[2] ^= (uint32_t)((len * 8) >> 32), g.y[3] ^= (uint32_t)(len * 8);
    ghash_mul(g.y, g.h);
    tag[0] = bswap(g.y[0] ^ g.ej0[0]), tag[1] = bswap(g.y[1] ^ g.ej0[1]);
    tag[2] = bswap(g.y[2] ^ g.ej0[2]), tag[3] = bswap(g.y[3] ^ g.ej0[3]);
}

// A message of exactly BLOCKS 16-byte blocks, in place on little-endian words: `data` goes from plaintext to ciphertext, or
// with DECRYPT the other way; `tag` is the tag of the CIPHERTEXT either way (the caller compares it when opening). This is what
// a kernel runs (BLOCKS = 5 for the light note, 3 for the outgoing note), and what mg_aes256_gcm runs for those two lengths.
template <int B, int BLOCKS, bool DECRYPT, class S> MG_AES_FN void crypt_from(const S &s, Gcm &g, uint32_t (&data)[4 * BLOCKS]) {
    uint32_t ks[4];
    keystream(s, g, (uint32_t)B + 2u, ks);
    if (DECRYPT) absorb(g, data[4 * B], data[4 * B + 1], data[4 * B + 2], data[4 * B + 3]);
    data[4 * B] ^= ks[0], data[4 * B + 1] ^= ks[1], data[4 * B + 2] ^= ks[2], data[4 * B + 3] ^= ks[3];
    if (!DECRYPT) absorb(g, data[4 * B], data[4 * B + 1], data[4 * B + 2], data[4 * B + 3]);
    if constexpr (B + 1 < BLOCKS) crypt_from<B + 1, BLOCKS, DECRYPT>(s, g, data);
}
template <int BLOCKS, bool DECRYPT, class S>
MG_AES_FN void crypt_blocks(const S &s, const uint32_t (&key)[8], const uint32_t (&nonce)[3], uint32_t (&data)[4 * BLOCKS],
                            uint32_t (&tag)[4]) {
    Gcm g;
    gcm_init(s, key, nonce, g);
    crypt_from<0, BLOCKS, DECRYPT>(s, g, data);
    finish(g, 16u * BLOCKS, tag);
}

// ---- host: any length, bytes in memory -----------------------------------------------------------------------------------
inline uint32_t load_le(const uint8_t *p, size_t avail) { // up to four bytes, the missing ones zero
    uint32_t r = 0;
    for (size_t k = 0; k < 4 && k < avail; ++k) r |= (uint32_t)p[k] << (8 * k);
    return r;
}
inline void store_le(uint8_t *p, uint32_t w, size_t room) {
    for (size_t k = 0; k < 4 && k < room; ++k) p[k] = (uint8_t)(w >> (8 * k));
}
template <int BLOCKS> inline void crypt_whole(const uint32_t (&key)[8], const uint32_t (&nonce)[3], const uint8_t *in, bool decrypt,
                                              uint8_t *out, uint32_t (&tag)[4]) {
    uint32_t d[4 * BLOCKS];
    for (int j = 0; j < 4 * BLOCKS; ++j) d[j] = load_le(in + 4 * j, 4);
    if (decrypt) crypt_blocks<BLOCKS, true>(HostSbox(), key, nonce, d, tag);
    else crypt_blocks<BLOCKS, false>(HostSbox(), key, nonce, d, tag);
    for (int j = 0; j < 4 * BLOCKS; ++j) store_le(out + 4 * j, d[j], 4);
}
// `len` message bytes from `in` to `out` (which may be `in`), and the tag of the ciphertext. Messages of 48 and 80 bytes go
// through crypt_blocks<3> / <5>, the instantiations of the kernels; every other length through the block loop below.
inline void crypt(const uint8_t key[32], const uint8_t nonce[12], const uint8_t *in, size_t len, bool decrypt, uint8_t *out,
                  uint8_t tag_out[16]) {
    uint32_t k[8], nn[3], tag[4];
    for (int j = 0; j < 8; ++j) k[j] = load_le(key + 4 * j, 4);
    for (int j = 0; j < 3; ++j) nn[j] = load_le(nonce + 4 * j, 4);
    if (len == 48) crypt_whole<3>(k, nn, in, decrypt, out, tag);
    else if (len == 80) crypt_whole<5>(k, nn, in, decrypt, out, tag);
    else {
        const HostSbox s;
        Gcm g;
        gcm_init(s, k, nn, g);
        for (size_t off = 0, b = 0; off < len; off += 16, ++b) {
            const size_t m = len - off < 16 ? len - off : 16;
            uint32_t ks[4], c[4];
            keystream(s, g, (uint32_t)b + 2u, ks);
            for (int j = 0; j < 4; ++j) {
                const size_t have = m > 4 * (size_t)j ? m - 4 * j : 0;
                const uint32_t w = load_le(in + off + 4 * j, have), x = w ^ ks[j];
                const uint32_t keep = have >= 4 ? 0xffffffffu : have ? (1u << (8 * have)) - 1u : 0u; // the keystream past the end
                c[j] = (decrypt ? w : x) & keep;                                                     // never reaches the hash
                store_le(out + off + 4 * j, x, have);
            }
            absorb(g, c[0], c[1], c[2], c[3]);
        }
        finish(g, len, tag);
    }
    for (int j = 0; j < 4; ++j) store_le(tag_out + 4 * j, tag[j], 4);
}

} // namespace aes
} // namespace mg
