// Kernels of the embedded curve of BN254 (ed_on_bn254) and of manta-pay's Poseidon note encryption: one point / note per lane,
// wave64. The scalar of MUL_SHARED and the bits of l are the same for every lane, so those ladders branch uniformly; per-lane
// scalars select instead of branching (MUL_PAIRWISE) or index a table (MUL_FIXED). Group law, square root, the per-lane scalar
// products and the encoder: edwards_dev.h; permutation: poseidon.h; field helpers of the codec (canonical comparison, sign):
// point_codec.h. Behind each kernel, its launch function (edwards.h).
#include "edwards.h"
#include "edwards_dev.h"
#include "poseidon.h"

namespace mg {
namespace ed {

typedef EdBn254 E;
typedef Bn254FrCfg C;
typedef Fp<C> F;
typedef Ext<E> P;

// ark-ec 0.3 `GroupAffine<P: TEModelParameters>: CanonicalDeserialize`: x little-endian with `EdwardsFlags` in bit 255 (set iff
// y > -y); x = 0 is the identity whatever the flag; otherwise `get_point_from_x`: y^2 = (a x^2 - 1) / (d x^2 - 1) (d x^2 != 1: d
// is a non-square), the root picked by the flag, then the subgroup test. Rejected points come back as zeros.
__global__ __launch_bounds__(LANE_BLOCK) void decode_kernel(const u32 *__restrict__ in, size_t n, int checked,
                                                            u32 *__restrict__ out, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F x = F::load(in + i * 8);
    const bool greatest = (x.v[7] >> 31) != 0;
    x.v[7] &= 0x7fffffffu;
    const bool bad = codec::geq_p<C>(x); // bit 254 is part of x: any value with it set is >= p
    const bool zero = x.is_zero();
    x = F::to_mont(x);
    const F x2 = F::sqr(x), one = F::one();
    const F y2 = F::mul(F::sub(x2, one), F::inv(F::sub(F::mul(Curve<E>::d(), x2), one)));
    F r;
    const bool on = fsqrt<E>(y2, r);
    const F y = F::select(codec::is_high<C>(r) != greatest, F::neg(r), r);
    bool in_group = true;
    if (checked) in_group = times_l_is_identity<E>(Aff<F>{x, y});
    const uint8_t st = bad ? PT_BAD_ENCODING : zero ? PT_OK : !on ? PT_NOT_ON_CURVE : !in_group ? PT_NOT_IN_SUBGROUP : PT_OK;
    const bool keep = st == PT_OK;
    const F z = F::zero();
    F::select(keep, x, z).store(out + i * 16);
    F::select(keep, zero ? one : y, z).store(out + i * 16 + 8);
    status[i] = st;
}

__global__ __launch_bounds__(LANE_BLOCK) void check_kernel(const u32 *__restrict__ aff, size_t n, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Aff<F> p = Aff<F>::load(aff + i * 16);
    const uint8_t st = point_status<E>(p);
    const bool in_group = times_l_is_identity<E>(p);
    status[i] = st != PT_OK ? st : !in_group ? PT_NOT_IN_SUBGROUP : PT_OK;
}

__global__ __launch_bounds__(LANE_BLOCK) void encode_kernel(const u32 *__restrict__ aff, size_t n, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    encode<E>(Aff<F>::load(aff + i * 16)).store(out + i * 8);
}

// n points x one scalar (key agreement `epk * vk`): plain double-and-add from the scalar's top bit; the bit is wave-uniform
__global__ __launch_bounds__(LANE_BLOCK) void mul_shared_kernel(const u32 *__restrict__ pts, size_t n, const u32 *__restrict__ k,
                                                                int top, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Niels<F> q = P::niels(Aff<F>::load(pts + i * 16));
    P acc = P::identity();
#pragma unroll 1
    for (int b = top; b >= 0; --b) {
        acc = P::dbl(acc);
        if ((k[b >> 5] >> (b & 31)) & 1u) acc = P::madd(acc, q);
    }
    acc.to_affine().store(out + i * 16);
}

// n scalars x one base, from the base's table
__global__ __launch_bounds__(LANE_BLOCK) void mul_fixed_kernel(const u32 *__restrict__ table, const u32 *__restrict__ sc, size_t n,
                                                               u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = sc[i * 8 + j];
    mul_fixed<E>(table, k).to_affine().store(out + i * 16);
}

// n scalars x n points
__global__ __launch_bounds__(LANE_BLOCK) void mul_pairwise_kernel(const u32 *__restrict__ pts, const u32 *__restrict__ sc, size_t n,
                                                                  u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = sc[i * 8 + j];
    mul_select<E>(k, P::niels(Aff<F>::load(pts + i * 16))).to_affine().store(out + i * 16);
}

__global__ __launch_bounds__(LANE_BLOCK) void add_kernel(const u32 *__restrict__ a, const u32 *__restrict__ b, size_t n,
                                                         u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    P::madd(P::from_affine(Aff<F>::load(a + i * 16)), P::niels(Aff<F>::load(b + i * 16))).to_affine().store(out + i * 16);
}

// `FixedDuplexer<1, Poseidon3>` (manta-pay/src/crypto/poseidon/encryption.rs, manta-crypto/src/permutation/duplex.rs): state <-
// initial state; setup blocks (x, y, 0) of the key and (0, 0, 0) of the empty header (`padded_chunks_with` emits its remainder
// chunk even when empty), each added to words 1..3 and followed by the permutation (`Sponge::absorb` = write, permute); then the
// message block: encryption adds the plaintext and reads the ciphertext off words 1..3, decryption subtracts words 1..3 from the
// ciphertext and overwrites them with it; one more permutation; tag = word 1. Decryption reports a tag mismatch, or a value
// word (plaintext word 2) of 2^128 or more (`try_into_u128`, config/utxo.rs:716-731), and returns zeros for such a note.
template <bool DECRYPT>
__global__ __launch_bounds__(LANE_BLOCK) void sponge_kernel(const u32 *__restrict__ prm, const u32 *__restrict__ keys,
                                                            const u32 *__restrict__ blocks, const u32 *__restrict__ tags, size_t n,
                                                            u32 *__restrict__ out, u32 *__restrict__ tag_out,
                                                            uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int HF = ED_CIPHER_FULL / 2, PART = ED_CIPHER_PARTIAL;
    const u32 *init = prm + (size_t)((ED_CIPHER_FULL + ED_CIPHER_PARTIAL) * 4 + 16) * 8;
    F st[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = F::load(init + j * 8);
    st[1] = F::add(st[1], F::load(keys + i * 16));
    st[2] = F::add(st[2], F::load(keys + i * 16 + 8));
#pragma unroll 1
    for (int s = 0; s < 2; ++s) pos::permute<C, 4>(st, prm, HF, PART); // the key block, then the header's zero block
    F m[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const F blk = F::load(blocks + (i * 3 + j) * 8);
        if (DECRYPT) {
            m[j] = F::sub(blk, st[j + 1]);
            st[j + 1] = blk;
        } else {
            st[j + 1] = F::add(st[j + 1], blk);
            m[j] = st[j + 1];
        }
    }
    pos::permute<C, 4>(st, prm, HF, PART);
    if (DECRYPT) {
        const bool small = fits_u128(m[2]);
        const uint8_t s = !(st[1] == F::load(tags + i * 8)) ? NOTE_BAD_TAG : !small ? NOTE_BAD_VALUE : NOTE_OK;
        const F z = F::zero();
#pragma unroll
        for (int j = 0; j < 3; ++j) F::select(s == NOTE_OK, m[j], z).store(out + (i * 3 + j) * 8);
        status[i] = s;
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) m[j].store(out + (i * 3 + j) * 8);
        st[1].store(tag_out + i * 8);
    }
}

} // namespace ed

hipError_t ed_decode(hipStream_t s, const u32 *encodings, size_t n, bool checked, u32 *points, uint8_t *status) {
    return launch_lanes(ed::decode_kernel, s, n, encodings, n, (int)checked, points, status);
}
hipError_t ed_check(hipStream_t s, const u32 *points, size_t n, uint8_t *status) {
    return launch_lanes(ed::check_kernel, s, n, points, n, status);
}
hipError_t ed_encode(hipStream_t s, const u32 *points, size_t n, u32 *encodings) {
    return launch_lanes(ed::encode_kernel, s, n, points, n, encodings);
}
hipError_t ed_mul_shared(hipStream_t s, const u32 *points, size_t n, const u32 *scalar, int top, u32 *out) {
    return launch_lanes(ed::mul_shared_kernel, s, n, points, n, scalar, top, out);
}
hipError_t ed_mul_fixed(hipStream_t s, const u32 *table, const u32 *scalars, size_t n, u32 *out) {
    return launch_lanes(ed::mul_fixed_kernel, s, n, table, scalars, n, out);
}
hipError_t ed_mul_pairwise(hipStream_t s, const u32 *points, const u32 *scalars, size_t n, u32 *out) {
    return launch_lanes(ed::mul_pairwise_kernel, s, n, points, scalars, n, out);
}
hipError_t ed_add(hipStream_t s, const u32 *a, const u32 *b, size_t n, u32 *out) {
    return launch_lanes(ed::add_kernel, s, n, a, b, n, out);
}
hipError_t ed_encrypt(hipStream_t s, const u32 *prm, const u32 *keys, const u32 *plain, size_t n, u32 *cipher_out, u32 *tag_out) {
    return launch_lanes(ed::sponge_kernel<false>, s, n, prm, keys, plain, nullptr, n, cipher_out, tag_out, nullptr);
}
hipError_t ed_decrypt(hipStream_t s, const u32 *prm, const u32 *keys, const u32 *blocks, const u32 *tags, size_t n, u32 *plain_out,
                      uint8_t *status) {
    return launch_lanes(ed::sponge_kernel<true>, s, n, prm, keys, blocks, tags, n, plain_out, nullptr, status);
}

} // namespace mg
