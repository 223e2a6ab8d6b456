// Kernels of the embedded curve of BN254 (ed_on_bn254) and of manta-pay's Poseidon note encryption: one point / note per lane,
// wave64. The scalar of MUL_SHARED and the bits of l are the same for every lane, so those ladders branch uniformly; per-lane
// scalars select instead of branching (MUL_PAIRWISE) or index a table (MUL_FIXED). Group law and square root: edwards_dev.h;
// permutation: poseidon.h; field helpers of the codec (canonical comparison, sign): point_codec.h.
#include "edwards.h"
#include "edwards_dev.h"
#include "point_codec.h"
#include "poseidon.h"

namespace mg {
namespace ed {

typedef EdBn254 E;
typedef Bn254FrCfg C;
typedef Fp<C> F;
typedef Ext<E> P;
constexpr int BLOCK = 256;

// ark-ec 0.3 `GroupAffine<P: TEModelParameters>: CanonicalDeserialize`: x little-endian with `EdwardsFlags` in bit 255 (set iff
// y > -y); x = 0 is the identity whatever the flag; otherwise `get_point_from_x`: y^2 = (a x^2 - 1) / (d x^2 - 1) (d x^2 != 1: d
// is a non-square), the root picked by the flag, then the subgroup test. Rejected points come back as zeros.
__global__ __launch_bounds__(BLOCK) void decode_kernel(const u32 *__restrict__ in, size_t n, int checked, u32 *__restrict__ out,
                                                       uint8_t *__restrict__ status) {
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

__global__ __launch_bounds__(BLOCK) void check_kernel(const u32 *__restrict__ aff, size_t n, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Aff<F> p = Aff<F>::load(aff + i * 16);
    const bool bad = codec::geq_p<C>(p.x) || codec::geq_p<C>(p.y);
    const bool on = on_curve<E>(p);
    const bool in_group = times_l_is_identity<E>(p);
    status[i] = bad ? PT_BAD_ENCODING : !on ? PT_NOT_ON_CURVE : !in_group ? PT_NOT_IN_SUBGROUP : PT_OK;
}

// `CanonicalSerialize`: the identity (0, 1) is 32 zero bytes; any other point is x with bit 255 = (y > -y)
__global__ __launch_bounds__(BLOCK) void encode_kernel(const u32 *__restrict__ aff, size_t n, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Aff<F> p = Aff<F>::load(aff + i * 16);
    const bool ident = p.x.is_zero() && p.y == F::one();
    F x = F::from_mont(p.x);
    if (!ident && codec::is_high<C>(p.y)) x.v[7] |= 0x80000000u;
    x.store(out + i * 8);
}

// n points x one scalar (key agreement `epk * vk`): plain double-and-add from the scalar's top bit; the bit is wave-uniform
__global__ __launch_bounds__(BLOCK) void mul_shared_kernel(const u32 *__restrict__ pts, size_t n, const u32 *__restrict__ k, int top,
                                                           u32 *__restrict__ out) {
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

// n scalars x one base: 63 gathered additions, no doubling (table: edwards.h)
__global__ __launch_bounds__(BLOCK) void mul_fixed_kernel(const u32 *__restrict__ table, const u32 *__restrict__ sc, size_t n,
                                                          u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = sc[i * 8 + j];
    P acc = P::identity();
#pragma unroll 1
    for (int w = 0; w < ED_WINDOWS; ++w) {
        u32 word = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j == (w >> 3)) word = k[j];
        const u32 m = (word >> ((w & 7) * 4)) & 15u;
        acc = P::madd(acc, Niels<F>::load(table + (size_t)(w * 16 + m) * 24));
    }
    acc.to_affine().store(out + i * 16);
}

// n scalars x n points: double, add always, keep the sum where the lane's bit is set
__global__ __launch_bounds__(BLOCK) void mul_pairwise_kernel(const u32 *__restrict__ pts, const u32 *__restrict__ sc, size_t n,
                                                             u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = sc[i * 8 + j];
    const Niels<F> q = P::niels(Aff<F>::load(pts + i * 16));
    P acc = P::identity();
#pragma unroll 1
    for (int b = E::L_BITS - 1; b >= 0; --b) {
        acc = P::dbl(acc);
        acc = P::select(bit_of(k, b) != 0, P::madd(acc, q), acc);
    }
    acc.to_affine().store(out + i * 16);
}

__global__ __launch_bounds__(BLOCK) void add_kernel(const u32 *__restrict__ a, const u32 *__restrict__ b, size_t n,
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
__global__ __launch_bounds__(BLOCK) void sponge_kernel(const u32 *__restrict__ prm, const u32 *__restrict__ keys,
                                                       const u32 *__restrict__ blocks, const u32 *__restrict__ tags, size_t n,
                                                       u32 *__restrict__ out, u32 *__restrict__ tag_out, uint8_t *__restrict__ status) {
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
        const F v = F::from_mont(m[2]);
        const bool small = (v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0;
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

hipError_t edwards_launch_bn254(const EdwardsLaunch &a) {
    if (a.n == 0) return hipSuccess;
    const dim3 grid((unsigned)((a.n + ed::BLOCK - 1) / ed::BLOCK)), blk(ed::BLOCK);
    switch (a.op) {
    case EdwardsLaunch::DECODE:
        hipLaunchKernelGGL(ed::decode_kernel, grid, blk, 0, a.stream, a.a, a.n, a.checked, a.out, a.status);
        break;
    case EdwardsLaunch::CHECK: hipLaunchKernelGGL(ed::check_kernel, grid, blk, 0, a.stream, a.a, a.n, a.status); break;
    case EdwardsLaunch::ENCODE: hipLaunchKernelGGL(ed::encode_kernel, grid, blk, 0, a.stream, a.a, a.n, a.out); break;
    case EdwardsLaunch::MUL_SHARED:
        hipLaunchKernelGGL(ed::mul_shared_kernel, grid, blk, 0, a.stream, a.a, a.n, a.consts, a.top, a.out);
        break;
    case EdwardsLaunch::MUL_FIXED:
        hipLaunchKernelGGL(ed::mul_fixed_kernel, grid, blk, 0, a.stream, a.consts, a.b, a.n, a.out);
        break;
    case EdwardsLaunch::MUL_PAIRWISE:
        hipLaunchKernelGGL(ed::mul_pairwise_kernel, grid, blk, 0, a.stream, a.a, a.b, a.n, a.out);
        break;
    case EdwardsLaunch::ADD: hipLaunchKernelGGL(ed::add_kernel, grid, blk, 0, a.stream, a.a, a.b, a.n, a.out); break;
    case EdwardsLaunch::ENCRYPT:
        hipLaunchKernelGGL(ed::sponge_kernel<false>, grid, blk, 0, a.stream, a.consts, a.a, a.b, (const u32 *)nullptr, a.n, a.out,
                           a.out2, (uint8_t *)nullptr);
        break;
    case EdwardsLaunch::DECRYPT:
        hipLaunchKernelGGL(ed::sponge_kernel<true>, grid, blk, 0, a.stream, a.consts, a.a, a.b, a.c, a.n, a.out, (u32 *)nullptr,
                           a.status);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace mg
