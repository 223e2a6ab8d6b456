// Kernels of manta-pay's Schnorr authorization signature over ed_on_bn254: one signature per lane, wave64, canonical
// Fp<Bn254FrCfg>. The challenge is h = Blake2s-256("manta-pay/1.0.0/Schnorr-hash" | enc(pk) | enc(R) | message) as a
// little-endian integer mod l (`SchnorrHashFunction::hash`, `from_le_bytes_mod_order`); verification is the ledger's
// `auth::VerifySignature::verify` (protocol.rs:1102-1125): s G == R is refused, then s G == R + h pk decides; signing is
// s = k + sk h mod l (`Schnorr::sign`). Group law: edwards_dev.h; hash: blake2s.h; field helpers of the encoder: point_codec.h.
#include "schnorr.h"
#include "blake2s.h"
#include "edwards.h"
#include "edwards_dev.h"
#include "point_codec.h"

namespace mg {
namespace schnorr {

typedef EdBn254 E;
typedef Bn254FrCfg C;
typedef Fp<C> F;
typedef Fp<EdBn254ScalarCfg> S; // integers mod l
typedef ed::Ext<E> P;
typedef ed::Aff<F> A;
typedef ed::Niels<F> Q;
constexpr int BLOCK = 256;

// "manta-pay/1.0.0/Schnorr-hash" as little-endian words: 28 bytes, so enc(pk) starts at word 7, enc(R) at word 15, the message
// at word 23, and the first block ends after the first word of enc(R)
constexpr int TAG_WORDS = 7, HEAD_WORDS = TAG_WORDS + 16;
constexpr u32 TAG[TAG_WORDS] = {0x746e616du, 0x61702d61u, 0x2e312f79u, 0x2f302e30u, 0x6e686353u, 0x2d72726fu, 0x68736168u};

// `CanonicalSerialize` of edwards_bn254.hip encode_kernel, in registers
MG_DEV F encode(const A &p) {
    const bool ident = p.x.is_zero() && p.y == F::one();
    F x = F::from_mont(p.x);
    if (!ident && codec::is_high<C>(p.y)) x.v[7] |= 0x80000000u;
    return x;
}

// The stream of one lane for blake2s::digest: the 23 words of tag | enc(pk) | enc(R), then the lane's message row. Word J of
// block b is a head word in blocks 0 and 1 only, picked by selects over compile-time indices; a message word is loaded only if
// its first byte is inside the lane's length, and the 1 to 3 bytes of a tail word past the length are masked off, so nothing
// behind the length reaches the hash.
struct Stream {
    u32 head[HEAD_WORDS];
    const u32 *row;
    u32 len;
    template <int J> MG_DEV u32 word(u64 block) const {
        const u32 b = (u32)block;
        u32 r = 0;
        const u32 w = b * 16u + (u32)J - (u32)HEAD_WORDS; // index into the row; wraps where this is a head word
        if (b * 16u + (u32)J >= (u32)HEAD_WORDS && (u64)w * 4 < len) {
            const u32 left = len - w * 4;
            r = row[w];
            if (left < 4) r &= 0xffffffffu >> (32 - 8 * left);
        }
        r = b == 0 ? head[J] : r;
        if (J + 16 < HEAD_WORDS) r = b == 1 ? head[J + 16 < HEAD_WORDS ? J + 16 : 0] : r;
        return r;
    }
};

// v < 2^256 -> v mod l: the quotient is at most 42, six conditional subtractions of 32 l .. l (32 l < 2^256)
MG_DEV void reduce_mod_l(u32 (&v)[8]) {
    ed::sub_shifted_l_if_geq<5>(v);
    ed::sub_shifted_l_if_geq<4>(v);
    ed::sub_shifted_l_if_geq<3>(v);
    ed::sub_shifted_l_if_geq<2>(v);
    ed::sub_shifted_l_if_geq<1>(v);
    ed::sub_shifted_l_if_geq<0>(v);
}

__global__ __launch_bounds__(BLOCK) void challenge_kernel(const u32 *__restrict__ pks, const u32 *__restrict__ nonce_pts,
                                                          const u32 *__restrict__ messages, const u32 *__restrict__ lengths,
                                                          u32 stride, size_t n, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Stream s;
    const F epk = encode(A::load(pks + i * 16)), er = encode(A::load(nonce_pts + i * 16));
#pragma unroll
    for (int j = 0; j < TAG_WORDS; ++j) s.head[j] = TAG[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) s.head[TAG_WORDS + j] = epk.v[j], s.head[TAG_WORDS + 8 + j] = er.v[j];
    s.len = lengths ? lengths[i] : stride;
    s.len = s.len < stride ? s.len : stride; // the host layer refuses a longer one; a row is never read past its end
    s.row = messages + i * (size_t)(stride / 4);
    u32 h[8];
    blake2s::digest((u64)HEAD_WORDS * 4 + s.len, s, h);
    reduce_mod_l(h);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[i * 8 + j] = h[j];
}

MG_DEV bool geq_l(const u32 (&v)[8]) {
    u32 bw = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const u64 d = (u64)v[j] - E::L[j] - bw;
        bw = (u32)(d >> 63);
    }
    return bw == 0;
}

// a == (x : y) of an affine point, a projective: X = x Z and Y = y Z (Z != 0 for whatever the complete law made of curve points)
MG_DEV bool same_point(const P &a, const F &x, const F &y) { return a.X == F::mul(x, a.Z) && a.Y == F::mul(y, a.Z); }

// A = s G by the 63 gathered additions of mul_fixed_kernel, B = h pk by the double / add-always / select ladder of
// mul_pairwise_kernel, C = B + R; both comparisons projective, no inversion and no data-dependent branch: a lane that is
// already refused computes on and is masked where the status is chosen.
__global__ __launch_bounds__(BLOCK) void verify_kernel(const u32 *__restrict__ table, const u32 *__restrict__ pks,
                                                       const u32 *__restrict__ nonce_pts, const u32 *__restrict__ scalars,
                                                       const u32 *__restrict__ challenges, size_t n,
                                                       uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = scalars[i * 8 + j];
    bool bad = geq_l(k);
    P a = P::identity();
#pragma unroll 1
    for (int w = 0; w < ED_WINDOWS; ++w) {
        u32 word = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j == (w >> 3)) word = k[j];
        const u32 m = (word >> ((w & 7) * 4)) & 15u;
        a = P::madd(a, Q::load(table + (size_t)(w * 16 + m) * 24));
    }
    const A pk = A::load(pks + i * 16);
    bad = bad || codec::geq_p<C>(pk.x) || codec::geq_p<C>(pk.y) || !ed::on_curve<E>(pk);
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = challenges[i * 8 + j];
    const Q q = P::niels(pk);
    P b = P::identity();
#pragma unroll 1
    for (int t = E::L_BITS - 1; t >= 0; --t) {
        b = P::dbl(b);
        b = P::select(ed::bit_of(k, t) != 0, P::madd(b, q), b);
    }
    const A r = A::load(nonce_pts + i * 16);
    bad = bad || codec::geq_p<C>(r.x) || codec::geq_p<C>(r.y) || !ed::on_curve<E>(r);
    const P c = P::madd(b, P::niels(r));
    const bool degenerate = same_point(a, r.x, r.y);
    const bool equal = F::mul(a.X, c.Z) == F::mul(c.X, a.Z) && F::mul(a.Y, c.Z) == F::mul(c.Y, a.Z);
    status[i] = bad ? SIG_BAD_ENCODING : degenerate ? SIG_DEGENERATE : !equal ? SIG_MISMATCH : SIG_OK;
}

// s = k + sk h mod l: sk to Montgomery form mod l, one Montgomery product with the plain h, one modular addition
__global__ __launch_bounds__(BLOCK) void sign_finish_kernel(const u32 *__restrict__ keys, const u32 *__restrict__ nonces,
                                                            const u32 *__restrict__ challenges, size_t n, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const S skh = S::mul(S::to_mont(S::load(keys + i * 8)), S::load(challenges + i * 8));
    S::add(S::load(nonces + i * 8), skh).store(out + i * 8);
}

} // namespace schnorr

hipError_t schnorr_launch_bn254(const SchnorrLaunch &a) {
    if (a.n == 0) return hipSuccess;
    const dim3 grid((unsigned)((a.n + schnorr::BLOCK - 1) / schnorr::BLOCK)), blk(schnorr::BLOCK);
    switch (a.op) {
    case SchnorrLaunch::CHALLENGE:
        hipLaunchKernelGGL(schnorr::challenge_kernel, grid, blk, 0, a.stream, a.pks, a.nonce_pts, a.messages, a.lengths, a.stride,
                           a.n, a.challenges);
        break;
    case SchnorrLaunch::VERIFY:
        hipLaunchKernelGGL(schnorr::verify_kernel, grid, blk, 0, a.stream, a.table, a.pks, a.nonce_pts, a.scalars,
                           (const u32 *)a.challenges, a.n, a.status);
        break;
    case SchnorrLaunch::SIGN_FINISH:
        hipLaunchKernelGGL(schnorr::sign_finish_kernel, grid, blk, 0, a.stream, a.keys, a.scalars, (const u32 *)a.challenges, a.n,
                           a.out);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace mg
