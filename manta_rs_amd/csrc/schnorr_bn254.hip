// Kernels of manta-pay's Schnorr authorization signature over ed_on_bn254: one signature per lane, wave64, canonical
// Fp<Bn254FrCfg>. The challenge is h = Blake2s-256("manta-pay/1.0.0/Schnorr-hash" | enc(pk) | enc(R) | message) as a
// little-endian integer mod l (`SchnorrHashFunction::hash`, `from_le_bytes_mod_order`); verification is the ledger's
// `auth::VerifySignature::verify` (protocol.rs:1102-1125): s G == R is refused, then s G == R + h pk decides; signing is
// s = k + sk h mod l (`Schnorr::sign`). Group law, encoder and the two scalar products: edwards_dev.h; hash: blake2s.h. Behind
// each kernel, its launch function (schnorr.h).
#include "schnorr.h"
#include "blake2s.h"
#include "edwards_dev.h"

namespace mg {
namespace schnorr {

typedef EdBn254 E;
typedef Bn254FrCfg C;
typedef Fp<C> F;
typedef Fp<EdBn254ScalarCfg> S; // integers mod l
typedef ed::Ext<E> P;
typedef ed::Aff<F> A;

// "manta-pay/1.0.0/Schnorr-hash" as little-endian words: 28 bytes, so enc(pk) starts at word 7, enc(R) at word 15, the message
// at word 23, and the first block ends after the first word of enc(R)
constexpr int TAG_WORDS = 7, HEAD_WORDS = TAG_WORDS + 16;
constexpr u32 TAG[TAG_WORDS] = {0x746e616du, 0x61702d61u, 0x2e312f79u, 0x2f302e30u, 0x6e686353u, 0x2d72726fu, 0x68736168u};

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

__global__ __launch_bounds__(LANE_BLOCK) void challenge_kernel(const u32 *__restrict__ pks, const u32 *__restrict__ nonce_pts,
                                                               const u32 *__restrict__ messages, const u32 *__restrict__ lengths,
                                                               u32 stride, size_t n, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Stream s;
    const F epk = ed::encode<E>(A::load(pks + i * 16)), er = ed::encode<E>(A::load(nonce_pts + i * 16));
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

// A = s G from the generator's table, B = h pk by the select ladder, C = B + R; both comparisons projective, no inversion and no
// data-dependent branch: a lane that is already refused computes on and is masked where the status is chosen.
__global__ __launch_bounds__(LANE_BLOCK) void verify_kernel(const u32 *__restrict__ table, const u32 *__restrict__ pks,
                                                            const u32 *__restrict__ nonce_pts, const u32 *__restrict__ scalars,
                                                            const u32 *__restrict__ challenges, size_t n,
                                                            uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = scalars[i * 8 + j];
    bool bad = geq_l(k);
    const P a = ed::mul_fixed<E>(table, k);
    const A pk = A::load(pks + i * 16);
    bad = bad || ed::point_status<E>(pk) != PT_OK;
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = challenges[i * 8 + j];
    const P b = ed::mul_select<E>(k, P::niels(pk));
    const A r = A::load(nonce_pts + i * 16);
    bad = bad || ed::point_status<E>(r) != PT_OK;
    const P c = P::madd(b, P::niels(r));
    const bool degenerate = same_point(a, r.x, r.y);
    const bool equal = F::mul(a.X, c.Z) == F::mul(c.X, a.Z) && F::mul(a.Y, c.Z) == F::mul(c.Y, a.Z);
    status[i] = bad ? SIG_BAD_ENCODING : degenerate ? SIG_DEGENERATE : !equal ? SIG_MISMATCH : SIG_OK;
}

// s = k + sk h mod l: sk to Montgomery form mod l, one Montgomery product with the plain h, one modular addition
__global__ __launch_bounds__(LANE_BLOCK) void sign_finish_kernel(const u32 *__restrict__ keys, const u32 *__restrict__ nonces,
                                                                 const u32 *__restrict__ challenges, size_t n,
                                                                 u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const S skh = S::mul(S::to_mont(S::load(keys + i * 8)), S::load(challenges + i * 8));
    S::add(S::load(nonces + i * 8), skh).store(out + i * 8);
}

} // namespace schnorr

hipError_t schnorr_challenge(hipStream_t s, const u32 *pks, const u32 *nonce_pts, const u32 *messages, const u32 *lengths,
                             u32 stride, size_t n, u32 *challenges) {
    return launch_lanes(schnorr::challenge_kernel, s, n, pks, nonce_pts, messages, lengths, stride, n, challenges);
}
hipError_t schnorr_verify(hipStream_t s, const u32 *table, const u32 *pks, const u32 *nonce_pts, const u32 *scalars,
                          const u32 *challenges, size_t n, uint8_t *status) {
    return launch_lanes(schnorr::verify_kernel, s, n, table, pks, nonce_pts, scalars, challenges, n, status);
}
hipError_t schnorr_sign_finish(hipStream_t s, const u32 *signing_keys, const u32 *nonces, const u32 *challenges, size_t n,
                               u32 *scalars_out) {
    return launch_lanes(schnorr::sign_finish_kernel, s, n, signing_keys, nonces, challenges, n, scalars_out);
}

} // namespace mg
