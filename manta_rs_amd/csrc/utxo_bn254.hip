// Kernels of manta-pay's UTXO statement over BN254 Fr (manta-accounting/src/transfer/utxo/protocol.rs `derive_mint`,
// `utxo_reconstruct`, `utxo_check`, `item_hash`, `derive_spend`; manta-pay/src/config/utxo.rs): one UTXO or one key per lane,
// wave64. One lane runs its whole chain -- commitment (Poseidon5), compare, accumulator item (Poseidon4), nullifier commitment
// (Poseidon3) -- with the intermediates in registers. The permutation is pos::permute of poseidon.h; the constants of the four
// hashers sit in one device buffer (utxo.h) and are read at wave-uniform addresses. The transparent / opaque selection and the
// compare are selects: a failed lane keeps computing and is masked at the store. Behind each kernel, its launch function (utxo.h).
#include "utxo.h"
#include "edwards_dev.h"
#include "poseidon.h"

namespace mg {
namespace utxo {

typedef EdBn254 E;
typedef Bn254FrCfg C;
typedef Fp<C> F;
constexpr int HF = UTXO_FULL / 2;

// `Hasher::hash`: word 0 of the permutation of (tag, inputs)
template <int T> MG_DEV F hash(const u32 *__restrict__ prm, int partial, const F (&in)[T - 1]) {
    F st[T];
    st[0] = pos::tag_of<C>(prm, T, HF, partial);
#pragma unroll
    for (int j = 1; j < T; ++j) st[j] = in[j - 1];
    pos::permute<C, T>(st, prm, HF, partial);
    return st[0];
}

// `derive_mint` (protocol.rs:1152-1207) without the notes: commitment = H5(randomness, secret id, secret value, rk.x, rk.y)
// (config/utxo.rs:367-393), record = flag | public id | public value | commitment, item = H4(record) (utxo.rs:1153-1167).
// `Visibility::secret` / `public` (protocol.rs:93-114): the asset on its side, (0, 0) on the other.
__global__ __launch_bounds__(LANE_BLOCK) void mint_kernel(const u32 *__restrict__ prm, const u32 *__restrict__ keys,
                                                          const u32 *__restrict__ plain, const uint8_t *__restrict__ flags,
                                                          size_t n, u32 *__restrict__ utxos, u32 *__restrict__ items,
                                                          uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 fl = flags[i];
    const bool transparent = fl == 1;
    const F z = F::zero();
    const F id = F::load(plain + i * 24 + 8), val = F::load(plain + i * 24 + 16);
    const bool bad = fl > 1 || !ed::fits_u128(val);
    const F in5[5] = {F::load(plain + i * 24), F::select(transparent, z, id), F::select(transparent, z, val),
                      F::load(keys + i * 16), F::load(keys + i * 16 + 8)};
    const F cm = hash<6>(prm + UTXO_H5_OFF, UTXO_H5_PARTIAL, in5);
    const F in4[4] = {F::select(transparent, F::one(), z), F::select(transparent, id, z), F::select(transparent, val, z), cm};
    const F item = hash<5>(prm + UTXO_H4_OFF, UTXO_H4_PARTIAL, in4);
#pragma unroll
    for (int j = 0; j < 4; ++j) F::select(bad, z, in4[j]).store(utxos + (i * 4 + j) * 8);
    F::select(bad, z, item).store(items + i * 8);
    status[i] = bad ? UTXO_BAD_ENCODING : UTXO_OK;
}

// `utxo_check` (protocol.rs:1461-1499): the record is rebuilt from the plaintext's asset, the identifier (the record's flag, the
// plaintext's randomness) and the address's receiving key, and compared whole -- flag, both public words, commitment -- with the
// ledger's; then `item_hash` and, with an authorization key, the nullifier commitment H3(pak.x, pak.y, item) of `derive_spend`
// (protocol.rs:1291-1350, utxo.rs:1465-1485). shared = rk.x | rk.y | pak.x | pak.y.
template <bool NULLIFIER>
__global__ __launch_bounds__(LANE_BLOCK) void open_kernel(const u32 *__restrict__ prm, const u32 *__restrict__ shared,
                                                          const u32 *__restrict__ plain, const u32 *__restrict__ utxos, size_t n,
                                                          u32 *__restrict__ items, u32 *__restrict__ nullifiers,
                                                          uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F z = F::zero();
    const F flag = F::load(utxos + i * 32), pid = F::load(utxos + i * 32 + 8), pval = F::load(utxos + i * 32 + 16);
    const F id = F::load(plain + i * 24 + 8), val = F::load(plain + i * 24 + 16);
    const bool transparent = flag == F::one();
    const bool bad = !(transparent || flag.is_zero()) || !ed::fits_u128(val) || !ed::fits_u128(pval);
    const bool same_public = F::select(transparent, id, z) == pid && F::select(transparent, val, z) == pval;
    const F in5[5] = {F::load(plain + i * 24), F::select(transparent, z, id), F::select(transparent, z, val), F::load(shared),
                      F::load(shared + 8)};
    const F cm = hash<6>(prm + UTXO_H5_OFF, UTXO_H5_PARTIAL, in5);
    const bool match = same_public && cm == F::load(utxos + i * 32 + 24);
    const F in4[4] = {flag, pid, pval, cm};
    const F item = hash<5>(prm + UTXO_H4_OFF, UTXO_H4_PARTIAL, in4);
    const uint8_t st = bad ? UTXO_BAD_ENCODING : !match ? UTXO_MISMATCH : UTXO_OK;
    const bool keep = st == UTXO_OK;
    F::select(keep, item, z).store(items + i * 8);
    if (NULLIFIER) {
        const F in3[3] = {F::load(shared + 16), F::load(shared + 24), item};
        F::select(keep, hash<4>(prm + UTXO_H3_OFF, UTXO_H3_PARTIAL, in3), z).store(nullifiers + i * 8);
    }
    status[i] = st;
}

// `ViewingKeyDerivationFunction::viewing_key` (utxo.rs:523-545): H2(pak.x, pak.y) as an integer, reduced mod l
// (`rem_mod_prime`). r < 8 l, so the quotient's three bits are three conditional subtractions of 4 l, 2 l and l.
__global__ __launch_bounds__(LANE_BLOCK) void viewing_keys_kernel(const u32 *__restrict__ prm, const u32 *__restrict__ paks,
                                                                  size_t n, u32 *__restrict__ scalars) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F in2[2] = {F::load(paks + i * 16), F::load(paks + i * 16 + 8)};
    F v = F::from_mont(hash<3>(prm + UTXO_H2_OFF, UTXO_H2_PARTIAL, in2));
    ed::sub_shifted_l_if_geq<2>(v.v);
    ed::sub_shifted_l_if_geq<1>(v.v);
    ed::sub_shifted_l_if_geq<0>(v.v);
    v.store(scalars + i * 8);
}

} // namespace utxo

hipError_t utxo_mint(hipStream_t s, const u32 *prm, const u32 *recv_keys, const u32 *plain, const uint8_t *flags, size_t n,
                     u32 *utxos_out, u32 *items, uint8_t *status) {
    return launch_lanes(utxo::mint_kernel, s, n, prm, recv_keys, plain, flags, n, utxos_out, items, status);
}
hipError_t utxo_open(hipStream_t s, const u32 *prm, const u32 *shared, const u32 *plain, const u32 *utxos, size_t n, u32 *items,
                     u32 *nullifiers, uint8_t *status) {
    return launch_lanes(nullifiers ? utxo::open_kernel<true> : utxo::open_kernel<false>, s, n, prm, shared, plain, utxos, n, items,
                        nullifiers, status);
}
hipError_t utxo_viewing_keys(hipStream_t s, const u32 *prm, const u32 *paks, size_t n, u32 *scalars) {
    return launch_lanes(utxo::viewing_keys_kernel, s, n, prm, paks, n, scalars);
}

} // namespace mg
