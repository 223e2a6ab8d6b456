// Groth16 verification on the MI355X: pairing engine interface + the verifying-key object.
#pragma once
#include "../../include/mantagpu.h"
#include "engine.h"

namespace mg {

// A set of n pairs (P_i, Q_i) for the Miller loops, the one argument of every engine call that takes pairs. Plain pointers,
// borrowed for the call (begin() has staged what it needs before it returns).
struct PairList {
    size_t n = 0;
    // n affine G1 points, host Montgomery words; all zero = infinity, and such a pair contributes 1. The entries of the XYZZ
    // prefix below, and of the pairs a two-step product takes later, are not read
    const u32 *p_affine_host = nullptr;
    // n pointers: d_coeffs[i] = the prepared Q_i in device memory (from prepare()), or null where Q_i is a fresh affine point,
    // prepared on the fly next to its Miller loop
    const u32 *const *d_coeffs = nullptr;
    // n affine G2 points, host Montgomery words, read where d_coeffs[i] is null; may be null when every pair is prepared.
    // A fresh Q_i that is all zero (infinity) leaves its pair out: the engine sees to that itself
    const u32 *q_affine_host = nullptr;
    // optional, n flags: skip[i] != 0 leaves pair i out (it contributes 1) -- the only way to leave out a PREPARED pair,
    // whose infinity shows in no argument (its coefficient block is all zero and must never be consumed)
    const unsigned char *skip = nullptr;
    // optional prefix: the G1 points of the first n_xyzz pairs lie in DEVICE memory as (X, Y, ZZ, ZZZ), 4 fq_words() each, left
    // there by a kernel on the HIP stream `producer`, which the Miller launch waits for (the lines of such a pair are taken
    // times ZZ ZZZ, which the final exponentiation removes: no inversion between a scalar multiplication and its pairing)
    const u32 *d_p_xyzz = nullptr;
    size_t n_xyzz = 0;
    void *producer = nullptr;
};

class PairingEngine {
  public:
    virtual ~PairingEngine() {}
    virtual int n_coeffs() const = 0;    // line-coefficient triples per prepared G2 point (91 BN254 / 68 BLS12-381)
    virtual int coeff_words() const = 0; // u32 per triple
    virtual int f12_words() const = 0;
    virtual int fq_words() const = 0;
    // G2Prepared::from for n affine points (host, Montgomery) -> device array n x n_coeffs x coeff_words (hipFree it)
    virtual int prepare(const u32 *q_affine_host, size_t n, u32 **d_out) = 0;
    // out = [final_exponentiation] ( prod_i MillerLoop(P_i, Q_i) )
    virtual int pairing_product(const PairList &pairs, bool do_final_exp, u32 *out_f12_host) = 0;
    // the same in two steps: the Miller loops of the first n_early pairs start at once (P points of those only; coefficients /
    // Q / skip of all n); end() takes the G1 points of the other pairs -- which must have prepared coefficients -- and finishes.
    // A handle is consumed by exactly one end() or abandon().
    virtual int pairing_product_begin(const PairList &pairs, size_t n_early, void **handle) = 0;
    virtual int pairing_product_end(void *handle, const u32 *p_late_affine_host, bool do_final_exp, u32 *out_f12_host) = 0;
    virtual void pairing_product_abandon(void *handle) = 0;
    // *ok = (prod_i e(P_i, Q_i) == 1): all points host affine Montgomery words, every Q_i prepared on the fly; a pair with an
    // infinity member (all-zero words) contributes 1
    virtual int product_is_one(const u32 *p_affine_host, const u32 *q_affine_host, size_t n, int *ok) = 0;
    // n_groups <= MG_VERIFY_EACH_CHUNK independent products of group_size <= 64 pairs each, a verdict each:
    //     verdict_host[t] = (final_exponentiation(prod_{j < group_size} MillerLoop(P_{t,j}, Q_{t,j})) == target)
    // pairs.n = group_size * n_groups, MEMBER-MAJOR: pair j of group t at index j * n_groups + t in every array (an XYZZ prefix
    // of n_groups pairs: the first member of every group comes from the device). d_target: an Fq12 in device memory,
    // null = 1. One Miller launch and one tail launch whatever the verdicts; only the verdict bytes are downloaded.
    virtual int pairing_check_groups(const PairList &pairs, size_t group_size, size_t n_groups, const u32 *d_target,
                                     unsigned char *verdict_host) = 0;
    // product_is_one per group: points [n_groups][group_size], group-major as a caller holds them; any n_groups (chunked)
    virtual int product_is_one_each(const u32 *p_affine_host, const u32 *q_affine_host, size_t group_size, size_t n_groups,
                                    unsigned char *ok) = 0;
    // one building block of the pairing over n elements (mantagpu.h mg_pairing_op): host arrays in and out, one launch
    virtual int tower_op(int op, const u32 *a, const u32 *b, const int16_t *coeffs, size_t n, u32 *out) = 0;
};
// what mg_pairing_op refuses, decided on the host before any device work
inline int pairing_op_check(int op, const void *a, const void *b, const int16_t *coeffs, size_t n, const void *out) {
    if (op < MG_PAIRING_MUL12 || op > MG_PAIRING_FQ_LINCOMB || !a || !out || n == 0 || n > MG_PAIRING_OP_MAX) return MG_ERR_ARG;
    if ((op == MG_PAIRING_MUL12 || op == MG_PAIRING_ELL || op == MG_PAIRING_FQ2_MUL) && !b) return MG_ERR_ARG;
    if (op == MG_PAIRING_FQ_LINCOMB) { // `lincomb` needs the positive and the negative coefficient sum below 256 each
        if (!coeffs) return MG_ERR_ARG;
        for (size_t i = 0; i < n; ++i) {
            int pos = 0, neg = 0;
            for (int m = 0; m < MG_PAIRING_LINCOMB_OPERANDS; ++m) {
                const int c = coeffs[i * MG_PAIRING_LINCOMB_OPERANDS + m];
                if (c < -255 || c > 255) return MG_ERR_ARG;
                pos += c > 0 ? c : 0, neg += c < 0 ? -c : 0;
            }
            if (pos >= 256 || neg >= 256) return MG_ERR_ARG;
        }
    }
    return MG_OK;
}
PairingEngine *make_pairing_engine_bn254();
PairingEngine *make_pairing_engine_bls381();
PairingEngine *get_pairing_engine(int curve); // per (device, curve)

class Verifier {
  public:
    virtual ~Verifier() {}
    virtual u64 n_inputs() const = 0;
    // ark-groth16 verify_proof: inputs = P - 1 public inputs (Montgomery Fr), proof = a | b | c affine Montgomery
    virtual int verify(const u64 *inputs_mont, const u64 *proof_points, int *ok) = 0;
    // k proofs at once by random linear combination; rand = k x 2 u64 (128-bit coefficients from the caller's RNG)
    virtual int verify_batch(u64 k, const u64 *inputs_mont, const u64 *proof_points, const u64 *rand128, int *ok) = 0;
    // k proofs, a verdict each: ok[i] = what verify() answers for row i (three pairs per proof, MG_VERIFY_EACH_CHUNK proofs per pass)
    virtual int verify_each(u64 k, const u64 *inputs_mont, const u64 *proof_points, uint8_t *ok) = 0;
    virtual size_t encoded_size() const = 0;
    virtual int encode(uint8_t *out) const = 0;          // VerifyingContext wire format, groth16.rs:337-361
    virtual int alpha_beta_bytes(uint8_t *out) const = 0; // 12 canonical Fq elements, arkworks order
};
int verifier_create(int curve, const u64 *alpha_g1, const u64 *beta_g2, const u64 *gamma_g2, const u64 *delta_g2,
                    const u64 *gamma_abc_g1, u64 n_inputs, Verifier **out);
int verifier_create_from_bytes(int curve, const uint8_t *bytes, size_t len, Verifier **out);
// Proof::deserialize (compressed a | b | c) -> affine Montgomery points; checks canonical encoding, curve and subgroup
int proof_decode(int curve, const uint8_t *bytes, u64 *points_out);

} // namespace mg
