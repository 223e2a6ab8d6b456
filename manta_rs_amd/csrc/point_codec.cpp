// Host layer of the batched point codec (mantagpu.h mg_points_decode / mg_points_check / mg_points_encode /
// mg_proofs_decode / mg_ppot_points_decode / mg_ppot_points_encode): argument checks, status counting and the proof split; kernels and chunking in point_codec.h.
#include "point_codec.h"

namespace mg {

namespace {

int run(int curve, const PointCodecArgs &a) {
    if (curve == 0) return point_codec_bn254(a);
    if (curve == 1) return point_codec_bls381(a);
    return MG_ERR_ARG;
}
bool valid(int curve, int group) { return (curve == 0 || curve == 1) && (group == 1 || group == 2); }
size_t fq_bytes(int curve) { return curve == 0 ? 32 : 48; }

} // namespace

int points_decode(int curve, int group, const uint8_t *bytes, size_t n, int compressed, int checked, u64 *out,
                  uint8_t *status, size_t *n_bad) {
    if (!valid(curve, group) || (n && (!bytes || !out))) return MG_ERR_ARG;
    if (compressed && !checked) return MG_ERR_ARG; // arkworks has no unchecked compressed read: the root is the check
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    const int rc = run(curve, PointCodecArgs{group, 0, compressed != 0, checked != 0, bytes, n, out, status});
    if (rc == MG_OK && n_bad) *n_bad = count_bad(status, n);
    return rc;
}

int points_check(int curve, int group, const u64 *affine, size_t n, uint8_t *status, size_t *n_bad) {
    if (!valid(curve, group) || (n && !affine)) return MG_ERR_ARG;
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    const int rc = run(curve, PointCodecArgs{group, 1, 0, 1, affine, n, nullptr, status});
    if (rc == MG_OK && n_bad) *n_bad = count_bad(status, n);
    return rc;
}

int points_encode(int curve, int group, const u64 *affine, size_t n, int compressed, uint8_t *out) {
    if (!valid(curve, group) || (n && (!affine || !out))) return MG_ERR_ARG;
    return run(curve, PointCodecArgs{group, 2, compressed != 0, 0, affine, n, out, nullptr});
}

// The PPoT record format (point_codec.h `Ppot`): Bn254 only, the ceremony's curve; both forms may be read unchecked
int ppot_points_decode(int curve, int group, const uint8_t *bytes, size_t n, int compressed, int checked, u64 *out,
                       uint8_t *status, size_t *n_bad) {
    if (curve != 0 || !valid(curve, group) || (n && (!bytes || !out))) return MG_ERR_ARG;
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    const int rc = run(curve, PointCodecArgs{group, 0, compressed != 0, checked != 0, bytes, n, out, status, 1});
    if (rc == MG_OK && n_bad) *n_bad = count_bad(status, n);
    return rc;
}

int ppot_points_encode(int curve, int group, const u64 *affine, size_t n, int compressed, uint8_t *out) {
    if (curve != 0 || !valid(curve, group) || (n && (!affine || !out))) return MG_ERR_ARG;
    return run(curve, PointCodecArgs{group, 2, compressed != 0, 0, affine, n, out, nullptr, 1});
}

// k compressed proofs a | b | c: the 2k G1 points (a_i, c_i) and the k G2 points go to the GPU as two batches
int proofs_decode(int curve, const uint8_t *bytes, size_t k, u64 *points_out, uint8_t *ok) {
    if ((curve != 0 && curve != 1) || (k && (!bytes || !points_out || !ok))) return MG_ERR_ARG;
    if (k == 0) return MG_OK;
    const size_t fb = fq_bytes(curve), pb = 4 * fb, l1 = fb / 4, l2 = fb / 2; // u64 limbs of a G1 / G2 point
    std::vector<uint8_t> g1(2 * k * fb), g2(k * 2 * fb), s1(2 * k), s2(k);
    for (size_t i = 0; i < k; ++i) {
        const uint8_t *p = bytes + i * pb;
        std::memcpy(g1.data() + 2 * i * fb, p, fb);
        std::memcpy(g1.data() + (2 * i + 1) * fb, p + 3 * fb, fb);
        std::memcpy(g2.data() + i * 2 * fb, p + fb, 2 * fb);
    }
    std::vector<u64> p1(2 * k * l1), p2(k * l2);
    int rc = points_decode(curve, 1, g1.data(), 2 * k, 1, 1, p1.data(), s1.data(), nullptr);
    if (rc == MG_OK) rc = points_decode(curve, 2, g2.data(), k, 1, 1, p2.data(), s2.data(), nullptr);
    if (rc != MG_OK) return rc;
    const size_t row = 2 * l1 + l2;
    for (size_t i = 0; i < k; ++i) {
        u64 *o = points_out + i * row;
        ok[i] = s1[2 * i] == PT_OK && s2[i] == PT_OK && s1[2 * i + 1] == PT_OK;
        if (!ok[i]) {
            std::memset(o, 0, row * 8);
            continue;
        }
        std::memcpy(o, p1.data() + 2 * i * l1, l1 * 8);
        std::memcpy(o + l1, p2.data() + i * l2, l2 * 8);
        std::memcpy(o + l1 + l2, p1.data() + (2 * i + 1) * l1, l1 * 8);
    }
    return MG_OK;
}

} // namespace mg
