// Phase-2 key initialisation of the trusted setup on the MI355X: `mpc::initialize` (manta-trusted-setup/src/groth16/mpc.rs:353-431)
// turns a powers-of-tau accumulator into the first phase-2 proving key of a circuit, gamma = delta = 1. Both halves run on the
// GPU: the four group IFFTs that make the Lagrange bases (GroupEngine::group_ntt_device) and `specialize_to_phase_2`
// (:251-294), the column sums of the QAP matrices over those bases (GroupEngine::qap_columns, qap_columns.h). The host validates
// the matrices and lists their entries -- O(m + nnz) -- and copies the key out. Each power vector is uploaded once, the Lagrange
// bases never leave device memory, only the key comes back. SURVEY.md section 8(f-4).
#include "prover.h"
#include "staging.h"
#include <cstring>

namespace mg {
namespace {

// the entry list of GroupEngine::qap_columns, grown matrix by matrix
struct EntryList {
    std::vector<u32> col, src;
    std::vector<u64> val;
    void reserve(size_t n) { col.reserve(n), src.reserve(n), val.reserve(4 * n); }
    // every stored entry (i, j) of M: column col0 + j, basis row src0 + i
    void add_matrix(const mg_csr *M, u64 m, u32 col0, u32 src0) {
        for (u64 i = 0; i < m; ++i)
            for (u32 k = M->row_ptr[i]; k < M->row_ptr[i + 1]; ++k) col.push_back(col0 + M->col[k]), src.push_back(src0 + (u32)i);
        val.insert(val.end(), M->val, M->val + 4 * M->nnz);
    }
    // `add_dummy_constraints` (mpc.rs:299-312): column col0 + i takes basis row src0 + i with the coefficient 1, i < P
    void add_dummies(u64 P, u32 col0, u32 src0, const u64 one[4]) {
        for (u64 i = 0; i < P; ++i) col.push_back(col0 + (u32)i), src.push_back(src0 + (u32)i), val.insert(val.end(), one, one + 4);
    }
    QapEntries view() const { return QapEntries{col.data(), src.data(), val.data(), col.size()}; }
};

} // namespace

int qap_columns(int curve, int group, size_t n_terms, const u64 *const *bases, const mg_csr *const *mats, u64 m, u64 n_cols,
                u32 entries_per_lane, u64 *out) {
    GroupEngine *e = get_engine(curve, group);
    if (!e || !n_terms || !bases || !mats || !out || m == 0 || n_cols == 0 || m >= ((u64)1 << 32) || n_cols >= ((u64)1 << 32))
        return MG_ERR_ARG;
    u64 total = 0;
    for (size_t t = 0; t < n_terms; ++t) {
        if (!bases[t]) return MG_ERR_ARG;
        if (const int rc = validate_csr(mats[t], m, n_cols)) return rc;
        total += mats[t]->nnz;
        if (total >= ((u64)1 << 31)) return MG_ERR_ARG; // the sort's limit
    }
    if (n_cols > e->qap_max_columns()) return MG_ERR_ARG;
    if ((u64)n_terms * m >= ((u64)1 << 32)) return MG_ERR_ARG; // basis rows are 32-bit indices
    const size_t pt = (size_t)e->affine_words() * 4;
    if (total == 0) {
        std::memset(out, 0, (size_t)n_cols * pt);
        return MG_OK;
    }
    EntryList en;
    en.reserve(total);
    for (size_t t = 0; t < n_terms; ++t) en.add_matrix(mats[t], m, 0u, (u32)(t * m));
    DevCall d; // the bases of all terms, one behind the other
    if (const int rc = d.begin({n_terms * (size_t)m * pt}, "mg_qap_columns")) return rc;
    for (size_t t = 0; t < n_terms; ++t) d.up(0, bases[t], (size_t)m * pt, t * (size_t)m * pt);
    d.run([&] { return e->qap_columns(d.dev<u32>(0), n_terms * (size_t)m, en.view(), n_cols, entries_per_lane, (u32 *)out); });
    return d.finish();
}

int mpc_initialize(int curve, const mg_kzg_view *pw, const mg_csr *a, const mg_csr *b, const mg_csr *c, u64 m, u64 V, u64 P, u64 h_len,
                   const u64 *g1_gen, const u64 *g2_gen, const mg_pk_out *out) {
    FrEngine *fr = get_ntt_engine(curve);
    GroupEngine *g1 = get_engine(curve, 1), *g2 = get_engine(curve, 2);
    if (!fr || !g1 || !g2 || !pw || !a || !b || !c || !g1_gen || !g2_gen || !out || m == 0) return MG_ERR_ARG;
    if (!out->alpha_g1 || !out->beta_g1 || !out->delta_g1 || !out->beta_g2 || !out->gamma_g2 || !out->delta_g2 ||
        !out->gamma_abc_g1 || !out->a_query || !out->b_g1_query || !out->b_g2_query || !out->h_query || !out->l_query)
        return MG_ERR_ARG;
    if (!pw->tau_powers_g1 || !pw->tau_powers_g2 || !pw->alpha_tau_powers_g1 || !pw->beta_tau_powers_g1 || !pw->beta_g2)
        return MG_ERR_ARG;
    if (V < 2 || P < 1 || P >= V || m >= ((u64)1 << 31) || V >= ((u64)1 << 30)) return MG_ERR_ARG; // (3 V columns, 3 D basis rows: 32 bits)
    unsigned lg = 0;
    while (((u64)1 << lg) < m + P) ++lg; // GeneralEvaluationDomain::new(m + P)
    if ((int)lg > fr->two_adicity()) return MG_ERR_DOMAIN; // `TooManyConstraints` (before the matrices are read)
    if (lg > 26) return MG_ERR_ARG;                         // the group NTT's own limit
    int rc;
    if ((rc = validate_csr(a, m, V)) || (rc = validate_csr(b, m, V)) || (rc = validate_csr(c, m, V))) return rc;
    const u64 D = (u64)1 << lg;
    if (h_len != D - 1 && h_len != D) return MG_ERR_ARG;
    if (pw->n_g1 < D + h_len || pw->n_g2 < D) return MG_ERR_ARG; // where the reference would index out of bounds
    const u64 n1 = 2 * a->nnz + 2 * b->nnz + c->nnz + 2 * P; // entries of the G1 call
    if (n1 >= ((u64)1 << 31) || 3 * V > g1->qap_max_columns() || V > g2->qap_max_columns()) return MG_ERR_ARG;

    const u32 *tw = nullptr;
    u64 ninv[4], one[4];
    if ((rc = fr->domain_twiddles(lg, true, &tw, ninv))) return rc;
    g1->scalar_one_mont(one);
    const size_t p1 = (size_t)g1->affine_words() * 4, p2 = (size_t)g2->affine_words() * 4; // bytes per point
    std::vector<u32> h(h_len * p1 / 4), s1(3 * V * p1 / 4), s2(V * p2 / 4);
    {
        // G1: tau^i G (D + h_len of them) | alpha tau^i G | beta tau^i G | the Lagrange bases tauL, alphaL, betaL | h_query
        DevCall d;
        if ((rc = d.begin({(D + h_len) * p1, D * p1, D * p1, 3 * D * p1, h_len * p1}, "mg_mpc_initialize"))) return rc;
        d.up(0, pw->tau_powers_g1, (D + h_len) * p1);
        d.up(1, pw->alpha_tau_powers_g1, D * p1);
        d.up(2, pw->beta_tau_powers_g1, D * p1);
        u32 *const lag = d.dev<u32>(3);
        // h_query[i] = tau^(i+D) G - tau^i G (:372-377)
        d.run([&] { return g1->sub_device(d.dev<u32>(0) + D * (p1 / 4), d.dev<u32>(0), h_len, d.dev<u32>(4)); });
        for (int v = 0; v < 3; ++v) // :378-381
            d.run([&] { return g1->group_ntt_device(d.dev<u32>(v), lg, tw, (const u32 *)ninv, lag + (size_t)v * D * (p1 / 4)); });
        d.down(h.data(), 4, h_len * p1);
        // ONE column-sum call for the three G1 results: columns [0, V) a_query = A^T tauL (+ dummies), [V, 2V) b_g1_query = B^T tauL,
        // [2V, 3V) ext = A^T betaL + B^T alphaL + C^T tauL (+ dummies); basis rows [0, D) tauL, [D, 2D) alphaL, [2D, 3D) betaL
        EntryList en;
        en.reserve(n1);
        const u32 v = (u32)V, d32 = (u32)D;
        en.add_matrix(a, m, 0u, 0u), en.add_dummies(P, 0u, (u32)m, one);
        en.add_matrix(b, m, v, 0u);
        en.add_matrix(a, m, 2 * v, 2 * d32), en.add_matrix(b, m, 2 * v, d32), en.add_matrix(c, m, 2 * v, 0u);
        en.add_dummies(P, 2 * v, 2 * d32 + (u32)m, one);
        d.run([&] { return g1->qap_columns(lag, 3 * D, en.view(), 3 * V, 0, s1.data()); });
        if ((rc = d.finish())) return rc;
    }
    {
        DevCall d; // G2: tau^i G2 | tauL2
        if ((rc = d.begin({D * p2, D * p2}, "mg_mpc_initialize"))) return rc;
        d.up(0, pw->tau_powers_g2, D * p2);
        d.run([&] { return g2->group_ntt_device(d.dev<u32>(0), lg, tw, (const u32 *)ninv, d.dev<u32>(1)); });
        EntryList en;
        en.reserve(b->nnz);
        en.add_matrix(b, m, 0u, 0u);
        d.run([&] { return g2->qap_columns(d.dev<u32>(1), D, en.view(), V, 0, s2.data()); });
        if ((rc = d.finish())) return rc;
    }
    // everything succeeded: the key
    const unsigned char *q1 = (const unsigned char *)s1.data();
    std::memcpy(out->alpha_g1, pw->alpha_tau_powers_g1, p1);
    std::memcpy(out->beta_g1, pw->beta_tau_powers_g1, p1);
    std::memcpy(out->beta_g2, pw->beta_g2, p2);
    std::memcpy(out->delta_g1, g1_gen, p1);
    std::memcpy(out->gamma_g2, g2_gen, p2);
    std::memcpy(out->delta_g2, g2_gen, p2);
    std::memcpy(out->a_query, q1, V * p1);
    std::memcpy(out->b_g1_query, q1 + V * p1, V * p1);
    std::memcpy(out->gamma_abc_g1, q1 + 2 * V * p1, P * p1);
    std::memcpy(out->l_query, q1 + (2 * V + P) * p1, (V - P) * p1);
    std::memcpy(out->b_g2_query, s2.data(), V * p2);
    std::memcpy(out->h_query, h.data(), h_len * p1);
    return MG_OK;
}

} // namespace mg
