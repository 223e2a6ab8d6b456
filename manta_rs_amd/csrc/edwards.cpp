// Host layer of the embedded-curve operations and the Poseidon note encryption (mantagpu.h mg_edwards_* / mg_note_cipher_* /
// mg_notes_*): argument checks (all before any device work), the fixed-base table, chunking. Kernels in edwards_bn254.hip.
#include "edwards.h"
#include "edwards_dev.h"
#include "host_ec.h"
#include "point_codec.h"
#include <cstring>
#include <vector>

namespace mg {
namespace {

typedef host::HFp<Bn254FrCfg> H;

H h_const(const u32 *w) {
    H r;
    r.load_words(w);
    return r;
}

// the group law of edwards_dev.h on the host, for the 1 008 entries of a fixed-base table
struct HExt {
    H X, Y, Z, T;
    static HExt from_affine(const H &x, const H &y) { return HExt{x, y, H::one(), H::mul(x, y)}; }
    static HExt dbl(const HExt &p) {
        const H A = H::sqr(p.X), B = H::sqr(p.Y), C = H::dbl(H::sqr(p.Z));
        const H E = H::sub(H::sub(H::sqr(H::add(p.X, p.Y)), A), B), G = H::add(A, B), F = H::sub(G, C), Hh = H::sub(A, B);
        return HExt{H::mul(E, F), H::mul(G, Hh), H::mul(F, G), H::mul(E, Hh)};
    }
    static HExt add(const HExt &p, const HExt &q) {
        const H A = H::mul(p.X, q.X), B = H::mul(p.Y, q.Y), C = H::mul(H::mul(p.T, q.T), h_const(EdBn254::D)), D = H::mul(p.Z, q.Z);
        const H E = H::sub(H::sub(H::mul(H::add(p.X, p.Y), H::add(q.X, q.Y)), A), B);
        const H F = H::sub(D, C), G = H::add(D, C), Hh = H::sub(B, A);
        return HExt{H::mul(E, F), H::mul(G, Hh), H::mul(F, G), H::mul(E, Hh)};
    }
};

bool coords_reduced(const u64 *p) { return !H::geq_p(p) && !H::geq_p(p + 4); }
bool h_on_curve(const H &x, const H &y) {
    const H x2 = H::sqr(x), y2 = H::sqr(y);
    return H::add(x2, y2) == H::add(H::one(), H::mul(h_const(EdBn254::D), H::mul(x2, y2)));
}

// entry [j][m] = m 16^j B as x | y | d x y; one inversion for the whole table (Montgomery's trick)
void build_table(const u64 *base, std::vector<u32> &out) {
    H bx, by;
    std::memcpy(bx.v, base, 32);
    std::memcpy(by.v, base + 4, 32);
    std::vector<HExt> e(ED_TABLE_ENTRIES);
    HExt w = HExt::from_affine(bx, by);
    const HExt id = HExt{H::zero(), H::one(), H::one(), H::zero()};
    for (int j = 0; j < ED_WINDOWS; ++j) {
        e[j * 16] = id;
        e[j * 16 + 1] = w;
        for (int m = 2; m < 16; ++m) e[j * 16 + m] = HExt::add(e[j * 16 + m - 1], w);
        for (int k = 0; k < ED_WINDOW_BITS; ++k) w = HExt::dbl(w);
    }
    std::vector<H> pre(ED_TABLE_ENTRIES);
    H acc = H::one();
    for (int i = 0; i < ED_TABLE_ENTRIES; ++i) {
        pre[i] = acc;
        acc = H::mul(acc, e[i].Z);
    }
    H inv = H::inv(acc);
    const H d = h_const(EdBn254::D);
    out.resize(ED_TABLE_WORDS);
    for (int i = ED_TABLE_ENTRIES - 1; i >= 0; --i) {
        const H zi = H::mul(inv, pre[i]);
        inv = H::mul(inv, e[i].Z);
        const H x = H::mul(e[i].X, zi), y = H::mul(e[i].Y, zi);
        x.store_words(&out[(size_t)i * 24]);
        y.store_words(&out[(size_t)i * 24 + 8]);
        H::mul(d, H::mul(x, y)).store_words(&out[(size_t)i * 24 + 16]);
    }
}

bool scalar_ok(const u64 *k) { // < l
    for (int i = 3; i >= 0; --i) {
        const u64 li = (u64)EdBn254::L[2 * i] | ((u64)EdBn254::L[2 * i + 1] << 32);
        if (k[i] != li) return k[i] < li;
    }
    return false;
}
bool scalars_ok(const u64 *k, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!scalar_ok(k + 4 * i)) return false;
    return true;
}
int top_bit(const u64 *k) {
    for (int i = 255; i >= 0; --i)
        if ((k[i >> 6] >> (i & 63)) & 1) return i;
    return -1;
}

struct DevMem { // one call's device memory, freed on every path
    void *p = nullptr;
    ~DevMem() {
        if (p) hipFree(p);
    }
};

struct Span { // one per-lane array of a call: host pointer and bytes per lane
    const void *src;
    void *dst;
    size_t stride;
};

// The lanes of a call, EDWARDS_CHUNK at a time on the calling thread's setup stream: `consts` (the same for every lane) is
// uploaded once, each chunk's inputs are copied in, `launch(d_consts, d_in[], d_out[], count, stream)` enqueues kernels, the
// outputs are copied back. Device memory of a call = consts + scratch + min(n, EDWARDS_CHUNK) x (sum of the strides + scratch).
template <class Launch>
int run_chunks(size_t n, const void *consts, size_t const_bytes, std::vector<Span> ins, std::vector<Span> outs,
               size_t scratch_stride, Launch launch) {
    if (n == 0) return MG_OK;
    HeavyOp no_capture_meanwhile; // device memory is allocated and freed inside the call
    hipStream_t s = setup_stream();
    if (!s) return MG_ERR_OOM;
    const size_t cap = n < EDWARDS_CHUNK ? n : EDWARDS_CHUNK;
    const auto padded = [](size_t b) { return (b + 255) & ~size_t(255); }; // every array starts on a 256-byte boundary
    size_t total = padded(const_bytes) + padded(cap * scratch_stride);
    for (const Span &x : ins) total += padded(cap * x.stride);
    for (const Span &x : outs) total += padded(cap * x.stride);
    DevMem m;
    MG_HIP(hipMalloc(&m.p, total));
    uint8_t *p = (uint8_t *)m.p;
    if (const_bytes) MG_HIP(hipMemcpyAsync(p, consts, const_bytes, hipMemcpyHostToDevice, s));
    const uint8_t *d_consts = p;
    p += padded(const_bytes);
    std::vector<uint8_t *> d_in, d_out;
    for (const Span &x : ins) d_in.push_back(p), p += padded(cap * x.stride);
    for (const Span &x : outs) d_out.push_back(p), p += padded(cap * x.stride);
    uint8_t *d_scratch = p;
    for (size_t off = 0; off < n; off += cap) {
        const size_t cnt = n - off < cap ? n - off : cap;
        for (size_t q = 0; q < ins.size(); ++q)
            MG_HIP(hipMemcpyAsync(d_in[q], (const uint8_t *)ins[q].src + off * ins[q].stride, cnt * ins[q].stride,
                                  hipMemcpyHostToDevice, s));
        MG_HIP(launch(d_consts, d_in, d_out, d_scratch, cnt, s));
        for (size_t q = 0; q < outs.size(); ++q)
            MG_HIP(hipMemcpyAsync((uint8_t *)outs[q].dst + off * outs[q].stride, d_out[q], cnt * outs[q].stride,
                                  hipMemcpyDeviceToHost, s));
        MG_HIP(hipStreamSynchronize(s));
    }
    return MG_OK;
}

size_t count_bad(const uint8_t *st, size_t n) {
    size_t b = 0;
    for (size_t i = 0; i < n; ++i) b += st[i] != PT_OK;
    return b;
}

} // namespace
} // namespace mg

struct mg_note_cipher {
    std::vector<mg::u32> prm;   // round keys | MDS | initial state, Montgomery words
    std::vector<mg::u32> table; // fixed-base table of the generator
};

namespace mg {

int edwards_decode(int curve, const uint8_t *bytes, size_t n, int checked, u64 *out, uint8_t *status, size_t *n_bad) {
    if (curve != 0 || (n && (!bytes || !out))) return MG_ERR_ARG;
    std::vector<uint8_t> own;
    if (!status) {
        own.resize(n);
        status = own.data();
    }
    const int rc = run_chunks(n, nullptr, 0, {{bytes, nullptr, 32}}, {{nullptr, out, 64}, {nullptr, status, 1}}, 0,
                              [&](const uint8_t *, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *, size_t cnt,
                                  hipStream_t s) {
                                  EdwardsLaunch a{};
                                  a.op = EdwardsLaunch::DECODE;
                                  a.checked = checked != 0;
                                  a.a = (const u32 *)di[0];
                                  a.out = (u32 *)dout[0];
                                  a.status = dout[1];
                                  a.n = cnt;
                                  a.stream = s;
                                  return edwards_launch_bn254(a);
                              });
    if (rc == MG_OK && n_bad) *n_bad = count_bad(status, n);
    return rc;
}

int edwards_check(int curve, const u64 *affine, size_t n, uint8_t *status, size_t *n_bad) {
    if (curve != 0 || (n && !affine)) return MG_ERR_ARG;
    std::vector<uint8_t> own;
    if (!status) {
        own.resize(n);
        status = own.data();
    }
    const int rc = run_chunks(n, nullptr, 0, {{affine, nullptr, 64}}, {{nullptr, status, 1}}, 0,
                              [&](const uint8_t *, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *, size_t cnt,
                                  hipStream_t s) {
                                  EdwardsLaunch a{};
                                  a.op = EdwardsLaunch::CHECK;
                                  a.a = (const u32 *)di[0];
                                  a.status = dout[0];
                                  a.n = cnt;
                                  a.stream = s;
                                  return edwards_launch_bn254(a);
                              });
    if (rc == MG_OK && n_bad) *n_bad = count_bad(status, n);
    return rc;
}

int edwards_encode(int curve, const u64 *affine, size_t n, uint8_t *out) {
    if (curve != 0 || (n && (!affine || !out))) return MG_ERR_ARG;
    return run_chunks(n, nullptr, 0, {{affine, nullptr, 64}}, {{nullptr, out, 32}}, 0,
                      [&](const uint8_t *, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *, size_t cnt,
                          hipStream_t s) {
                          EdwardsLaunch a{};
                          a.op = EdwardsLaunch::ENCODE;
                          a.a = (const u32 *)di[0];
                          a.out = (u32 *)dout[0];
                          a.n = cnt;
                          a.stream = s;
                          return edwards_launch_bn254(a);
                      });
}

int edwards_mul(int curve, int mode, const u64 *points, size_t n_points, const u64 *scalars, size_t n_scalars, u64 *out) {
    if (curve != 0 || mode < 0 || mode > 2) return MG_ERR_ARG;
    if ((n_points && !points) || (n_scalars && !scalars)) return MG_ERR_ARG;
    if (mode == 0 && n_scalars != 1) return MG_ERR_ARG;
    if (mode == 1 && n_points != 1) return MG_ERR_ARG;
    if (mode == 2 && n_points != n_scalars) return MG_ERR_ARG;
    const size_t n = mode == 0 ? n_points : n_scalars;
    if (n && !out) return MG_ERR_ARG;
    if (!scalars_ok(scalars, n_scalars)) return MG_ERR_ARG;
    if (mode == 1 && !coords_reduced(points)) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    if (mode == 0) {
        const int top = top_bit(scalars);
        return run_chunks(n, scalars, 32, {{points, nullptr, 64}}, {{nullptr, out, 64}}, 0,
                          [&](const uint8_t *dc, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *, size_t cnt,
                              hipStream_t s) {
                              EdwardsLaunch a{};
                              a.op = EdwardsLaunch::MUL_SHARED;
                              a.consts = (const u32 *)dc;
                              a.top = top;
                              a.a = (const u32 *)di[0];
                              a.out = (u32 *)dout[0];
                              a.n = cnt;
                              a.stream = s;
                              return edwards_launch_bn254(a);
                          });
    }
    if (mode == 1) {
        std::vector<u32> table;
        build_table(points, table);
        return run_chunks(n, table.data(), table.size() * 4, {{scalars, nullptr, 32}}, {{nullptr, out, 64}}, 0,
                          [&](const uint8_t *dc, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *, size_t cnt,
                              hipStream_t s) {
                              EdwardsLaunch a{};
                              a.op = EdwardsLaunch::MUL_FIXED;
                              a.consts = (const u32 *)dc;
                              a.b = (const u32 *)di[0];
                              a.out = (u32 *)dout[0];
                              a.n = cnt;
                              a.stream = s;
                              return edwards_launch_bn254(a);
                          });
    }
    return run_chunks(n, nullptr, 0, {{points, nullptr, 64}, {scalars, nullptr, 32}}, {{nullptr, out, 64}}, 0,
                      [&](const uint8_t *, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *, size_t cnt,
                          hipStream_t s) {
                          EdwardsLaunch a{};
                          a.op = EdwardsLaunch::MUL_PAIRWISE;
                          a.a = (const u32 *)di[0];
                          a.b = (const u32 *)di[1];
                          a.out = (u32 *)dout[0];
                          a.n = cnt;
                          a.stream = s;
                          return edwards_launch_bn254(a);
                      });
}

int edwards_add(int curve, const u64 *a_pts, const u64 *b_pts, size_t n, u64 *out) {
    if (curve != 0 || (n && (!a_pts || !b_pts || !out))) return MG_ERR_ARG;
    return run_chunks(n, nullptr, 0, {{a_pts, nullptr, 64}, {b_pts, nullptr, 64}}, {{nullptr, out, 64}}, 0,
                      [&](const uint8_t *, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *, size_t cnt,
                          hipStream_t s) {
                          EdwardsLaunch a{};
                          a.op = EdwardsLaunch::ADD;
                          a.a = (const u32 *)di[0];
                          a.b = (const u32 *)di[1];
                          a.out = (u32 *)dout[0];
                          a.n = cnt;
                          a.stream = s;
                          return edwards_launch_bn254(a);
                      });
}

// bytes = `IncomingBaseEncryptionScheme` in the manta codec: the width-4 permutation (63 x 4 round keys | 4 x 4 MDS), then
// `FixedEncryption::initial_state` as a u64 length (4) and four elements
int note_cipher_create(int curve, const uint8_t *bytes, size_t len, const u64 *generator, mg_note_cipher **out) {
    if (out) *out = nullptr;
    if (curve != 0 || !bytes || !generator || !out) return MG_ERR_ARG;
    constexpr size_t NP = (size_t)(ED_CIPHER_FULL + ED_CIPHER_PARTIAL) * 4 + 16;
    if (len != NP * 32 + 8 + 4 * 32) return MG_ERR_ARG;
    u64 state_len;
    std::memcpy(&state_len, bytes + NP * 32, 8);
    if (state_len != 4) return MG_ERR_ARG;
    std::vector<u32> prm((size_t)ED_CIPHER_ELEMS * 8);
    for (size_t i = 0; i < (size_t)ED_CIPHER_ELEMS; ++i) {
        H a;
        std::memcpy(a.v, bytes + 32 * i + (i >= NP ? 8 : 0), 32); // little-endian canonical: a value >= p is refused
        if (H::geq_p(a.v)) return MG_ERR_ARG;
        H::to_mont(a).store_words(&prm[i * 8]);
    }
    if (!coords_reduced(generator)) return MG_ERR_ARG;
    H gx, gy;
    std::memcpy(gx.v, generator, 32);
    std::memcpy(gy.v, generator + 4, 32);
    if (!h_on_curve(gx, gy)) return MG_ERR_ARG;
    mg_note_cipher *h = new mg_note_cipher;
    h->prm = std::move(prm);
    build_table(generator, h->table);
    *out = h;
    return MG_OK;
}

void note_cipher_destroy(mg_note_cipher *h) { delete h; }

// consts of a notes call: cipher parameters | fixed-base table | the shared scalar (decrypt)
int notes_encrypt(const mg_note_cipher *h, const u64 *recv_keys, const u64 *randomness, const u64 *plaintexts, size_t n,
                  u64 *epk_out, u64 *ciphertext_out, u64 *tag_out) {
    if (!h || (n && (!recv_keys || !randomness || !plaintexts || !epk_out || !ciphertext_out || !tag_out))) return MG_ERR_ARG;
    if (!scalars_ok(randomness, n)) return MG_ERR_ARG;
    std::vector<u32> consts(h->prm);
    consts.insert(consts.end(), h->table.begin(), h->table.end());
    const size_t prm_words = h->prm.size();
    return run_chunks(n, consts.data(), consts.size() * 4, {{recv_keys, nullptr, 64}, {randomness, nullptr, 32}, {plaintexts, nullptr, 96}},
                      {{nullptr, epk_out, 64}, {nullptr, ciphertext_out, 96}, {nullptr, tag_out, 32}}, 64,
                      [&](const uint8_t *dc, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *scratch, size_t cnt,
                          hipStream_t s) {
                          EdwardsLaunch a{};
                          a.n = cnt;
                          a.stream = s;
                          a.op = EdwardsLaunch::MUL_FIXED; // epk = G * randomness
                          a.consts = (const u32 *)dc + prm_words;
                          a.b = (const u32 *)di[1];
                          a.out = (u32 *)dout[0];
                          hipError_t e = edwards_launch_bn254(a);
                          if (e != hipSuccess) return e;
                          a.op = EdwardsLaunch::MUL_PAIRWISE; // key = recv_key * randomness
                          a.a = (const u32 *)di[0];
                          a.out = (u32 *)scratch;
                          if ((e = edwards_launch_bn254(a)) != hipSuccess) return e;
                          a.op = EdwardsLaunch::ENCRYPT;
                          a.consts = (const u32 *)dc;
                          a.a = (const u32 *)scratch;
                          a.b = (const u32 *)di[2];
                          a.out = (u32 *)dout[1];
                          a.out2 = (u32 *)dout[2];
                          return edwards_launch_bn254(a);
                      });
}

int notes_decrypt(const mg_note_cipher *h, const u64 *viewing_key, const u64 *epks, const u64 *ciphertexts, const u64 *tags,
                  size_t n, u64 *plaintext_out, uint8_t *ok, uint8_t *status) {
    if (!h || !viewing_key || (n && (!epks || !ciphertexts || !tags || !plaintext_out || !ok))) return MG_ERR_ARG;
    if (!scalar_ok(viewing_key)) return MG_ERR_ARG;
    std::vector<uint8_t> own;
    if (!status) {
        own.resize(n);
        status = own.data();
    }
    std::vector<u32> consts(h->prm);
    const size_t prm_words = consts.size();
    consts.resize(prm_words + 8);
    std::memcpy(&consts[prm_words], viewing_key, 32);
    const int top = top_bit(viewing_key);
    const int rc = run_chunks(n, consts.data(), consts.size() * 4, {{epks, nullptr, 64}, {ciphertexts, nullptr, 96}, {tags, nullptr, 32}},
                              {{nullptr, plaintext_out, 96}, {nullptr, status, 1}}, 64,
                              [&](const uint8_t *dc, std::vector<uint8_t *> &di, std::vector<uint8_t *> &dout, uint8_t *scratch,
                                  size_t cnt, hipStream_t s) {
                                  EdwardsLaunch a{};
                                  a.n = cnt;
                                  a.stream = s;
                                  a.op = EdwardsLaunch::MUL_SHARED; // key = epk * viewing key
                                  a.consts = (const u32 *)dc + prm_words;
                                  a.top = top;
                                  a.a = (const u32 *)di[0];
                                  a.out = (u32 *)scratch;
                                  const hipError_t e = edwards_launch_bn254(a);
                                  if (e != hipSuccess) return e;
                                  a.op = EdwardsLaunch::DECRYPT;
                                  a.consts = (const u32 *)dc;
                                  a.a = (const u32 *)scratch;
                                  a.b = (const u32 *)di[1];
                                  a.c = (const u32 *)di[2];
                                  a.out = (u32 *)dout[0];
                                  a.status = dout[1];
                                  return edwards_launch_bn254(a);
                              });
    if (rc == MG_OK)
        for (size_t i = 0; i < n; ++i) ok[i] = status[i] == NOTE_OK;
    return rc;
}

} // namespace mg
