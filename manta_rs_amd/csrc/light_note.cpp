// Host layer of the AES-GCM notes, the address partition and the Merkle shard index (mantagpu.h mg_light_notes_* /
// mg_outgoing_notes_* / mg_address_partitions / mg_merkle_shard_indices, mg_aes256_gcm, mg_blake2s): argument checks (all before
// any device work), the wallet's own partition of a scanning call, the compaction of its matching lanes, chunking. Kernels in
// light_note_bn254.hip; the key agreements are the kernels of edwards_bn254.hip, the generator's table is the model's (utxo.h).
#include "light_note.h"
#include "aes_gcm.h"
#include "blake2s.h"
#include "edwards_host.h"
#include "utxo.h"
#include <vector>

namespace mg {
namespace {

using namespace edh;

// the widest per-lane record of these calls is 96 bytes: n of them, and n of anything smaller, must not wrap a size_t
bool lanes_ok(size_t n) { return n <= SIZE_MAX / 128; }

// `AddressPartitionFunction::partition` of one affine Montgomery point on the host, as byte_hash_kernel<2> computes it
uint8_t partition_of(const u32 *point) {
    static const char prefix[] = "manta-v1.0.0/address-partition-function";
    uint8_t stream[sizeof(prefix) - 1 + 64], out;
    std::memcpy(stream, prefix, sizeof(prefix) - 1);
    for (int c = 0; c < 2; ++c) {
        const H v = H::from_mont(h_const(point + 8 * c));
        std::memcpy(stream + sizeof(prefix) - 1 + 32 * c, v.v, 32);
    }
    blake2s::hash(stream, sizeof(stream), &out, 1);
    return out;
}

typedef hipError_t (*OpenKernel)(hipStream_t, const u32 *, const u32 *, size_t, u32 *, uint8_t *);

// What the two opening calls share. consts: the viewing key; scratch: the agreed points epk * viewing_key, which never leave
// the device. `lanes`: null, or the m lanes of the call that are tried, in order: their epks and notes are gathered into
// buffers of m lanes, which the device passes read, and the results are scattered back -- every other lane keeps what the
// caller of this function put into plaintext_out / status.
int open_notes(const u64 *viewing_key, const u64 *epks, const uint8_t *sealed, size_t sealed_bytes, size_t plain_bytes,
               const std::vector<size_t> *lanes, size_t n, u64 *plaintext_out, uint8_t *status, OpenKernel kernel) {
    const int top = top_bit(viewing_key);
    const auto run = [&](const u64 *ep, const uint8_t *ct, size_t m, void *pt, uint8_t *st) {
        return run_chunks(EDWARDS_STAGING, m, viewing_key, 32,
                          {Span::in(ep, 64), Span::in(ct, sealed_bytes), Span::out(pt, plain_bytes), Span::out(st, 1)}, 64,
                          [&](const Chunk &c) {
                              u32 *key = (u32 *)c.scratch;
                              const hipError_t e = ed_mul_shared(c.stream, (const u32 *)c.a[0], c.n, (const u32 *)c.consts, top, key);
                              if (e != hipSuccess) return e;
                              return kernel(c.stream, key, (const u32 *)c.a[1], c.n, (u32 *)c.a[2], c.a[3]);
                          });
    };
    if (!lanes) return run(epks, sealed, n, plaintext_out, status);
    const size_t m = lanes->size();
    std::vector<u64> ep(m * 8);
    std::vector<uint8_t> ct(m * sealed_bytes), pt(m * plain_bytes), st(m);
    for (size_t k = 0; k < m; ++k) {
        std::memcpy(&ep[k * 8], epks + (*lanes)[k] * 8, 64);
        std::memcpy(&ct[k * sealed_bytes], sealed + (*lanes)[k] * sealed_bytes, sealed_bytes);
    }
    const int rc = run(ep.data(), ct.data(), m, pt.data(), st.data());
    if (rc != MG_OK) return rc;
    for (size_t k = 0; k < m; ++k) {
        std::memcpy((uint8_t *)plaintext_out + (*lanes)[k] * plain_bytes, &pt[k * plain_bytes], plain_bytes);
        status[(*lanes)[k]] = st[k];
    }
    return MG_OK;
}

} // namespace

int blake2s_var(const uint8_t *data, size_t len, size_t out_len, uint8_t *out) {
    if ((!data && len) || !out || out_len < 1 || out_len > 32) return MG_ERR_ARG;
    static const uint8_t none = 0;
    blake2s::hash(data ? data : &none, len, out, out_len);
    return MG_OK;
}

// decrypt: in = ciphertext | tag; the plaintext is released only behind a verified tag, else it is zeros
int aes256_gcm(const uint8_t *key, const uint8_t *nonce, const uint8_t *in, size_t len, int decrypt, uint8_t *out, int *ok) {
    if (!key || !nonce || (!in && len) || (decrypt && (len < 16 || !ok)) || len > SIZE_MAX - 16) return MG_ERR_ARG;
    const size_t body = decrypt ? len - 16 : len;
    if (!out && (body || !decrypt)) return MG_ERR_ARG;
    static const uint8_t none = 0;
    uint8_t tag[16];
    std::vector<uint8_t> text(body ? body : 1);
    aes::crypt(key, nonce, in ? in : &none, body, decrypt != 0, text.data(), tag);
    if (!decrypt) {
        std::memcpy(out, text.data(), body);
        std::memcpy(out + body, tag, 16);
        if (ok) *ok = 1;
        return MG_OK;
    }
    uint8_t diff = 0;
    for (int j = 0; j < 16; ++j) diff |= tag[j] ^ in[body + j];
    *ok = diff == 0;
    for (size_t j = 0; j < body; ++j) out[j] = diff ? 0 : text[j];
    return MG_OK;
}

int address_partitions(const mg_utxo_model *h, const u64 *recv_keys, size_t n, uint8_t *out) {
    if (!h || !lanes_ok(n) || (n && (!recv_keys || !out))) return MG_ERR_ARG;
    return run_chunks(EDWARDS_STAGING, n, nullptr, 0, {Span::in(recv_keys, 64), Span::out(out, 1)}, 0, [&](const Chunk &c) {
        return address_partition(c.stream, (const u32 *)c.a[0], c.n, c.a[1]);
    });
}

int merkle_shard_indices(int curve, const u64 *leaves, size_t n, uint8_t *out) {
    if (curve != 0 || !lanes_ok(n) || (n && (!leaves || !out))) return MG_ERR_ARG;
    return run_chunks(EDWARDS_STAGING, n, nullptr, 0, {Span::in(leaves, 32), Span::out(out, 1)}, 0, [&](const Chunk &c) {
        return merkle_shard_index(c.stream, (const u32 *)c.a[0], c.n, c.a[1]);
    });
}

// consts: the generator's table, when the ephemeral keys are asked for; scratch: the agreed points recv_key * randomness
int light_notes_encrypt(const mg_utxo_model *h, const u64 *recv_keys, const u64 *randomness, const u64 *plaintexts, size_t n,
                        u64 *epk_out, uint8_t *ciphertexts_out, uint8_t *status) {
    if (!h || !lanes_ok(n) || (n && (!recv_keys || !randomness || !plaintexts || !ciphertexts_out || !status))) return MG_ERR_ARG;
    if (!scalars_ok(randomness, n)) return MG_ERR_ARG;
    std::vector<Span> arrays = {Span::in(recv_keys, 64), Span::in(randomness, 32), Span::in(plaintexts, 96),
                                Span::out(ciphertexts_out, LIGHT_NOTE_BYTES), Span::out(status, 1)};
    if (epk_out) arrays.push_back(Span::out(epk_out, 64));
    return run_chunks(EDWARDS_STAGING, n, epk_out ? utxo_model_table(h) : nullptr, epk_out ? (size_t)ED_TABLE_WORDS * 4 : 0, arrays,
                      64, [&](const Chunk &c) {
                          const u32 *rand = (const u32 *)c.a[1];
                          u32 *key = (u32 *)c.scratch, *epk = epk_out ? (u32 *)c.a[5] : nullptr;
                          hipError_t e = hipSuccess;
                          if (epk && (e = ed_mul_fixed(c.stream, (const u32 *)c.consts, rand, c.n, epk)) != hipSuccess) return e;
                          if ((e = ed_mul_pairwise(c.stream, (const u32 *)c.a[0], rand, c.n, key)) != hipSuccess) return e;
                          return light_note_seal(c.stream, key, (const u32 *)c.a[2], c.n, epk, (u32 *)c.a[3], c.a[4]);
                      });
}

int light_notes_open(const mg_utxo_model *h, const u64 *viewing_key, const u64 *epks, const uint8_t *ciphertexts,
                     const uint8_t *partitions, size_t n, u64 *plaintext_out, uint8_t *ok, uint8_t *status, size_t *n_tried) {
    if (!h || !viewing_key || !lanes_ok(n) || (n && (!epks || !ciphertexts || !plaintext_out || !ok))) return MG_ERR_ARG;
    if (!scalar_ok(viewing_key)) return MG_ERR_ARG;
    if (n_tried) *n_tried = 0;
    if (n == 0) return MG_OK;
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    std::vector<size_t> lanes;
    if (partitions) { // `NoteOpen::open`: only the notes that carry the byte of viewing_key * G reach a key agreement
        u32 address[16];
        fixed_base_mul(utxo_model_table(h), viewing_key, address);
        const uint8_t mine = partition_of(address);
        for (size_t i = 0; i < n; ++i)
            if (partitions[i] == mine) lanes.push_back(i);
        std::memset(plaintext_out, 0, n * 96);
        std::memset(status, NOTE_OTHER_PARTITION, n);
    }
    const int rc = open_notes(viewing_key, epks, ciphertexts, LIGHT_NOTE_BYTES, 96, partitions ? &lanes : nullptr, n, plaintext_out,
                              status, light_note_open);
    if (rc != MG_OK) return rc;
    for (size_t i = 0; i < n; ++i) ok[i] = status[i] == NOTE_OK;
    if (n_tried) *n_tried = partitions ? lanes.size() : n;
    return MG_OK;
}

// consts: the generator's table | the table of the one receiving key, built on the host for this call (1 008 host additions and
// one inversion buy every lane a product of 63 gathered additions instead of a ladder of 251 doublings and additions)
int outgoing_notes_encrypt(const mg_utxo_model *h, const u64 *recv_key, const u64 *randomness, const u64 *assets, size_t n,
                           u64 *epk_out, uint8_t *ciphertexts_out, uint8_t *status) {
    if (!h || !recv_key || !lanes_ok(n) || (n && (!randomness || !assets || !epk_out || !ciphertexts_out || !status)))
        return MG_ERR_ARG;
    if (!point_ok(recv_key) || !scalars_ok(randomness, n)) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    std::vector<u32> consts(utxo_model_table(h), utxo_model_table(h) + ED_TABLE_WORDS), own_table;
    build_table(recv_key, own_table);
    consts.insert(consts.end(), own_table.begin(), own_table.end());
    return run_chunks(EDWARDS_STAGING, n, consts.data(), consts.size() * 4,
                      {Span::in(randomness, 32), Span::in(assets, 64), Span::out(epk_out, 64),
                       Span::out(ciphertexts_out, OUTGOING_NOTE_BYTES), Span::out(status, 1)},
                      64, [&](const Chunk &c) {
                          const u32 *table = (const u32 *)c.consts, *rand = (const u32 *)c.a[0];
                          u32 *key = (u32 *)c.scratch, *epk = (u32 *)c.a[2];
                          hipError_t e = ed_mul_fixed(c.stream, table, rand, c.n, epk);
                          if (e != hipSuccess) return e;
                          if ((e = ed_mul_fixed(c.stream, table + ED_TABLE_WORDS, rand, c.n, key)) != hipSuccess) return e;
                          return outgoing_note_seal(c.stream, key, (const u32 *)c.a[1], c.n, epk, (u32 *)c.a[3], c.a[4]);
                      });
}

int outgoing_notes_open(const mg_utxo_model *h, const u64 *viewing_key, const u64 *epks, const uint8_t *ciphertexts, size_t n,
                        u64 *assets_out, uint8_t *ok, uint8_t *status) {
    if (!h || !viewing_key || !lanes_ok(n) || (n && (!epks || !ciphertexts || !assets_out || !ok))) return MG_ERR_ARG;
    if (!scalar_ok(viewing_key)) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    std::vector<uint8_t> own;
    status = status_or_own(status, n, own);
    const int rc = open_notes(viewing_key, epks, ciphertexts, OUTGOING_NOTE_BYTES, 64, nullptr, n, assets_out, status,
                              outgoing_note_open);
    if (rc != MG_OK) return rc;
    for (size_t i = 0; i < n; ++i) ok[i] = status[i] == NOTE_OK;
    return MG_OK;
}

} // namespace mg
