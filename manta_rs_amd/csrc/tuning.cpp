// Tuning (tuning.h): ONE table with a row per field. The compiled-in defaults, the range check, the one-time read of the
// environment and the list behind mg_tuning_env_names are loops over it. No HIP here: a plain host compiler builds this file.
#include "tuning.h"
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>

namespace mg {
namespace {
enum Kind { INT, GRAPH, GB };
struct Field {
    size_t off;
    const char *env;
    Kind kind;
    int64_t dflt, lo, hi; // inclusive bounds
    bool zero_auto;       // 0 = the library's choice, although outside [lo, hi]
};
#define MG_TF(f) offsetof(Tuning, f)
constexpr Field FIELDS[] = {
    {MG_TF(graph_mode), "MANTA_GRAPH", GRAPH, GRAPH_MODE_SINGLE, 0, 2, false},
    {MG_TF(graph_mode_batch), "MANTA_GRAPH_BATCH", GRAPH, -1, -1, 2, false},
    {MG_TF(prove_streams), "MANTA_PROVE_STREAMS", INT, 6, 3, 6, false}, // (1 = the linear part A of the round-4 defect: -DMG_DIAG only)
    {MG_TF(linear_chains), "MANTA_Z3_LINEAR", INT, 3, 0, 3, false},
    {MG_TF(coalesce_inflight), "MANTA_COALESCE", INT, 2, 0, 4, false},
    // (0 / 40 / 80 / 150 / 300 us -> six threads 1 609 / 1 621 / 1 784 / 1 850 / 1 620 proofs/s)
    {MG_TF(coalesce_gather_us), "MANTA_COALESCE_GATHER_US", INT, 100, 0, 2000, false},
    {MG_TF(batch_inflight), "MANTA_BATCH_INFLIGHT", INT, 3, 1, 16, false},
    {MG_TF(queue_aware), "MANTA_QUEUE_AWARE", INT, 1, 0, 1, false},
    {MG_TF(msm_dedicated_queues), "MANTA_MSM_DEDICATED_QUEUES", INT, 1, 0, 2, false},
    {MG_TF(window_bits_narrow), "MANTA_PROVE_C", INT, 0, 2, 20, true},
    {MG_TF(window_bits_wide), "MANTA_PROVE_CW", INT, 0, 6, 16, true},
    {MG_TF(window_bits_h), "MANTA_PROVE_CH", INT, 0, 2, 20, true},
    {MG_TF(window_bits_g2), "MANTA_PROVE_CG2", INT, 0, 4, 18, true},
    {MG_TF(full_table_bytes), "MANTA_FULL_TABLE_GB", GB, -1, -1, INT64_MAX, false},
};
#undef MG_TF
constexpr size_t N_FIELDS = sizeof(FIELDS) / sizeof(FIELDS[0]);
constexpr size_t width(const Field &f) { return f.kind == GB ? sizeof(int64_t) : sizeof(int32_t); }
// a row per field of Tuning after struct_size, in the struct's order: the rows tile the struct
constexpr bool rows_tile_the_struct() {
    size_t at = offsetof(Tuning, graph_mode);
    for (const Field &f : FIELDS) {
        if (f.off != at) return false;
        at += width(f);
    }
    return at == sizeof(Tuning);
}
static_assert(rows_tile_the_struct(), "one row of FIELDS per field of Tuning");

struct EnvNames {
    const char *v[N_FIELDS + 2];
    constexpr EnvNames() : v{} {
        for (size_t i = 0; i < N_FIELDS; ++i) v[i] = FIELDS[i].env;
        v[N_FIELDS] = "MANTA_RCCL_LIB"; // prover.cpp: where librccl.so is (then v{}'s terminating NULL)
    }
};
constexpr EnvNames ENV_NAMES;

// (the rows tile the struct: at f.off lives an int64_t for a GB row and an int32_t for every other)
int64_t get(const Tuning &t, const Field &f) {
    const char *p = (const char *)&t + f.off;
    return f.kind == GB ? *(const int64_t *)p : *(const int32_t *)p;
}
void put(Tuning &t, const Field &f, int64_t v) { // (v is in [lo, hi] or a default: an INT or GRAPH row's fits 32 bits)
    char *p = (char *)&t + f.off;
    if (f.kind == GB) *(int64_t *)p = v;
    else *(int32_t *)p = (int32_t)v;
}
bool accepts(const Field &f, int64_t v) { return (v >= f.lo && v <= f.hi) || (f.zero_auto && v == 0); }
// the rule of tuning.h: the whole string, of the field's kind; the range is accepts()'s business
bool parse(const Field &f, const char *e, int64_t &v) {
    char *end = nullptr;
    if (f.kind == GRAPH) {
        const char *const words[] = {"off", "single", "split", "0", "1", "2"}; // GRAPH_MODE_OFF, _SINGLE, _SPLIT twice
        for (int i = 0; i < 6; ++i)
            if (!std::strcmp(e, words[i])) return v = i % 3, true;
        return false;
    }
    if (f.kind == GB) {
        const double gb = std::strtod(e, &end);
        if (end == e || *end || !std::isfinite(gb)) return false;
        if (gb < 0) return v = -1, true;
        const double bytes = gb * 1e9;
        if (!(bytes < 9223372036854775808.0)) return false; // 2^63: compared as doubles, cast only when it fits
        return v = (int64_t)bytes, true;
    }
    const long x = std::strtol(e, &end, 10); // (saturates at LONG_MAX / LONG_MIN, which the 32-bit check refuses)
    if (end == e || *end || x < INT32_MIN || x > INT32_MAX) return false;
    return v = x, true;
}

std::mutex g_mu;
Tuning g_tuning;
std::atomic<uint64_t> g_generation{0}; // of g_tuning; 0: the environment has not been read yet
// the ONE place the shipped library reads MANTA_* tuning variables
void tuning_from_env_locked() {
    g_tuning = tuning_defaults();
    for (const Field &f : FIELDS) {
        const char *e = std::getenv(f.env);
        int64_t v = 0;
        if (e && *e && parse(f, e, v) && accepts(f, v)) put(g_tuning, f, v);
    }
}
} // namespace

Tuning tuning_defaults() {
    Tuning t{};
    t.struct_size = (uint32_t)sizeof(Tuning);
    for (const Field &f : FIELDS) put(t, f, f.dflt);
    return t;
}
int normalize_tuning(Tuning &t) {
    for (const Field &f : FIELDS)
        if (!accepts(f, get(t, f))) return MG_ERR_ARG;
    t.struct_size = (uint32_t)sizeof(Tuning);
    return MG_OK;
}
const Tuning &tuning() {
    // (a snapshot per thread: contexts copy it when they are created; set_tuning may run beside readers. The lock is taken
    // only when the snapshot is older than the process-wide values.)
    static thread_local Tuning snap;
    static thread_local uint64_t snap_generation = 0;
    if (!snap_generation || snap_generation != g_generation.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> g(g_mu);
        if (!g_generation.load(std::memory_order_relaxed)) tuning_from_env_locked(), g_generation.store(1, std::memory_order_release);
        snap = g_tuning;
        snap_generation = g_generation.load(std::memory_order_relaxed);
    }
    return snap;
}
int set_tuning(const Tuning &t_in) {
    Tuning t = t_in;
    const int rc = normalize_tuning(t);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(g_mu);
    g_tuning = t;
    g_generation.fetch_add(1, std::memory_order_release); // (from 0 too: the environment no longer applies, the host has spoken)
    return MG_OK;
}
const char *const *tuning_env_names() { return ENV_NAMES.v; }

} // namespace mg
