// Stand-alone check of csrc/tuning.cpp on the host, meant for a sanitized build (no HIP, no GPU, nothing loaded into Python):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imanta_rs_amd/csrc tools/tuning_check.cpp
//       manta_rs_amd/csrc/tuning.cpp -lpthread -o tools/bin/tuning_check                                    (one command)
//   for gb in 1e12 nan inf -3 3.5; do tools/bin/tuning_check $gb; done        (results: profiles/runtime_split.txt)
// argv[1] is the value of MANTA_FULL_TABLE_GB (the environment is read once per process). Exit status 0: every check held.
#include "tuning.h"
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
using namespace mg;

int main(int argc, char **argv) {
    const char *env[][2] = {{"MANTA_COALESCE", "abc"}, {"MANTA_BATCH_INFLIGHT", "2x"}, {"MANTA_GRAPH_BATCH", "bogus"}, // malformed
                            {"MANTA_PROVE_C", "99999999999"}, {"MANTA_Z3_LINEAR", ""}, {"MANTA_PROVE_STREAMS", "9"},   // too long, empty, out of range
                            {"MANTA_GRAPH", "split"}, {"MANTA_PROVE_CW", "9"}, {"MANTA_FULL_TABLE_GB", argc > 1 ? argv[1] : "1e12"}};
    for (auto &e : env) setenv(e[0], e[1], 1);
    const Tuning t = tuning(), d = tuning_defaults();
    std::printf("MANTA_FULL_TABLE_GB=%s -> graph %d/%d streams %d linear %d coalesce %d/%d batch %d qa %d dq %d c %d/%d/%d/%d table %lld\n",
                env[8][1], t.graph_mode, t.graph_mode_batch, t.prove_streams, t.linear_chains, t.coalesce_inflight, t.coalesce_gather_us,
                t.batch_inflight, t.queue_aware, t.msm_dedicated_queues, t.window_bits_narrow, t.window_bits_wide, t.window_bits_h,
                t.window_bits_g2, (long long)t.full_table_bytes);
    Tuning want = d; // only the three well-formed values apply
    want.graph_mode = GRAPH_MODE_SPLIT, want.window_bits_wide = 9;
    if (!std::strcmp(env[8][1], "3.5")) want.full_table_bytes = 3500000000ll;
    int bad = std::memcmp(&t, &want, sizeof(t)) != 0;
    // one out-of-range field per row: refused, and the values in force stay
    for (size_t off = offsetof(Tuning, graph_mode); off < sizeof(Tuning); off += 4) {
        Tuning x = d;
        const int32_t big = 100000;
        const int64_t neg = -2;
        if (off == offsetof(Tuning, full_table_bytes)) std::memcpy((char *)&x + off, &neg, 8), off += 4;
        else std::memcpy((char *)&x + off, &big, 4);
        bad += set_tuning(x) != MG_ERR_ARG || std::memcmp(&tuning(), &want, sizeof(t)) != 0;
    }
    // four readers beside one writer: every snapshot is one whole struct the writer set, and the last one is seen
    Tuning x0 = d;
    x0.batch_inflight = 1; // (coalesce_gather_us is 100: from here on every struct in force has gather = 100 * batch)
    bad += set_tuning(x0) != MG_OK;
    std::vector<std::thread> th;
    int torn[4] = {};
    for (int r = 0; r < 4; ++r)
        th.emplace_back([&torn, r] {
            for (int i = 0; i < 200000; ++i) {
                const Tuning &s = tuning();
                torn[r] += s.coalesce_gather_us != 100 * s.batch_inflight;
            }
        });
    for (int i = 0; i < 20000; ++i) {
        Tuning x = d;
        x.batch_inflight = 1 + i % 16, x.coalesce_gather_us = 100 * x.batch_inflight;
        bad += set_tuning(x) != MG_OK;
    }
    for (auto &x : th) x.join();
    bad += torn[0] + torn[1] + torn[2] + torn[3] + (tuning().batch_inflight != 1 + 19999 % 16);
    std::printf("refusals and generation counter: %s\n", bad ? "FAILED" : "ok");
    return bad != 0;
}
