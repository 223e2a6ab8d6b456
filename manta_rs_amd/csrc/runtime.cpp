// Common host runtime of the MI355X Groth16 hot path: error reporting, the per-thread timing numbers, grow-only device buffers,
// the capture lock, the per-engine MSM workspace pool and the (curve, group) engine registry. Streams: streams.cpp; tuning: tuning.cpp.
#include "engine.h"
#include <cstdio>
#include <string>

namespace mg {

static thread_local std::string g_last_error;
void set_last_hip_error(hipError_t e, const char *expr, const char *file, int line) {
    char buf[512];
    std::snprintf(buf, sizeof(buf), "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, expr);
    g_last_error = buf;
}
void set_last_error_text(const char *text) { g_last_error = text ? text : ""; }
const char *last_error_string() { return g_last_error.c_str(); }

static bool g_kernel_timing = false;
void set_kernel_timing(bool on) { g_kernel_timing = on; }
bool kernel_timing() { return g_kernel_timing; }
LastTimes &last_times() {
    static thread_local LastTimes t;
    return t;
}

int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap) return MG_OK;
    if (p) {
        hipFree(p);
        p = nullptr;
        cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256; // slack so that near-equal sizes do not thrash
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        p = nullptr;
        return hip_status(e, "hipMalloc(DevBuf)");
    }
    cap = want;
    return MG_OK;
}
void DevBuf::release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
}

std::shared_mutex &capture_mutex() {
    static std::shared_mutex mu;
    return mu;
}
static thread_local int tl_heavy_depth = 0;
HeavyOp::HeavyOp() {
    if (tl_heavy_depth++ == 0) capture_mutex().lock_shared();
}
HeavyOp::~HeavyOp() {
    if (--tl_heavy_depth == 0) capture_mutex().unlock_shared();
}

static std::atomic<int> g_graph_clients{0};
GraphClient::GraphClient() { g_graph_clients.fetch_add(1, std::memory_order_relaxed); }
GraphClient::~GraphClient() { g_graph_clients.fetch_sub(1, std::memory_order_relaxed); }
int graph_clients_alive() { return g_graph_clients.load(std::memory_order_relaxed); }

MsmWorkspace::~MsmWorkspace() {
    DevBuf *all[] = {&keys_in, &keys_out, &vals_in, &vals_out, &sort_tmp, &buckets, &pkeys[0], &pkeys[1],
                     &ppts[0], &ppts[1], &redA,     &redS,    &misc, &count, &front, &extra, &folded, &scratch};
    for (DevBuf *b : all) b->release();
    if (h_stage) hipHostFree(h_stage);
    if (h_flag) hipHostFree(h_flag);
    if (h_clk) hipHostFree(h_clk);
    if (solo) { // (drained, then pooled: never destroyed)
        (void)hipStreamSynchronize(solo);
        stream_pool_put_dedicated(solo);
    }
    if (d_token) hipFree(d_token);
    if (done) hipEventDestroy(done);
    if (t0) hipEventDestroy(t0);
    if (t1) hipEventDestroy(t1);
    if (side_fork) hipEventDestroy(side_fork);
    if (side_join) hipEventDestroy(side_join);
    if (stream) { // (drained, then pooled: never destroyed)
        (void)hipStreamSynchronize(stream);
        stream_pool_put_normal(stream);
    }
}

MsmWorkspace *GroupEngine::ws_acquire() {
    {
        std::lock_guard<std::mutex> g(ws_mu_);
        if (!ws_free_.empty()) {
            MsmWorkspace *w = ws_free_.back();
            ws_free_.pop_back();
            return w;
        }
    }
    MsmWorkspace *w = new MsmWorkspace();
    w->device = current_device();
    if (!(w->stream = stream_pool_get_normal()) ||
        hipEventCreateWithFlags(&w->done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&w->t0) != hipSuccess || hipEventCreate(&w->t1) != hipSuccess) {
        delete w;
        return nullptr;
    }
    return w;
}
// The idle pool is bounded: beyond MAX_IDLE_WS a released workspace is destroyed (its grow-only buffers are
// freed), so HBM held for past MSM sizes / dropped contexts does not accumulate.
void GroupEngine::ws_release(MsmWorkspace *w) {
    if (!w) return;
    w->use_solo = false;
    {
        std::lock_guard<std::mutex> g(ws_mu_);
        if (ws_free_.size() < MAX_IDLE_WS) {
            ws_free_.push_back(w);
            return;
        }
    }
    int prev = 0;
    hipGetDevice(&prev);
    hipSetDevice(w->device);
    delete w;
    hipSetDevice(prev);
}

// one engine per (device, curve, group): an engine's workspaces, streams and tables live on the device that was
// current when it was first asked for
GroupEngine *get_engine(int curve, int group) {
    static std::mutex mu;
    static GroupEngine *tab[MAX_DEVICES][2][2] = {};
    if (curve < 0 || curve > 1 || group < 1 || group > 2) return nullptr;
    const int dev = current_device();
    std::lock_guard<std::mutex> g(mu);
    GroupEngine *&e = tab[dev][curve][group - 1];
    if (!e) {
        if (curve == 0)
            e = group == 1 ? make_engine_bn254_g1() : make_engine_bn254_g2();
        else
            e = group == 1 ? make_engine_bls381_g1() : make_engine_bls381_g2();
    }
    return e;
}

} // namespace mg