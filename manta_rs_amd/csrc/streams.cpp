// Every stream the library creates, except the engines' process-lifetime side streams (msm_engine.h): three pools of one type,
// the calling thread's setup stream, and the queue-aware stream sets of single-proof slots.
//
// THE RULE: streams are pooled for the life of the process and NEVER destroyed; there is no hipStreamDestroy on any product path.
// It works around one defect of the HIP runtime this library is loaded next to (libamdhip64 of ROCm 7.0,
// hip::Graph::UpdateStreams): when a multi-branch graph is launched, the exec's internal parallel streams that share a hardware
// queue with the launch stream are skipped, but only ONE spare stream exists -- if two of them alias the launch stream's queue the
// loop reads past the vector and hipGraphLaunch segfaults (seen about once in ten processes after contexts had come and gone;
// stream destruction unbalances the queue use counts and made it 7 in 8). Round 5, tools/soak.py with a context recycled every
// 2 s, reached it through the MSM workspaces: the engine's idle pool overflowed, workspaces were deleted, their streams destroyed --
// and the process died within a minute with "free(): corrupted unsorted chunks" (or answered MG_ERROR_HIP under a debugger's timing).
//
// (The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues, default 4; streams that share one
// serialise. The library leaves the variable alone: measured on MI355X, PrivateTransfer shape, 6 queues against 4 give
// +6 % batched proofs/s and -4 % sequential latency in a process that only proves (tools/hw_queues_sweep.sh) but -20 % for
// two threads of single proofs and nothing for the batched stream inside bench.py's process; 8 queues halve everything.)
#include "engine.h"
#include "tuning.h"
#include <hip/hip_ext.h>
#include <map>

namespace mg {

int current_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MAX_DEVICES) return 0;
    return d;
}

namespace {
std::mutex g_stream_mu;
// Streams of one kind: idle ones per device (a stream belongs to the device it was created on), and the device of every stream the
// pool has created. A stream is created only on a miss, outside the lock, on the caller's current device.
struct StreamPool {
    hipStream_t (*const create)();
    const bool latch_refusal; // a device whose create() failed once is not asked again
    std::vector<hipStream_t> idle[MAX_DEVICES];
    std::map<hipStream_t, int> dev;
    bool refused[MAX_DEVICES] = {};

    hipStream_t get() {
        const int d = current_device();
        {
            std::lock_guard<std::mutex> g(g_stream_mu);
            if (refused[d]) return nullptr;
            if (!idle[d].empty()) {
                hipStream_t s = idle[d].back();
                idle[d].pop_back();
                return s;
            }
        }
        hipStream_t s = create();
        std::lock_guard<std::mutex> g(g_stream_mu);
        if (s) dev[s] = d;
        else if (latch_refusal) (void)hipGetLastError(), refused[d] = true;
        return s;
    }
    void put(hipStream_t s) {
        if (!s) return;
        std::lock_guard<std::mutex> g(g_stream_mu);
        auto it = dev.find(s);
        // (a stream this pool did not create: no caller has one today. It is dropped, which leaks it -- not filed under a device
        // that may not be its own, and not destroyed)
        if (it != dev.end()) idle[it->second].push_back(s);
    }
};

// Proof-slot streams (the streams graphs are captured from and launched on) are HIGH-PRIORITY: the exec's internal streams of the
// defect above are normal-priority; a high-priority launch stream lives in the other hardware-queue pool and can never alias them.
hipStream_t create_high() {
    hipStream_t s = nullptr;
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return nullptr;
    return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi) == hipSuccess ? s : nullptr;
}
// NORMAL priority: MSM workspaces (the branch streams of a proof slot's forked capture) and every other short-lived stream
hipStream_t create_normal() {
    hipStream_t s = nullptr;
    return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? s : nullptr;
}
StreamPool g_high{create_high, false}, g_normal{create_normal, false};

// a stream on a hardware queue of its own (engine.h MsmWorkspace::solo)
hipStream_t create_dedicated() {
    const int dev = current_device();
    // The runtime's pool of shared normal-priority hardware queues must be FULL before the first dedicated queue exists: a process
    // that has created fewer ordinary streams than the pool holds (the runtime's GPU_MAX_HW_QUEUES, default 4) otherwise finds the dedicated queue
    // counted as a pool member, and later ordinary streams -- the NULL stream included -- are multiplexed onto it (measured: 316
    // Mscalar/s in a process with no foreign stream, 379-387 with two or more: profiles/r06_pipeline_phase.txt). Eight ordinary
    // streams are created once per device and kept in the library's normal-priority pool.
    {
        static std::mutex prime_mu;
        static bool primed[MAX_DEVICES] = {};
        std::lock_guard<std::mutex> g(prime_mu);
        if (!primed[dev]) {
            primed[dev] = true;
            hipStream_t fill[8] = {}; // (GPU_MAX_HW_QUEUES is 4 by default; a host that raised it to 8 is covered too)
            for (hipStream_t &f : fill)
                if (!(f = create_normal())) break;
            (void)hipGetLastError();
            std::lock_guard<std::mutex> g2(g_stream_mu);
            for (hipStream_t f : fill)
                if (f) g_normal.dev[f] = dev, g_normal.idle[dev].push_back(f);
        }
    }
    int cus = 0;
    hipStream_t s = nullptr;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
        std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u); // every CU: the point is the queue, not the mask
        for (int b = 0; b < cus; ++b) mask[(size_t)b / 32] |= 1u << (b % 32);
        if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) s = nullptr;
    }
    return s; // (nullptr: refused, latched by the pool -- the MSMs use their ordinary streams)
}
StreamPool g_dedicated{create_dedicated, true};
} // namespace

hipStream_t stream_pool_get() { return g_high.get(); }
void stream_pool_put(hipStream_t s) { g_high.put(s); }
hipStream_t stream_pool_get_normal() { return g_normal.get(); }
void stream_pool_put_normal(hipStream_t s) { g_normal.put(s); }
hipStream_t stream_pool_get_dedicated() {
    // (0: never -- e.g. hosts that need non-blocking semantics against their own NULL-stream work. Process-wide: a stand-alone MSM has no context)
    return tuning().msm_dedicated_queues ? g_dedicated.get() : nullptr;
}
void stream_pool_put_dedicated(hipStream_t s) { g_dedicated.put(s); }

// ---- the calling thread's setup stream (engine.h): one pooled normal-priority non-blocking stream per device it has touched
hipStream_t setup_stream() {
    struct ThreadSetupStreams {
        hipStream_t s[MAX_DEVICES] = {};
        ~ThreadSetupStreams() {
            for (hipStream_t x : s)
                if (x) stream_pool_put_normal(x); // (idle: every user waits for its own work before it returns)
        }
    };
    static thread_local ThreadSetupStreams tl;
    const int dev = current_device();
    if (!tl.s[dev]) tl.s[dev] = stream_pool_get_normal();
    return tl.s[dev];
}

// ---- queue-aware stream sets (see queues.hip) -------------------------------------------------------------------------------
namespace {
struct QueueClasses {
    std::vector<hipStream_t> rep;               // one stream of every hardware queue seen so far
    std::vector<std::vector<hipStream_t>> idle; // pooled streams by queue
    std::map<hipStream_t, int> cls;
};
struct DevQueues {
    QueueClasses pr[2]; // 0: normal priority, 1: high priority (the two levels have hardware queues of their own)
    std::vector<char> set_used;
    unsigned *mem = nullptr, token = 0;
    bool failed = false, ready = false;
    int probes = 0;
};
constexpr int PROBE_RETRIES = 4;
DevQueues g_q[MAX_DEVICES];
std::mutex g_q_mu;
// creates one stream of priority level pr, finds its queue and pools it; returns the class or -1
int add_classified_stream(DevQueues &q, int pr) {
    QueueClasses &c = q.pr[pr];
    hipStream_t s = pr ? create_high() : create_normal();
    if (!s) return -1;
    int found = -1;
    for (size_t k = 0; k < c.rep.size() && found < 0; ++k) {
        const int r = streams_share_queue(c.rep[k], s, q.mem, &q.token);
        if (r < 0) return -1; // (the stream is leaked: the library destroys none)
        if (r == 1) found = (int)k;
    }
    if (found < 0) { // the first stream seen on a queue stays the library's own: later probes run on it, never inside a user's work
        c.rep.push_back(s);
        c.idle.emplace_back();
        return (int)c.rep.size() - 1;
    }
    c.cls[s] = found;
    c.idle[found].push_back(s);
    return found;
}
hipStream_t take_in_class(DevQueues &q, int pr, int want) {
    QueueClasses &c = q.pr[pr];
    const int n = (int)c.rep.size();
    if (n == 0) return nullptr;
    want %= n;
    for (int tries = 0; c.idle[want].empty() && tries < 4 * n + 4; ++tries)
        if (add_classified_stream(q, pr) < 0) return nullptr;
    if (c.idle[want].empty()) return nullptr;
    hipStream_t s = c.idle[want].back();
    c.idle[want].pop_back();
    return s;
}
void give_back(DevQueues &q, int pr, hipStream_t s) {
    if (!s) return;
    auto it = q.pr[pr].cls.find(s);
    if (it != q.pr[pr].cls.end()) q.pr[pr].idle[it->second].push_back(s);
}
// the hardware queues of the current device are known (probed on the first call: ~20 ms); false: the probe failed
bool sets_ready_locked(DevQueues &q) {
    if (q.failed) return false;
    if (!q.ready) {
        // twelve streams per level: with the runtime's least-used-queue rule that is three per hardware queue, one of them kept for probes
        if (!q.mem) {
            q.failed = hipHostMalloc((void **)&q.mem, 64) != hipSuccess;
            if (!q.failed) q.mem[0] = q.mem[1] = 0;
        }
        for (int pr = 0; pr < 2 && !q.failed; ++pr)
            for (int i = 0; i < 12 && !q.failed; ++i) q.failed = add_classified_stream(q, pr) < 0;
        // fewer than three high-priority queues: a slot cannot have three of its own
        if (!q.failed) q.failed = q.pr[1].rep.size() < 3 || q.pr[0].rep.empty();
        if (q.failed) {
            (void)hipGetLastError();
            // not latched for the life of the process: a probe that ran on a busy GPU (fewer than three high-priority classes
            // seen) is repeated by a later context, at most PROBE_RETRIES times (the streams of a failed probe stay in the classes
            // they were put in; the library destroys none)
            if (++q.probes < PROBE_RETRIES) q.failed = false;
            return false;
        }
        q.ready = true;
    }
    return true;
}
} // namespace
bool stream_sets_ready() {
    const int dev = current_device();
    HeavyOp probes_synchronise_streams; // (not beside a capture)
    std::lock_guard<std::mutex> g(g_q_mu);
    return sets_ready_locked(g_q[dev]);
}
int stream_queue_counts(int *normal, int *high) {
    const int dev = current_device();
    std::lock_guard<std::mutex> g(g_q_mu);
    if (!g_q[dev].ready) return 0;
    *normal = (int)g_q[dev].pr[0].rep.size(), *high = (int)g_q[dev].pr[1].rep.size();
    return 1;
}
bool stream_set_acquire(StreamSet &out, bool z3_high) {
    const int dev = current_device();
    HeavyOp probes_synchronise_streams;
    std::lock_guard<std::mutex> g(g_q_mu);
    DevQueues &q = g_q[dev];
    if (!sets_ready_locked(q)) return false;
    size_t id = 0;
    while (id < q.set_used.size() && q.set_used[id]) ++id;
    if (id == q.set_used.size()) q.set_used.push_back(0);
    const int i = (int)id;
    hipStream_t a = take_in_class(q, 1, 2 * i), b = take_in_class(q, 1, 2 * i + 1);
    hipStream_t c = z3_high ? take_in_class(q, 1, 2 * i + 2) : take_in_class(q, 0, i);
    if (!a || !b || !c) {
        give_back(q, 1, a), give_back(q, 1, b), give_back(q, z3_high ? 1 : 0, c);
        (void)hipGetLastError();
        return false;
    }
    q.set_used[id] = 1;
    out.main = a, out.g2 = b, out.z3 = c, out.id = i, out.dev = dev, out.z3_high = z3_high;
    return true;
}
void stream_set_release(StreamSet &s) {
    if (s.id < 0) return;
    std::lock_guard<std::mutex> g(g_q_mu);
    DevQueues &q = g_q[s.dev];
    give_back(q, 1, s.main), give_back(q, 1, s.g2), give_back(q, s.z3_high ? 1 : 0, s.z3);
    if ((size_t)s.id < q.set_used.size()) q.set_used[s.id] = 0;
    s = StreamSet();
}

} // namespace mg
