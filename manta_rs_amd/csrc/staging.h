// Host side of the "arrays in the caller's memory in, arrays out" entry points: the device memory of one call (DevBlock), the
// chunk loop over the lanes of a call (run_chunks) and the small pieces such calls share. Host-only; no kernel lives here.
#pragma once
#include "engine.h"
#include "host_ec.h"
#include <cstring>
#include <vector>

namespace mg {

// One call's device memory: ONE hipMalloc holding all the arrays of the call, each on a 256-byte boundary -- and, when asked for,
// one hipHostMalloc of the same layout to copy through -- freed on every path out of the scope.
// The block holds the shared side of the capture lock for as long as it lives (engine.h capture_mutex: a hipMalloc / hipFree
// beside another thread's stream capture invalidates that capture), so a per-call allocation cannot exist without it. HeavyOp is
// re-entrant per thread: callers that already hold one are unaffected. A thread that CAPTURES holds the lock exclusively
// (prover_passes.h build_graphs) and must therefore never construct a block: taking the shared side would wait for itself. None
// does -- what runs inside a capture is enqueue_unit (enqueue_witness_map_body / enqueue_part_a / enqueue_msm), i.e. the Fr
// engine's passes and msm_launch on the slot's pooled workspaces, while blocks are constructed only by the host-array entry
// points of the C ABI (field, group, codec, Poseidon / Merkle and embedded-curve calls, mg_ntt), by verifying-key preparation and
// by key generation, none of which a proof pass calls. The other way round is excluded too: those entry points never prove, so
// no thread reaches build_graphs' blocking lock() with a block alive.
class DevBlock {
  public:
    DevBlock() {}
    ~DevBlock() {
        if (d_) hipFree(d_);
        if (h_) hipHostFree(h_);
    }
    DevBlock(const DevBlock &) = delete;
    DevBlock &operator=(const DevBlock &) = delete;
    // bytes[i] = the size of array i. MG_OK, or the status of the failed allocation with `what` kept for mg_last_error().
    int alloc(const std::vector<size_t> &bytes, const char *what, bool pinned = false) {
        const hipError_t e = get(bytes, pinned);
        return e == hipSuccess ? MG_OK : hip_status(e, what);
    }
    // for memory the caller can do without: false = nothing allocated and no error left behind
    bool try_alloc(const std::vector<size_t> &bytes) {
        if (get(bytes, false) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    }
    // array i on the device / in the pinned twin; an array of zero bytes is nullptr
    template <class T = uint8_t> T *dev(size_t i) const { return len_[i] ? (T *)(d_ + off_[i]) : nullptr; }
    template <class T = uint8_t> T *pin(size_t i) const { return len_[i] ? (T *)(h_ + off_[i]) : nullptr; }
    // hands the device memory to the caller, who hipFrees it (it starts at array 0)
    void *release() {
        void *p = d_;
        d_ = nullptr;
        return p;
    }

  private:
    hipError_t get(const std::vector<size_t> &bytes, bool pinned) {
        size_t total = 0;
        for (size_t b : bytes) off_.push_back(total), total += (b + 255) & ~size_t(255);
        len_ = bytes;
        hipError_t e = hipMalloc((void **)&d_, total);
        if (e != hipSuccess) d_ = nullptr;
        if (e == hipSuccess && pinned && (e = hipHostMalloc((void **)&h_, total, hipHostMallocDefault)) != hipSuccess) h_ = nullptr;
        return e;
    }
    HeavyOp no_capture_meanwhile_;
    uint8_t *d_ = nullptr, *h_ = nullptr;
    std::vector<size_t> off_, len_;
};

// ---- the chunk loop ----------------------------------------------------------------------------------------------------
struct Span { // one per-lane array of a call in the caller's memory, `stride` bytes per lane
    const void *src; // copied to the device before each chunk's launch (nullptr: output only)
    void *dst;       // copied back after it (nullptr: input only); src == dst: worked on in place, ONE device array
    size_t stride;
    static Span in(const void *p, size_t stride) { return Span{p, nullptr, stride}; }
    static Span out(void *p, size_t stride) { return Span{nullptr, p, stride}; }
    static Span inout(void *p, size_t stride) { return Span{p, p, stride}; }
};
struct Staging { // a module's recorded choices (DESIGN sections 10-12): lanes per device pass, and whether copies go through a pinned block
    size_t chunk;
    bool pinned;
};
struct Chunk { // what the launch callback gets: the device side of one chunk
    const uint8_t *consts;    // uploaded once per call, the same for every lane
    std::vector<uint8_t *> a; // the arrays, in the order of the call's spans
    uint8_t *scratch;         // scratch_stride bytes per lane
    size_t n;                 // lanes in this chunk
    hipStream_t stream;
};

// The n lanes of a call, st.chunk at a time on the calling thread's setup stream: `consts` is uploaded once, then per chunk the
// input arrays are copied in, `launch(const Chunk &) -> hipError_t` enqueues the kernels, the output arrays are copied back and
// the stream is waited for. Device memory of a call = consts + min(n, st.chunk) x (sum of the strides + scratch_stride), each
// array rounded up to 256 bytes; with st.pinned as much page-locked host memory again.
template <class Launch>
int run_chunks(Staging st, size_t n, const void *consts, size_t const_bytes, const std::vector<Span> &arrays, size_t scratch_stride,
               Launch launch) {
    if (n == 0) return MG_OK;
    hipStream_t s = setup_stream();
    if (!s) return MG_ERR_OOM;
    const size_t cap = n < st.chunk ? n : st.chunk, na = arrays.size();
    std::vector<size_t> bytes;
    for (const Span &x : arrays) bytes.push_back(cap * x.stride);
    bytes.push_back(const_bytes);
    bytes.push_back(cap * scratch_stride);
    DevBlock m;
    if (const int rc = m.alloc(bytes, "hipMalloc(chunk arrays)", st.pinned)) return rc;
    if (const_bytes) MG_HIP(hipMemcpyAsync(m.dev(na), consts, const_bytes, hipMemcpyHostToDevice, s));
    Chunk c{m.dev(na), {}, m.dev(na + 1), 0, s};
    for (size_t i = 0; i < na; ++i) c.a.push_back(m.dev(i));
    for (size_t off = 0; off < n; off += cap) {
        c.n = n - off < cap ? n - off : cap;
        for (size_t i = 0; i < na; ++i) {
            const Span &x = arrays[i];
            if (!x.src) continue;
            const void *from = (const uint8_t *)x.src + off * x.stride;
            if (st.pinned) from = std::memcpy(m.pin(i), from, c.n * x.stride);
            MG_HIP(hipMemcpyAsync(c.a[i], from, c.n * x.stride, hipMemcpyHostToDevice, s));
        }
        MG_HIP(launch(c));
        for (size_t i = 0; i < na; ++i) {
            const Span &x = arrays[i];
            if (!x.dst) continue;
            void *to = st.pinned ? m.pin(i) : (uint8_t *)x.dst + off * x.stride;
            MG_HIP(hipMemcpyAsync(to, c.a[i], c.n * x.stride, hipMemcpyDeviceToHost, s));
        }
        MG_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; st.pinned && i < na; ++i)
            if (arrays[i].dst) std::memcpy((uint8_t *)arrays[i].dst + off * arrays[i].stride, m.pin(i), c.n * arrays[i].stride);
    }
    return MG_OK;
}

// ---- small shared pieces -----------------------------------------------------------------------------------------------
// lanes whose status is not 0 (= PT_OK / MG_POINT_OK)
inline size_t count_bad(const uint8_t *status, size_t n) {
    size_t b = 0;
    for (size_t i = 0; i < n; ++i) b += status[i] != 0;
    return b;
}
// the caller's status array, or -- the argument may be NULL -- `own` sized for the call
inline uint8_t *status_or_own(uint8_t *status, size_t n, std::vector<uint8_t> &own) {
    if (status) return status;
    own.resize(n);
    return own.data();
}
// `count` field elements of 32 little-endian canonical bytes (ark-ff deserialize) -> Montgomery form, 32 bytes each at `out`
// (= the device words); false: a value >= the modulus, which is refused
template <class C> bool decode_canonical_elements(const uint8_t *bytes, size_t count, void *out) {
    typedef host::HFp<C> H;
    for (size_t i = 0; i < count; ++i) {
        H a;
        std::memcpy(a.v, bytes + 32 * i, 32);
        if (H::geq_p(a.v)) return false;
        const H m = H::to_mont(a);
        std::memcpy((uint8_t *)out + 32 * i, m.v, 32);
    }
    return true;
}

} // namespace mg
