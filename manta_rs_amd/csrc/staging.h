// Host side of the "arrays in the caller's memory in, arrays out" entry points: the device memory of one call (DevBlock), its
// copies, launches and one wait (DevCall), the chunk loop over the lanes of a call (run_chunks) and small shared pieces. Host-only.
#pragma once
#include "engine.h"
#include "host_ec.h"
#include <cstring>
#include <type_traits>
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
    size_t bytes(size_t i) const { return len_[i]; }
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

// One call's work on the device: its block, the stream everything goes to and the first error. Every step after a failure is
// skipped, so a call is written straight down and asks once, at finish().
// The exit rule: a call that enqueued anything waits for its stream on every path out, BEFORE its memory goes -- in finish(), or,
// when a path leaves without it, in the destructor, whose body runs before the block member frees device and pinned memory.
// The lifetime rule that follows: host memory that a copy of the scope reads or writes is declared BEFORE the scope and so
// outlives it (the destructor may still be waiting for those copies when locals declared later are already gone).
// begin() asks for the stream first and the block second: where there is no device a call ends with MG_ERR_OOM, nothing allocated.
class DevCall {
  public:
    ~DevCall() {
        if (busy_) hipStreamSynchronize(s_);
    }
    // bytes[i] = the size of array i, `what` names the call in mg_last_error(), on = its stream (none: the thread's setup stream)
    int begin(const std::vector<size_t> &bytes, const char *what, bool pinned = false, hipStream_t on = nullptr) {
        what_ = what;
        if (!(s_ = on ? on : setup_stream())) return MG_ERR_OOM;
        return m_.alloc(bytes, what, pinned);
    }
    hipStream_t stream() const { return s_; }
    template <class T = uint8_t> T *dev(size_t i) const { return m_.dev<T>(i); }
    template <class T = uint8_t> T *pin(size_t i) const { return m_.pin<T>(i); }
    // host -> array i (from byte `at` on), array -> array, array i -> host, zeros -> array i; no bytes or a null side: nothing to do
    void up(size_t i, const void *src, size_t n, size_t at = 0) { cp(dev_at(i, at), src, n, hipMemcpyHostToDevice); }
    void copy(size_t to, size_t from, size_t n) { cp(dev(to), dev(from), n, hipMemcpyDeviceToDevice); }
    void down(void *dst, size_t i, size_t n, size_t at = 0) { cp(dst, dev_at(i, at), n, hipMemcpyDeviceToHost); }
    void zero(size_t i) {
        if (dev(i)) run([&] { return hipMemsetAsync(dev(i), 0, m_.bytes(i), s_); });
    }
    // `enqueue()` puts kernels on stream() and returns nothing, a hipError_t or a library status (a nested engine call, which may
    // wait for the stream itself); hipGetLastError() is read behind it. launch: one kernel, the arguments of hipLaunchKernelGGL
    template <class F> void run(F enqueue) {
        if (failed()) return;
        busy_ = true;
        if constexpr (std::is_void<decltype(enqueue())>::value) enqueue();
        else note(enqueue());
        note(hipGetLastError());
    }
    template <class Kernel, class... A> void launch(Kernel kernel, dim3 grid, dim3 block, size_t lds, A... a) {
        run([&] { hipLaunchKernelGGL(kernel, grid, block, lds, s_, a...); });
    }
    // The one wait of the call (of a chunk, in run_chunks) and its first error, a library status from inside a launch as it came
    int finish() {
        const int synced = sync_status(s_, e_, what_);
        busy_ = false;
        return rc_ ? rc_ : synced;
    }

  private:
    bool failed() const { return rc_ || e_ != hipSuccess; }
    void note(hipError_t e) { e_ = failed() ? e_ : e; }
    void note(int rc) { rc_ = failed() ? rc_ : rc; }
    uint8_t *dev_at(size_t i, size_t at) const { return dev(i) ? dev(i) + at : nullptr; }
    void cp(void *dst, const void *src, size_t n, hipMemcpyKind kind) {
        if (n && dst && src) run([&] { return hipMemcpyAsync(dst, src, n, kind, s_); });
    }
    DevBlock m_;
    hipStream_t s_ = nullptr;
    const char *what_ = "";
    hipError_t e_ = hipSuccess;
    int rc_ = MG_OK;
    bool busy_ = false; // something may be in flight on s_
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
// input arrays are copied in, `launch(const Chunk &)` enqueues the kernels (DevCall::run: a hipError_t or a library status comes
// back), the output arrays are copied back and the stream is waited for, on a failure too. Device memory of a call = consts + min(n, st.chunk) x (sum of the strides + scratch_stride), each
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
    DevCall m;
    if (const int rc = m.begin(bytes, "hipMalloc(chunk arrays)", st.pinned)) return rc;
    m.up(na, consts, const_bytes);
    Chunk c{m.dev(na), {}, m.dev(na + 1), 0, m.stream()};
    for (size_t i = 0; i < na; ++i) c.a.push_back(m.dev(i));
    for (size_t off = 0; off < n; off += cap) {
        c.n = n - off < cap ? n - off : cap;
        for (size_t i = 0; i < na; ++i) {
            const Span &x = arrays[i];
            if (!x.src) continue;
            const void *from = (const uint8_t *)x.src + off * x.stride;
            if (st.pinned) from = std::memcpy(m.pin(i), from, c.n * x.stride);
            m.up(i, from, c.n * x.stride);
        }
        m.run([&] { return launch(c); });
        for (size_t i = 0; i < na; ++i)
            if (arrays[i].dst) m.down(st.pinned ? m.pin(i) : (uint8_t *)arrays[i].dst + off * arrays[i].stride, i, c.n * arrays[i].stride);
        if (const int rc = m.finish()) return rc;
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
