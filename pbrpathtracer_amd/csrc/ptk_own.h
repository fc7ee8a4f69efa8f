// Owners of what a context holds in the HIP runtime: device buffers, page-locked words, streams, events.  Each destructor releases
// what the owner holds, none can be copied; ptk_ctx's members are of these types, so `delete c` frees them (ptk_ctx.h).  The members
// that need the context (its error text, stream and device) are defined at the end of ptk_ctx.h.  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

struct ptk_ctx;

namespace ptk {

// A device buffer with its capacity, in the unit its user counts in (elements, pixels, bytes).  Reads as the pointer it holds.
template <class T>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    operator T*() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    void adopt(T* q, size_t n = 0) { release(); p = q; cap = n; }       // takes over an allocation made elsewhere
    // a fresh buffer of `bytes` bytes, capacity n: the bare attempt (a caller that retries with less), and with the context's error text
    hipError_t try_alloc(size_t bytes, size_t n) { release(); const hipError_t e = hipMalloc(&p, bytes); if (e == hipSuccess) cap = n; else p = nullptr; return e; }
    int alloc_bytes(ptk_ctx* c, size_t bytes, size_t n);
    int alloc(ptk_ctx* c, size_t n, size_t extra = 0) { return alloc_bytes(c, n * sizeof(T) + extra, n); }
    // "Grow to the largest call so far": at least `want` elements of `bytes_per` bytes + `extra` bytes.  The stream that uses the buffer
    // (the context's, unless named) is drained before the old buffer is freed; a refused allocation leaves null, capacity 0.
    int grow(ptk_ctx* c, size_t want, size_t bytes_per, size_t extra = 0, hipStream_t user = nullptr);
};

// Page-locked host words: the source or target of a small asynchronous copy.
template <class T>
struct Pinned {
    T* p = nullptr;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    operator T*() const { return p; }
    hipError_t alloc(size_t n) { return p ? hipSuccess : hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault); }
};

// A stream the context made.  It is drained before it goes.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { release(); }
    operator hipStream_t() const { return s; }
    hipError_t create(unsigned flags, int priority = 0) { return hipStreamCreateWithPriority(&s, flags, priority); }
    void sync() const { if (s) (void)hipStreamSynchronize(s); }
    void release() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); s = nullptr; } }
};

// One event.  Ordering events are made once with hipEventDisableTiming; timing events by the timers below.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};
// milliseconds from event a to event b, once b has happened
int event_ms(ptk_ctx* c, hipEvent_t a, hipEvent_t b, float* ms);

// The N timing events of an entry's last call, each made on first use.  `timed` is 0 while they hold no finished call - every time
// then reads zero - and the stage the call reached otherwise (1, unless the entry counts further).
template <int N>
struct Timer {
    Event ev[N];
    int timed = 0;
    void begin() { timed = 0; }
    int mark(ptk_ctx* c, int k, hipStream_t s);          // records event k on s
    void done(int stage = 1) { timed = stage; }
    int elapsed(ptk_ctx* c, int a, int b, float* ms) { *ms = 0.0f; return timed ? event_ms(c, ev[a], ev[b], ms) : 0; }
    // t[k]: from event first + k to the next one, for n intervals
    int spans(ptk_ctx* c, int first, int n, float* t)
    {
        int rc = 0;
        for (int k = 0; k < n && rc == 0; k++) rc = elapsed(c, first + k, first + k + 1, &t[k]);
        return rc;
    }
};

// Three timing events per timed pass (or block) of an entry's last call: before the first kernel, behind it, behind the second.
// `passes` counts the passes whose events were recorded; `timed` as above.
struct PassTimer {
    std::vector<Event> ev;
    int passes = 0, timed = 0;
    void begin() { passes = 0; timed = 0; }
    int reserve(ptk_ctx* c, int n);                      // makes the events of the first n passes
    hipEvent_t at(int pass, int k) const { return ev[(size_t)pass * 3 + k]; }
    // adds pass i's two intervals to *first and *second (either may be null)
    int add(ptk_ctx* c, int i, float* first, float* second);
};

}  // namespace ptk
