// Staging of a host entry's arrays through device memory for the length of the call (the body is the entry's `_device` twin).
// Two layers: the layout of the parts in one allocation - plain C++, no HIP; PTK_STAGE_LAYOUT_ONLY stops there - and the staging
// object, the one place that allocates, copies in, runs the body, copies out, synchronises and frees.  Internal.
#pragma once
#include <cstddef>

namespace ptk {

// Parts are added in order; each present part starts at the next multiple of kAlign bytes (so a part of odd byte size may sit
// anywhere).  An absent part - an optional array the caller did not pass, or no elements - takes no space and reports kAbsent.
struct StageLayout {
    static constexpr size_t kAlign = 16, kAbsent = ~(size_t)0;
    size_t total = 0;                            // bytes up to the end of the last present part
    size_t add(size_t elem_bytes, size_t count, bool present = true)
    {
        if (!present || count == 0) return kAbsent;
        const size_t at = (total + kAlign - 1) / kAlign * kAlign;
        total = at + elem_bytes * count;
        return at;
    }
};

}  // namespace ptk

#ifndef PTK_STAGE_LAYOUT_ONLY
#include "ptk_ctx.h"

namespace ptk {

class Stage {
    struct Part { size_t at, bytes; const void* load; void* store; };
    ptk_ctx* c;
    StageLayout layout;
    static constexpr int kMaxParts = 17;         // (the most an entry declares: ptk_reproject_moments' fourteen planes and three outputs)
    Part parts[kMaxParts];
    int num_parts = 0;
    char* base = nullptr;

public:
    // a part's device array, once run() has allocated it: null for an absent part
    template <class T>
    struct Slot { const Stage* s; size_t at; operator T*() const { return at == StageLayout::kAbsent ? nullptr : (T*)(s->base + at); } };
    explicit Stage(ptk_ctx* ctx) : c(ctx) {}
    Stage(const Stage&) = delete;

    // `count` elements at `host` (null: the part is absent), copied in before the body when `load`, copied out behind it when `store`
    template <class T>
    Slot<T> part(const T* host, size_t count, bool load, bool store)
    {
        const size_t at = layout.add(sizeof(T), count, host != nullptr);
        if (at != StageLayout::kAbsent && num_parts++ < kMaxParts) parts[num_parts - 1] = { at, sizeof(T) * count, load ? host : nullptr, store ? (void*)host : nullptr };
        return { this, at };
    }
    template <class T> Slot<T> in(const T* host, size_t count) { return part(host, count, true, false); }
    template <class T> Slot<T> out(T* host, size_t count) { return part(host, count, false, true); }
    template <class T> Slot<T> inout(T* host, size_t count, bool load) { return part(host, count, load, true); }      // (the *_ACCUMULATE flags)

    // what a body that launches kernels itself returns
    int launched() const { const hipError_t e = hipGetLastError(); return e == hipSuccess ? PTK_OK : fail(c, PTK_ERR_HIP, hipGetErrorString(e)); }

    // One allocation, the copies in, body() -> PTK_* on the context's stream, the copies out if all went well.  Returns the body's
    // code if that is not PTK_OK, else the first HIP error, else PTK_OK.
    template <class Body>
    int run(Body&& body)
    {
        if (num_parts > kMaxParts) return fail(c, PTK_ERR_LIMIT, "staging: more present parts than Stage::parts holds");
        hipError_t e = hipMalloc(&base, layout.total ? layout.total : 1);
        if (e != hipSuccess) return fail(c, PTK_ERR_HIP, std::string("hipMalloc (staging buffer): ") + hipGetErrorString(e));
        int rc = PTK_OK;
        for (int k = 0; k < num_parts; k++)
            if (const Part& p = parts[k]; e == hipSuccess && p.load) e = hipMemcpyAsync(base + p.at, p.load, p.bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
        {
            rc = body();
            for (int k = 0; k < num_parts; k++)
                if (const Part& p = parts[k]; rc == PTK_OK && e == hipSuccess && p.store) e = hipMemcpyAsync(p.store, base + p.at, p.bytes, hipMemcpyDeviceToHost, c->stream);
        }
        const hipError_t es = hipStreamSynchronize(c->stream);      // (also on the way out of a failure: the staging buffer may be in use)
        if (e == hipSuccess) e = es;
        (void)hipFree(base); base = nullptr;
        if (rc != PTK_OK) return rc;
        if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
        return PTK_OK;
    }
};

}  // namespace ptk
#endif
