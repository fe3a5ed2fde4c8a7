// rt_devbuf.h -- owners of what the host side allocates from HIP: device / pinned buffers, events, streams.  Each releases
// in its destructor, so a struct made of them needs no hand-kept list to free.  Nothing here synchronises: the caller drains
// whatever may still use a buffer before it lets one grow.
#pragma once
#include <hip/hip_runtime.h>

template <typename T, bool Pinned = false>
struct DevBuf {
    T *ptr = nullptr;
    size_t cap = 0;                        // elements; 0 whenever ptr is null, so a failed grow is retried by the next call
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { (void)release(); }
    operator T *() const { return ptr; }
    bool holds(size_t count) const { return ptr && count <= cap; }
    hipError_t release() {
        T *p = ptr;
        ptr = nullptr;
        cap = 0;
        if (!p) return hipSuccess;
        return Pinned ? hipHostFree(p) : hipFree(p);
    }
    // At least `count` elements (one when count is 0); the contents do not survive a reallocation.
    hipError_t grow(size_t count) {
        if (holds(count)) return hipSuccess;
        hipError_t e = release();
        if (e != hipSuccess) return e;
        const size_t n = count ? count : 1;
        e = Pinned ? hipHostMalloc((void **)&ptr, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&ptr, n * sizeof(T));
        if (e != hipSuccess) {
            ptr = nullptr;
            return e;
        }
        cap = n;
        return hipSuccess;
    }
    void swap(DevBuf &o) {
        T *p = ptr; ptr = o.ptr; o.ptr = p;
        size_t n = cap; cap = o.cap; o.cap = n;
    }
};
template <typename T>
using PinnedBuf = DevBuf<T, true>;

struct DevEvent {
    hipEvent_t ev = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    ~DevEvent() { if (ev) (void)hipEventDestroy(ev); }
    operator hipEvent_t() const { return ev; }
    hipError_t create(unsigned flags) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }   // once; later calls keep it
};

struct DevStream {
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream &) = delete;
    DevStream &operator=(const DevStream &) = delete;
    ~DevStream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

// Last use of a context-owned scratch that post passes on any stream work in (rt_bloom's ping-pong targets, rt_ssao's depth
// plane).  The scratch is one per context, so its users run one after another: a pass orders its stream behind the previous
// use (acquire), launches, and records its own (release).  Every use waits for the one before it, so the event of the last
// one stands for all of them: the host waits on it alone before the scratch is freed (drain).  Nothing here blocks the host
// in steady state; behind a use on the same stream the wait is already met by stream order.
struct ScratchUse {
    DevEvent ev;
    bool used = false;
    hipError_t create() { return ev.create(hipEventDisableTiming); }
    hipError_t acquire(hipStream_t s) { return used ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
    hipError_t release(hipStream_t s) {
        used = true;
        return hipEventRecord(ev, s);
    }
    hipError_t drain() { return used ? hipEventSynchronize(ev) : hipSuccess; }
};
