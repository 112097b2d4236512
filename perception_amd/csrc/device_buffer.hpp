// device_buffer.hpp - the owning buffer types of a context: DevBuf<T> (device memory) and PinBuf<T> (pinned host memory).
//
// A buffer frees its memory when it is destroyed, knows how many elements it holds and converts to T*, so that kernel
// arguments, subscripts and pointer arithmetic read as they would with a raw pointer (a C-style cast to another pointer type
// needs get()).  These two types and the guard helpers are the only callers of the runtime's allocation functions.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace cd {

#ifdef CD_ALLOC_GUARD
// Debug build (make VARIANT=guard FLAGS_EXTRA=-DCD_ALLOC_GUARD=262144): every device allocation of the library gets that many
// bytes of 0xA5 behind it, checked when it is freed - a kernel that WRITES past the end of an array is named on stderr instead
// of corrupting its neighbour (or faulting only when the neighbour happens to be unmapped); a kernel that only READS past the
// end stops faulting and leaves the guards intact, which says as much.
struct GuardEntry { void* p; size_t bytes; std::string name; };
inline std::mutex g_guard_mu;
inline std::vector<GuardEntry> g_guards;
inline hipError_t guard_malloc(void** p, size_t bytes, const char* name) {
    const hipError_t e = hipMalloc(p, bytes + (size_t)CD_ALLOC_GUARD);
    if (e != hipSuccess) return e;
    (void)hipMemset((char*)*p + bytes, 0xA5, (size_t)CD_ALLOC_GUARD);
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guards.push_back(GuardEntry{*p, bytes, name});
    return hipSuccess;
}
inline hipError_t guard_free(void* p) {
    GuardEntry ge{nullptr, 0, ""};
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        for (size_t i = 0; i < g_guards.size(); ++i)
            if (g_guards[i].p == p) { ge = g_guards[i]; g_guards.erase(g_guards.begin() + (long)i); break; }
    }
    if (ge.p) {
        std::vector<unsigned char> h((size_t)CD_ALLOC_GUARD);
        (void)hipDeviceSynchronize();
        if (hipMemcpy(h.data(), (char*)p + ge.bytes, h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
            size_t first = h.size(), last = 0, bad = 0;
            for (size_t i = 0; i < h.size(); ++i) if (h[i] != 0xA5) { if (first == h.size()) first = i; last = i; ++bad; }
            if (bad) std::fprintf(stderr, "cuboid_hip GUARD: %s (%zu bytes) was written past its end: %zu bytes between +%zu and +%zu\n", ge.name.c_str(), ge.bytes, bad, first, last);
        }
    }
    return hipFree(p);
}
#endif

struct DeviceMem {
#ifdef CD_ALLOC_GUARD
    static hipError_t get(void** p, size_t bytes, const char* name) { return guard_malloc(p, bytes, name); }
    static void give(void* p) { (void)guard_free(p); }
#else
    static hipError_t get(void** p, size_t bytes, const char*) { return hipMalloc(p, bytes); }
    static void give(void* p) { (void)hipFree(p); }
#endif
};
struct PinnedMem {
    static hipError_t get(void** p, size_t bytes, const char*) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void give(void* p) { (void)hipHostFree(p); }
};

template <class T, class Mem>
class OwnedBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;   // elements

public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    OwnedBuf& operator=(OwnedBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~OwnedBuf() { release(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
    void release() {
        if (p_) Mem::give(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // n elements, at least one; what the buffer held is freed.  name: the member's name (the guard build reports it)
    hipError_t alloc(size_t n, const char* name) {
        release();
        n = std::max<size_t>(n, 1);
        const hipError_t e = Mem::get((void**)&p_, n * sizeof(T), name);
        if (e == hipSuccess) cap_ = n; else p_ = nullptr;
        return e;
    }
    // grows the buffer to hold `need` elements (its contents are not kept); the stream is synchronised first, as work in
    // flight may still read the old memory
    hipError_t ensure(hipStream_t stream, size_t need, const char* name) {
        if (need <= cap_) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(stream);
        return e != hipSuccess ? e : alloc(need, name);
    }
};
template <class T> using DevBuf = OwnedBuf<T, DeviceMem>;
template <class T> using PinBuf = OwnedBuf<T, PinnedMem>;

}  // namespace cd
