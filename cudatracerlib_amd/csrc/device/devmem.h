// devmem.h — the owners of device and pinned host memory (host code only).
// They never synchronise and never report: the call site drains what still
// reads an old allocation before it grows, and words its own error.  A failed
// allocation leaves HIP's last error consumed, so a later hipGetLastError()
// after a launch cannot take it for the launch's.  Structs that go to kernels
// by value keep raw pointers, filled from get().
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace ctl {

inline hipError_t consumed(hipError_t e) {
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}
struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return consumed(hipMalloc(p, bytes)); }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return consumed(hipHostMalloc(p, bytes, hipHostMallocDefault)); }
    static void free(void* p) { (void)hipHostFree(p); }
};

// An owning, move-only array of T that only grows: pointer + capacity in elements.
template <class T, class Mem>
class MemArray {
    T* p_ = nullptr;
    size_t cap_ = 0;

public:
    MemArray() = default;
    MemArray(MemArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    MemArray& operator=(MemArray&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~MemArray() { reset(); }

    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    bool fits(size_t n) const { return n <= cap_; }
    void reset() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Frees the old allocation, then allocates n * sizeof(T) + pad_bytes (the
    // contents are not kept).  On failure the array is empty.
    hipError_t grow(size_t n, size_t pad_bytes = 0) {
        reset();
        void* p = nullptr;
        const hipError_t e = Mem::alloc(&p, n * sizeof(T) + pad_bytes);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }
};
template <class T> using DevArray = MemArray<T, DeviceMem>;
template <class T> using PinnedArray = MemArray<T, PinnedMem>;

// Device allocations that live as long as the pool; the raw pointers go into
// the caller's structs (often kernel arguments).
class DevPool {
    std::vector<void*> all_;

public:
    DevPool() = default;
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;
    ~DevPool() { clear(); }

    template <class T>
    hipError_t alloc(T** p, size_t n, size_t pad_bytes = 0) {
        void* q = nullptr;
        const hipError_t e = DeviceMem::alloc(&q, n * sizeof(T) + pad_bytes);
        if (e != hipSuccess) return e;
        all_.push_back(q);
        *p = static_cast<T*>(q);
        return hipSuccess;
    }
    void release(void* p) {   // frees the one entry p, if it is the pool's
        auto it = std::find(all_.begin(), all_.end(), p);
        if (it == all_.end()) return;
        DeviceMem::free(p);
        all_.erase(it);
    }
    void clear() {
        for (void* p : all_) DeviceMem::free(p);
        all_.clear();
    }
};

// An event, created on demand and destroyed with its owner.
class Event {
    hipEvent_t e_ = nullptr;

public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e_, flags); }
    operator hipEvent_t() const { return e_; }
};

}  // namespace ctl
