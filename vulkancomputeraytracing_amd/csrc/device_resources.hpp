// device_resources.hpp -- move-only owners of the HIP resources the host library keeps
// (renderer_state.hpp RendererState): device buffers, pinned host buffers and events. Header-only,
// never throws; errors come back as hipError_t. Each owner releases what it holds in its destructor, in
// reset() and when it is move-assigned, so a state struct of them is torn down by assigning a
// fresh one: no list of frees to keep in step with the members. Unit-tested on the CPU against
// counting stand-ins of the HIP calls (tests/test_device_resources_cpu.py).
#pragma once

#include <cstddef>
#include <utility>

#include <hip/hip_runtime_api.h>

namespace vcrt {

namespace detail {

struct DeviceMemory {
    static hipError_t allocate(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};

struct PinnedMemory {
    static hipError_t allocate(void** p, size_t bytes) {
        return hipHostMalloc(p, bytes, hipHostMallocDefault);
    }
    static void release(void* p) { (void)hipHostFree(p); }
};

// One allocation of `Memory`, counted in elements of T.
template <typename T, typename Memory>
class Buffer {
public:
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept
        : ptr_(std::exchange(o.ptr_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            reset();
            ptr_ = std::exchange(o.ptr_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~Buffer() { reset(); }

    T* data() const { return ptr_; }
    size_t capacity() const { return cap_; }  // in elements

    void reset() {
        if (ptr_) Memory::release(ptr_);
        ptr_ = nullptr;
        cap_ = 0;
    }

    // At least n elements, kept between calls and grown only: no call at all when n fits (so
    // n == 0 leaves an empty buffer null); otherwise the old allocation is freed, its contents
    // dropped, and n elements are allocated. On failure the buffer is empty. An exactly sized
    // buffer is a reserve() on an empty one.
    hipError_t reserve(size_t n) {
        if (n <= cap_) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = Memory::allocate(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        ptr_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }

private:
    T* ptr_ = nullptr;
    size_t cap_ = 0;
};

}  // namespace detail

template <typename T>
using DeviceBuffer = detail::Buffer<T, detail::DeviceMemory>;  // hipMalloc / hipFree
template <typename T>
using PinnedBuffer = detail::Buffer<T, detail::PinnedMemory>;  // hipHostMalloc / hipHostFree

class Event {
public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            ev_ = std::exchange(o.ev_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }

    hipEvent_t get() const { return ev_; }

    // The event, created on first use (flags: hipEventDefault, or hipEventDisableTiming for one
    // that only orders work); no call when it exists.
    hipError_t create(unsigned flags = hipEventDefault) {
        if (ev_) return hipSuccess;
        const hipError_t e = flags == hipEventDefault ? hipEventCreate(&ev_)
                                                      : hipEventCreateWithFlags(&ev_, flags);
        if (e != hipSuccess) ev_ = nullptr;
        return e;
    }

    void reset() {
        if (ev_) (void)hipEventDestroy(ev_);
        ev_ = nullptr;
    }

private:
    hipEvent_t ev_ = nullptr;
};

}  // namespace vcrt
