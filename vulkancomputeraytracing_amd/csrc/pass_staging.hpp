// pass_staging.hpp -- the two forms of a pass behind the C ABI (image_passes.cpp, ray_passes.cpp):
// the device form runs on the caller's planes, the host form on device copies of them taken from
// one pool. Header-only over device_resources.hpp and the HIP runtime API: it reaches into no
// state, so it is unit-tested on the CPU against counting stand-ins of the HIP calls
// (tests/test_pass_staging_cpu.py).
#pragma once

#include <chrono>
#include <cstddef>
#include <initializer_list>
#include <iterator>

#include <hip/hip_runtime_api.h>

#include "device_resources.hpp"
#include "hip_status.hpp"

namespace vcrt {

// The staging storage of the host forms, kept and grown only: a call takes a buffer for every
// plane that is there, in the order it lists them, from wide[] when the plane's elements are
// multiples of 16 bytes and from narrow[] otherwise. Within a call no two planes share a buffer,
// nothing outlives the call, and every plane starts an allocation of its own (16-byte aligned,
// whatever its element size).
struct StagingPool {
    DeviceBuffer<unsigned char> wide[8], narrow[4];
};

// One plane of a call as the caller passed it: null when the plane is optional and left out.
struct Plane {
    const void* host;
    size_t elem;        // bytes per element
    bool out;           // written by the pass: downloaded after the run
    bool keep = false;  // an output written only in part: uploaded first (the caller's condition)
};
inline Plane in4(const float* p) { return {p, 16, false}; }
inline Plane out4(float* p, bool keep = false) { return {p, 16, true, keep}; }
inline Plane in1(const float* p) { return {p, 4, false}; }
inline Plane out1(float* p) { return {p, 4, true}; }

// The planes a pass runs on. The device form runs on the caller's and makes no HIP call. The host
// form takes a device plane of `count` elements from the pool for every plane that is there,
// uploads the inputs and the kept outputs, and after the run downloads the outputs and
// synchronises once. A call of no elements copies and waits for nothing.
class Staging {
public:
    Staging(StagingPool& pool, hipStream_t stream) : pool_(pool), stream_(stream) {}

    VkResult begin(bool host_form, size_t count, std::initializer_list<Plane> planes) {
        host_form_ = host_form;
        count_ = count;
        // a call wider than the pool (a bug) is refused before anything is written
        size_t wide = 0, narrow = 0;
        for (const Plane& p : planes) (p.elem % 16 == 0 ? wide : narrow) += p.host != nullptr;
        if (planes.size() > kMaxPlanes ||
            (host_form && (wide > std::size(pool_.wide) || narrow > std::size(pool_.narrow))))
            return VK_ERROR_UNKNOWN;
        wide = narrow = 0;
        for (const Plane& p : planes) {
            void* d = const_cast<void*>(p.host);
            if (host_form && p.host) {
                DeviceBuffer<unsigned char>& b =
                    p.elem % 16 == 0 ? pool_.wide[wide++] : pool_.narrow[narrow++];
                VCRT_TRY(b.reserve(count * p.elem));
                d = b.data();
                if (count && (!p.out || p.keep))
                    VCRT_TRY(hipMemcpyAsync(d, p.host, count * p.elem, hipMemcpyHostToDevice,
                                            stream_));
            }
            plane_[n_] = p;
            dev_[n_++] = d;
        }
        return VK_SUCCESS;
    }
    // plane i of the list, on the device
    template <typename T = float>
    T* at(size_t i) const {
        return static_cast<T*>(dev_[i]);
    }
    VkResult end() {
        if (!host_form_ || count_ == 0) return VK_SUCCESS;
        for (size_t i = 0; i < n_; i++)
            if (plane_[i].out && plane_[i].host)
                VCRT_TRY(hipMemcpyAsync(const_cast<void*>(plane_[i].host), dev_[i],
                                        count_ * plane_[i].elem, hipMemcpyDeviceToHost, stream_));
        VCRT_TRY(hipStreamSynchronize(stream_));
        return VK_SUCCESS;
    }

private:
    static constexpr size_t kMaxPlanes = 12;  // the pool's
    StagingPool& pool_;
    hipStream_t stream_;
    bool host_form_ = false;
    size_t count_ = 0, n_ = 0;
    Plane plane_[kMaxPlanes];
    void* dev_[kMaxPlanes];
};

// What a form checks after the pass's own argument check, in this order: for the device form the
// planes' alignment, then the renderer and its module, then the kernel.
inline vcrt_result pass_ready(bool device_planes_misaligned, bool renderer_ready,
                              hipFunction_t kernel) {
    if (device_planes_misaligned || !renderer_ready) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (!kernel) return VCRT_ERROR_FEATURE_NOT_PRESENT;
    return VCRT_SUCCESS;
}

// The end of every form: after a good run the outputs come back and the call's time is taken.
template <typename Stats>
vcrt_result finish(VkResult ran, Staging& s, Stats* stats,
                   std::chrono::steady_clock::time_point t0) {
    if (ran != VK_SUCCESS) return ran;
    const VkResult r = s.end();
    if (r != VK_SUCCESS) return r;
    if (stats)
        stats->host_ms = std::chrono::duration<double, std::milli>(
                             std::chrono::steady_clock::now() - t0).count();
    return VCRT_SUCCESS;
}

}  // namespace vcrt
