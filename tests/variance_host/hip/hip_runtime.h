// A stand-in for <hip/hip_runtime.h> that lets g++ compile csrc/variance.hip for the host: the
// qualifiers vanish; a ballot holds the calling thread's bit alone; the direct kernels run one
// thread at a time, an LDS kernel's workgroup as 256 host threads (threadIdx is thread-local,
// __syncthreads a barrier the driver owns, an atomic add is one) and the dynamic LDS is an array
// the driver defines (tests/variance_host_driver.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__
#define __align__(x)
struct float4 {
    float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
struct dim3e {
    uint32_t x, y, z;
};
extern dim3e blockIdx;
extern thread_local dim3e threadIdx;
void __syncthreads();
static inline unsigned long long __ballot(int pred) {
    return pred ? 1ull << (threadIdx.x & 63u) : 0ull;
}
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __ffsll(unsigned long long v) {
    return __builtin_ffsll(static_cast<long long>(v));
}
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
    return __atomic_fetch_add(p, v, __ATOMIC_RELAXED);  // (the LDS kernels' threads run together)
}
