// A stand-in for <hip/hip_runtime.h> that lets g++ compile csrc/denoise.hip for the host: the
// qualifiers vanish, a workgroup runs as 256 host threads (threadIdx is thread-local,
// __syncthreads a barrier the driver owns) and the dynamic LDS is an array the driver defines
// (tests/denoise_host_driver.cpp).
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
