// A stand-in for <hip/hip_runtime.h> that lets g++ compile csrc/camera_lists.hip for the host:
// the qualifiers vanish, the launch coordinates are globals the driver sets before each call, and
// the kernels then run one "thread" at a time (tests/camera_lists_host_driver.cpp). Kernels that
// synchronise (the scan) cannot run this way and are not called.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <algorithm>
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct dim3e { uint32_t x, y, z; };
static dim3e blockIdx{0,0,0}, blockDim{256,1,1}, gridDim{1,1,1}, threadIdx{0,0,0};
static inline void __syncthreads() {}
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
using std::min; using std::max; using std::sqrt; using std::fabs;
