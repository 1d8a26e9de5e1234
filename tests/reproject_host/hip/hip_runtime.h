// A stand-in for <hip/hip_runtime.h> that lets g++ compile csrc/reproject.hip for the host: the
// qualifiers vanish and the kernel runs one thread at a time (tests/reproject_host_driver.cpp), so
// a ballot holds the calling thread's bit alone and an atomic add is an add.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct float4 {
    float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
struct dim3e {
    uint32_t x, y, z;
};
extern dim3e blockIdx;
extern dim3e threadIdx;
static inline unsigned long long __ballot(int pred) {
    return pred ? 1ull << (threadIdx.x & 63u) : 0ull;
}
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __ffsll(unsigned long long v) {
    return __builtin_ffsll(static_cast<long long>(v));
}
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
    const unsigned long long old = *p;
    *p = old + v;
    return old;
}
