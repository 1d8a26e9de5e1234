// reproject.hip -- temporal accumulation (include/vcrt.h vcrt_reproject, the definition;
// csrc/reproject.cpp vcrt_reproject_host, the same on the host): one launch per call, gfx950.
//
// One lane owns one output pixel: it reads its motion vector and its new colour, gathers the
// previous output bilinearly at the reprojected position from the taps whose surface key, history
// length and depth agree, and blends. The four taps run in the order (0,0), (1,0), (0,1), (1,1),
// every fp32 operation rounded on its own (no contraction, correctly rounded division), so the
// planes' bits depend on the inputs and the parameters only. A wave covers a 64-pixel segment of a
// row: the pixel's own planes are one coalesced 16-B load per lane, and since neighbours move
// alike a tap's loads are nearly so. A tap's colour is loaded only once it is accepted.
// Bounds: the position is tested against (-1, W) x (-1, H) first -- a NaN fails every comparison
// -- so floorf gives -1 .. W - 1 and -1 .. H - 1, exact in int32; every tap is then tested in x
// and y before any plane is read at it. Pixel indices stay below 2^26.
#include <hip/hip_runtime.h>

#include "reproject_abi.h"

#pragma clang fp contract(off)

using namespace vcrt;

namespace {

constexpr float kDepthEps = 0x1p-20f;  // the relative depth's denominator never vanishes

__device__ __forceinline__ float4 ld4(const float* plane, size_t i) {
    return reinterpret_cast<const float4*>(plane)[i];
}

struct History {
    float r, g, b, l, w;
};

// One tap: vcrt.h's b, the three tests and the five sums, in that order. (qx, qy) may lie outside
// the frame: then nothing is read.
__device__ __forceinline__ void tap(const ReprojectParams& p, float4 m, float b, int32_t qx,
                                    int32_t qy, History& acc) {
    if (b == 0.0f) return;
    if (qx < 0 || qy < 0 || qx >= static_cast<int32_t>(p.width) ||
        qy >= static_cast<int32_t>(p.height))
        return;
    const size_t q = static_cast<size_t>(qy) * p.width + static_cast<size_t>(qx);
    const float4 s_q = ld4(p.history_surface, q);
    if (!(s_q.x == m.w)) return;
    const float l_q = p.history_length[q];
    if (!(l_q >= 1.0f)) return;
    if (m.w != 1.0f && p.depth_tolerance != 0.0f) {
        const float num = fabsf(m.z - s_q.y);
        float den = fabsf(m.z) + fabsf(s_q.y);
        den = den + kDepthEps;
        if (!(num / den <= p.depth_tolerance)) return;
    }
    const float4 c_q = ld4(p.history_colour, q);
    acc.r = acc.r + b * c_q.x;
    acc.g = acc.g + b * c_q.y;
    acc.b = acc.b + b * c_q.z;
    acc.l = acc.l + b * l_q;
    acc.w = acc.w + b;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(vcrt::kReprojectThreads)
vcrt_reproject_pass(ReprojectParams p) {
    const uint32_t bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const uint32_t x = bx * kReprojectRowW + (threadIdx.x % kReprojectRowW);
    const uint32_t y = by * kReprojectRowH + (threadIdx.x / kReprojectRowW);
    if (x >= p.width || y >= p.height) return;
    const size_t gp = static_cast<size_t>(y) * p.width + x;
    const float4 m = ld4(p.motion, gp);
    const float4 c = ld4(p.colour, gp);
    const float W = static_cast<float>(p.width), H = static_cast<float>(p.height);
    History acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (m.w >= 1.0f && m.x > -1.0f && m.x < W && m.y > -1.0f && m.y < H) {
        const float fx = floorf(m.x), fy = floorf(m.y);
        const float ax = m.x - fx, ay = m.y - fy;
        const float bx0 = 1.0f - ax, by0 = 1.0f - ay;
        const int32_t ix = static_cast<int32_t>(fx), iy = static_cast<int32_t>(fy);
        tap(p, m, bx0 * by0, ix, iy, acc);
        tap(p, m, ax * by0, ix + 1, iy, acc);
        tap(p, m, bx0 * ay, ix, iy + 1, acc);
        tap(p, m, ax * ay, ix + 1, iy + 1, acc);
    }
    const bool took = acc.w > 0.0f;
    float4 o = c;
    float n = 1.0f;
    if (took) {
        const float hr = acc.r / acc.w, hg = acc.g / acc.w, hb = acc.b / acc.w;
        const float l = acc.l / acc.w;
        n = fminf(l + 1.0f, p.max_history);
        const float a = fmaxf(p.alpha, 1.0f / n);
        o.x = hr + a * (c.x - hr);
        o.y = hg + a * (c.y - hg);
        o.z = hb + a * (c.z - hb);
    }
    reinterpret_cast<float4*>(p.out)[gp] = o;
    p.out_length[gp] = n;
    if (p.tallies) {
        // per wave: the lanes inside the frame are here together, the first of them adds
        const unsigned long long live = __ballot(1), mask = __ballot(took);
        if ((threadIdx.x & 63u) == static_cast<uint32_t>(__ffsll(live) - 1) && mask)
            atomicAdd(&p.tallies[8u * (blockIdx.x % kReprojectTallySlots)],
                      static_cast<unsigned long long>(__popcll(mask)));
    }
}
