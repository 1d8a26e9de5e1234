// denoise.hip -- the denoiser's passes (include/vcrt.h vcrt_denoise, the definition; csrc/denoise.cpp
// vcrt_denoise_host, the same on the host): one launch per a-trous pass, gfx950.
//
// One lane owns one output pixel and runs its 25 taps with dy outer and dx inner, both ascending,
// every fp32 operation rounded on its own (no contraction, correctly rounded division), so the
// plane's bits depend on the inputs and the scales only. Two kernels compute them:
//   vcrt_denoise_pass      a wave covers a 64-pixel segment of a row, so each tap of each plane is
//                          one coalesced 16-B load per lane, served by L1/L2 after the first
//                          touch. Any step.
//   vcrt_denoise_pass_lds  a workgroup covers 32 x 8 pixels and first stages the footprint with
//                          its halo of 2 step -- the pass's input and the guide planes whose terms
//                          are on -- in LDS: (32 + 4 step) x (8 + 4 step) entries a plane, 20 KB
//                          (step 1) or 30 KB (step 2) for three planes. Pass 0's demodulation is
//                          then one division per staged pixel, not one per tap. Step 1 and 2.
// Both skip a tap once its guide terms alone reach 1: X >= 1 whatever the colour term adds, so
// w = h * 0 = +0, and +0 * s_q added to the sums changes no bit for a finite s_q -- the direct
// kernel saves the tap's colour load, which at step >= 4 is a third of its traffic.
// Bounds: every global load is of a tap or a staged entry inside the frame (tested in x and y,
// pixel indices below 2^26), every LDS index is below the staged entry count.
#include <hip/hip_runtime.h>

#include "denoise_abi.h"

#pragma clang fp contract(off)

using namespace vcrt;

namespace {

constexpr float kEps = 0x1p-10f;       // the demodulation's floor on the albedo
constexpr float kDepthEps = 0x1p-20f;  // the relative depth's denominator never vanishes

__device__ __forceinline__ float4 ld4(const float* plane, size_t i) {
    return reinterpret_cast<const float4*>(plane)[i];
}

// s_0 = colour / max(albedo, eps) per rgb channel (alpha unused)
__device__ __forceinline__ float4 demodulated(float4 c, float4 a) {
    return make_float4(c.x / fmaxf(a.x, kEps), c.y / fmaxf(a.y, kEps), c.z / fmaxf(a.z, kEps),
                       0.0f);
}

// The direct kernel's planes: a tap is a pixel index of the frame.
struct GlobalPlanes {
    const DenoiseParams& p;
    __device__ __forceinline__ float4 nd(size_t q) const { return ld4(p.normal_depth, q); }
    __device__ __forceinline__ float4 alb(size_t q) const { return ld4(p.albedo, q); }
    __device__ __forceinline__ float4 s(size_t q) const {
        const float4 c = ld4(p.in, q);
        return (p.flags & kDenoiseDemodIn) ? demodulated(c, ld4(p.albedo, q)) : c;
    }
};

// The LDS kernel's planes: a tap is an entry of the staged footprint.
struct StagedPlanes {
    const float4* l_s;
    const float4* l_a;
    const float4* l_n;
    __device__ __forceinline__ float4 nd(size_t q) const { return l_n[q]; }
    __device__ __forceinline__ float4 alb(size_t q) const { return l_a[q]; }
    __device__ __forceinline__ float4 s(size_t q) const { return l_s[q]; }
};

struct Sums {
    float r, g, b, w;
};

// One tap: vcrt.h's h, dn, rz, da, dl, X, e, w and the four sums, in that order.
template <class Planes>
__device__ __forceinline__ void tap(const DenoiseParams& p, const Planes& pl, float h, float4 n_p,
                                    float4 a_p, float4 s_p, size_t q, Sums& acc) {
    float tn = 0.0f, tz = 0.0f, ta = 0.0f, tl = 0.0f;
    if (p.flags & (kDenoiseNormal | kDenoiseDepth)) {
        const float4 n_q = pl.nd(q);
        if (p.flags & kDenoiseNormal) {
            const float d0 = n_p.x - n_q.x, d1 = n_p.y - n_q.y, d2 = n_p.z - n_q.z;
            float dn = d0 * d0;
            dn = dn + d1 * d1;
            dn = dn + d2 * d2;
            tn = dn * p.k_normal;
        }
        if (p.flags & kDenoiseDepth) {
            const float num = n_p.w - n_q.w;
            float den = fabsf(n_p.w) + fabsf(n_q.w);
            den = den + kDepthEps;
            const float rz = num / den;
            tz = (rz * rz) * p.k_depth;
        }
    }
    if (p.flags & kDenoiseAlbedo) {
        const float4 a_q = pl.alb(q);
        const float d0 = a_p.x - a_q.x, d1 = a_p.y - a_q.y, d2 = a_p.z - a_q.z, d3 = a_p.w - a_q.w;
        float da = d0 * d0;
        da = da + d1 * d1;
        da = da + d2 * d2;
        da = da + d3 * d3;
        ta = da * p.k_albedo;
    }
    float X = tn + tz;
    X = X + ta;
    if (X >= 1.0f) return;  // w = +0 whatever the colour says: the sums keep their bits
    const float4 s_q = pl.s(q);
    if (p.flags & kDenoiseColour) {
        const float d0 = s_p.x - s_q.x, d1 = s_p.y - s_q.y, d2 = s_p.z - s_q.z;
        float dl = d0 * d0;
        dl = dl + d1 * d1;
        dl = dl + d2 * d2;
        tl = dl * p.kl;
    }
    X = X + tl;
    const float e = 1.0f - fminf(X, 1.0f);
    const float w = h * (e * e);
    acc.r = acc.r + w * s_q.x;
    acc.g = acc.g + w * s_q.y;
    acc.b = acc.b + w * s_q.z;
    acc.w = acc.w + w;
}

// The pixel's 25 taps. (x, y) is inside the frame; centre and the tap index
// centre + step (dy pitch + dx) are pixel indices (pitch = width) or staged entries.
template <class Planes>
__device__ __forceinline__ Sums filter_pixel(const DenoiseParams& p, const Planes& pl, int32_t x,
                                             int32_t y, size_t centre, size_t pitch) {
    constexpr float k5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const int32_t step = static_cast<int32_t>(p.step);
    const int32_t W = static_cast<int32_t>(p.width), H = static_cast<int32_t>(p.height);
    float4 n_p = make_float4(0.f, 0.f, 0.f, 0.f), a_p = n_p;
    if (p.flags & (kDenoiseNormal | kDenoiseDepth)) n_p = pl.nd(centre);
    if (p.flags & kDenoiseAlbedo) a_p = pl.alb(centre);
    const float4 s_p = pl.s(centre);
    Sums acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int32_t qy = y + step * dy;
        if (qy < 0 || qy >= H) continue;
        // the row's entry under the centre: never negative, the row is inside the frame
        const size_t row = dy < 0 ? centre - static_cast<size_t>(-dy * step) * pitch
                                  : centre + static_cast<size_t>(dy * step) * pitch;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int32_t qx = x + step * dx;
            if (qx < 0 || qx >= W) continue;
            const size_t q = dx < 0 ? row - static_cast<size_t>(-dx * step)
                                    : row + static_cast<size_t>(dx * step);
            tap(p, pl, k5[dx + 2] * k5[dy + 2], n_p, a_p, s_p, q, acc);
        }
    }
    return acc;
}

// s_{l+1} = sums / wsum; the last pass multiplies the albedo back and carries colour's alpha.
__device__ __forceinline__ void store_pixel(const DenoiseParams& p, size_t gp, const Sums& acc) {
    float4 o = make_float4(acc.r / acc.w, acc.g / acc.w, acc.b / acc.w, 0.0f);
    if (p.flags & kDenoiseModOut) {
        const float4 a = ld4(p.albedo, gp);
        o.x = o.x * fmaxf(a.x, kEps);
        o.y = o.y * fmaxf(a.y, kEps);
        o.z = o.z * fmaxf(a.z, kEps);
    }
    if (p.flags & kDenoiseLast) o.w = ld4(p.colour, gp).w;
    reinterpret_cast<float4*>(p.out)[gp] = o;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(vcrt::kDenoiseThreads)
vcrt_denoise_pass(DenoiseParams p) {
    const uint32_t bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const uint32_t x = bx * kDenoiseRowW + (threadIdx.x % kDenoiseRowW);
    const uint32_t y = by * kDenoiseRowH + (threadIdx.x / kDenoiseRowW);
    if (x >= p.width || y >= p.height) return;
    const size_t gp = static_cast<size_t>(y) * p.width + x;
    const GlobalPlanes pl{p};
    const Sums acc = filter_pixel(p, pl, static_cast<int32_t>(x), static_cast<int32_t>(y), gp,
                                  p.width);
    store_pixel(p, gp, acc);
}

extern "C" __global__ void __launch_bounds__(vcrt::kDenoiseThreads)
vcrt_denoise_pass_lds(DenoiseParams p) {
    extern __shared__ __align__(16) float4 l_planes[];
    const uint32_t halo = 2u * p.step;
    const uint32_t tw = kDenoiseTileW + 2u * halo, th = kDenoiseTileH + 2u * halo;
    const uint32_t entries = tw * th;
    const bool stage_n = (p.flags & (kDenoiseNormal | kDenoiseDepth)) != 0;
    const bool stage_a = (p.flags & kDenoiseAlbedo) != 0;
    // the planes in the order s, albedo, normal_depth; a plane that is not staged takes no room
    float4* l_s = l_planes;
    float4* l_a = l_s + entries;
    float4* l_n = l_a + (stage_a ? entries : 0u);
    const uint32_t bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const int32_t x0 = static_cast<int32_t>(bx * kDenoiseTileW) - static_cast<int32_t>(halo);
    const int32_t y0 = static_cast<int32_t>(by * kDenoiseTileH) - static_cast<int32_t>(halo);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t i = threadIdx.x; i < entries; i += kDenoiseThreads) {
        const int32_t gx = x0 + static_cast<int32_t>(i % tw);
        const int32_t gy = y0 + static_cast<int32_t>(i / tw);
        // entries outside the frame are never read as taps: zero, so that LDS holds no stale bits
        float4 s = zero, a = zero, n = zero;
        if (gx >= 0 && gy >= 0 && gx < static_cast<int32_t>(p.width) &&
            gy < static_cast<int32_t>(p.height)) {
            const size_t q = static_cast<size_t>(gy) * p.width + static_cast<size_t>(gx);
            s = ld4(p.in, q);
            if (stage_a || (p.flags & kDenoiseDemodIn)) a = ld4(p.albedo, q);
            if (p.flags & kDenoiseDemodIn) s = demodulated(s, a);
            if (stage_n) n = ld4(p.normal_depth, q);
        }
        l_s[i] = s;
        if (stage_a) l_a[i] = a;
        if (stage_n) l_n[i] = n;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % kDenoiseTileW, ly = threadIdx.x / kDenoiseTileW;
    const uint32_t x = bx * kDenoiseTileW + lx, y = by * kDenoiseTileH + ly;
    if (x >= p.width || y >= p.height) return;
    const StagedPlanes pl{l_s, l_a, l_n};
    const size_t centre = static_cast<size_t>(ly + halo) * tw + (lx + halo);
    const Sums acc = filter_pixel(p, pl, static_cast<int32_t>(x), static_cast<int32_t>(y), centre,
                                  tw);
    store_pixel(p, static_cast<size_t>(y) * p.width + x, acc);
}
