// variance.hip -- variance-guided denoising's kernels (include/vcrt.h vcrt_reproject_moments,
// vcrt_variance, vcrt_denoise_variance, the definitions; csrc/variance.cpp the same on the host),
// gfx950.
//
// One lane owns one output pixel everywhere, every fp32 operation is rounded on its own (no
// contraction, correctly rounded division) and every sum runs in the order vcrt.h states, so the
// planes' bits depend on the inputs and the parameters only.
//   vcrt_reproject_moments_pass  vcrt_reproject_pass with the two luminance moments carried along:
//                                an accepted tap also loads its history moments (16 B).
//   vcrt_variance_pass           a pixel with the history reads its own moments; a younger one
//                                its 49 neighbours' surface keys and, where the key agrees, their
//                                moments, directly (L1/L2 serve the overlap).
//   vcrt_variance_pass_lds       the same from a staged 38 x 14 footprint: the measured choice
//                                (tools/variance_bench.py, profiles/variance.json); the direct
//                                kernel stays as VCRT_VARIANCE_LDS=0.
//   vcrt_denoise_var_pass{,_lds} the a-trous pass of denoise.hip with the variance riding in the
//                                signal's fourth channel: the colour term is steered by the 3 x 3
//                                binomial of that channel, and the channel is filtered with the
//                                squared weights. The direct kernel reads its taps from global
//                                memory at any step; the LDS kernel stages the footprint with its
//                                halo of 2 step (step 1 and 2), which holds the 3 x 3 taps too.
// Bounds: every global load is of the pixel itself or of a tap tested in x and y before it is read
// (reprojection: the position is tested against (-1, W) x (-1, H) first, a NaN fails, so floorf is
// exact in int32); every LDS index is below the staged entry count. Pixel indices stay below 2^26.
#include <hip/hip_runtime.h>

#include "denoise_abi.h"
#include "variance_abi.h"

#pragma clang fp contract(off)

using namespace vcrt;

namespace {

constexpr float kEps = 0x1p-10f;       // the demodulation's floor on the albedo
constexpr float kDepthEps = 0x1p-20f;  // the relative depth's denominator never vanishes
constexpr float kVarEps = 0x1p-20f;    // kv's denominator never vanishes

__device__ __forceinline__ float4 ld4(const float* plane, size_t i) {
    return reinterpret_cast<const float4*>(plane)[i];
}

__device__ __forceinline__ float lum(float r, float g, float b) {
    float y = 0.2126f * r + 0.7152f * g;
    y = y + 0.0722f * b;
    return y;
}

// ---- vcrt_reproject_moments ---------------------------------------------------------------------

struct History {
    float r, g, b, l, w, m1, m2;
};

// One tap: vcrt.h's b, the three tests and the seven sums, in that order. (qx, qy) may lie outside
// the frame: then nothing is read.
__device__ __forceinline__ void history_tap(const ReprojectMomentsParams& p, float4 m, float b,
                                            int32_t qx, int32_t qy, History& acc) {
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
    const float4 m_q = ld4(p.history_moments, q);
    acc.r = acc.r + b * c_q.x;
    acc.g = acc.g + b * c_q.y;
    acc.b = acc.b + b * c_q.z;
    acc.l = acc.l + b * l_q;
    acc.w = acc.w + b;
    acc.m1 = acc.m1 + b * m_q.x;
    acc.m2 = acc.m2 + b * m_q.y;
}

// ---- vcrt_denoise_variance ----------------------------------------------------------------------

// The direct kernel's planes: a tap is a pixel index of the frame.
struct GlobalPlanes {
    const DenoiseVarParams& p;
    __device__ __forceinline__ float4 nd(size_t q) const { return ld4(p.normal_depth, q); }
    __device__ __forceinline__ float4 alb(size_t q) const { return ld4(p.albedo, q); }
    __device__ __forceinline__ float var(size_t q) const {
        return (p.flags & kDenoiseVarIn) ? fmaxf(p.variance[q], 0.0f) : p.in[4 * q + 3];
    }
    __device__ __forceinline__ float4 s(size_t q) const {
        float4 c = ld4(p.in, q);
        if (p.flags & kDenoiseDemodIn) {
            const float4 a = ld4(p.albedo, q);
            c.x = c.x / fmaxf(a.x, kEps);
            c.y = c.y / fmaxf(a.y, kEps);
            c.z = c.z / fmaxf(a.z, kEps);
        }
        if (p.flags & kDenoiseVarIn) c.w = fmaxf(p.variance[q], 0.0f);
        return c;
    }
};

// The LDS kernel's planes: a tap is an entry of the staged footprint.
struct StagedPlanes {
    const float4* l_s;
    const float4* l_a;
    const float4* l_n;
    __device__ __forceinline__ float4 nd(size_t q) const { return l_n[q]; }
    __device__ __forceinline__ float4 alb(size_t q) const { return l_a[q]; }
    __device__ __forceinline__ float var(size_t q) const { return l_s[q].w; }
    __device__ __forceinline__ float4 s(size_t q) const { return l_s[q]; }
};

struct Sums {
    float r, g, b, w, v;
};

// One tap: vcrt.h's h, dn, rz, da, dy, X, e, w and the five sums, in that order.
template <class Planes>
__device__ __forceinline__ void filter_tap(const DenoiseVarParams& p, const Planes& pl, float h,
                                           float4 n_p, float4 a_p, float y_p, float kv, size_t q,
                                           Sums& acc) {
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
        const float dy = y_p - lum(s_q.x, s_q.y, s_q.z);
        tl = (dy * dy) * kv;
    }
    X = X + tl;
    const float e = 1.0f - fminf(X, 1.0f);
    const float w = h * (e * e);
    acc.r = acc.r + w * s_q.x;
    acc.g = acc.g + w * s_q.y;
    acc.b = acc.b + w * s_q.z;
    acc.w = acc.w + w;
    acc.v = acc.v + (w * w) * s_q.w;
}

// The pixel's 9 variance taps and 25 filter taps. (x, y) is inside the frame; centre and the tap
// index centre + (dy pitch + dx) are pixel indices (pitch = width) or staged entries.
template <class Planes>
__device__ __forceinline__ Sums filter_pixel(const DenoiseVarParams& p, const Planes& pl,
                                             int32_t x, int32_t y, size_t centre, size_t pitch) {
    constexpr float k5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    constexpr float k3[3] = {0.25f, 0.5f, 0.25f};
    const int32_t step = static_cast<int32_t>(p.step);
    const int32_t W = static_cast<int32_t>(p.width), H = static_cast<int32_t>(p.height);
    float4 n_p = make_float4(0.f, 0.f, 0.f, 0.f), a_p = n_p;
    if (p.flags & (kDenoiseNormal | kDenoiseDepth)) n_p = pl.nd(centre);
    if (p.flags & kDenoiseAlbedo) a_p = pl.alb(centre);
    float kv = 0.0f, y_p = 0.0f;
    if (p.flags & kDenoiseColour) {
        float gsum = 0.0f, gw = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int32_t qy = y + dy;
            if (qy < 0 || qy >= H) continue;
            const size_t row = dy < 0 ? centre - pitch : centre + static_cast<size_t>(dy) * pitch;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int32_t qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const size_t q = dx < 0 ? row - 1 : row + static_cast<size_t>(dx);
                const float h3 = k3[dx + 1] * k3[dy + 1];
                gsum = gsum + h3 * pl.var(q);
                gw = gw + h3;
            }
        }
        const float g = gsum / gw;
        float den = p.sc2 * g;
        den = den + kVarEps;
        kv = 1.0f / den;
        const float4 s_p = pl.s(centre);
        y_p = lum(s_p.x, s_p.y, s_p.z);
    }
    Sums acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
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
            filter_tap(p, pl, k5[dx + 2] * k5[dy + 2], n_p, a_p, y_p, kv, q, acc);
        }
    }
    return acc;
}

// s_{l+1} = sums / wsum, its variance vacc / wsum^2; the last pass multiplies the albedo back,
// carries colour's alpha and hands the variance to its own plane.
__device__ __forceinline__ void store_pixel(const DenoiseVarParams& p, size_t gp,
                                            const Sums& acc) {
    float4 o = make_float4(acc.r / acc.w, acc.g / acc.w, acc.b / acc.w, acc.v / (acc.w * acc.w));
    if (p.flags & kDenoiseModOut) {
        const float4 a = ld4(p.albedo, gp);
        o.x = o.x * fmaxf(a.x, kEps);
        o.y = o.y * fmaxf(a.y, kEps);
        o.z = o.z * fmaxf(a.z, kEps);
    }
    if (p.flags & kDenoiseLast) {
        if (p.out_variance) p.out_variance[gp] = o.w;
        o.w = ld4(p.colour, gp).w;
    }
    reinterpret_cast<float4*>(p.out)[gp] = o;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(vcrt::kMomentsThreads)
vcrt_reproject_moments_pass(ReprojectMomentsParams p) {
    const uint32_t bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const uint32_t x = bx * kMomentsRowW + (threadIdx.x % kMomentsRowW);
    const uint32_t y = by * kMomentsRowH + (threadIdx.x / kMomentsRowW);
    if (x >= p.width || y >= p.height) return;
    const size_t gp = static_cast<size_t>(y) * p.width + x;
    const float4 m = ld4(p.motion, gp);
    const float4 c = ld4(p.colour, gp);
    float sr = c.x, sg = c.y, sb = c.z;
    if (p.albedo) {
        const float4 a = ld4(p.albedo, gp);
        sr = c.x / fmaxf(a.x, kEps);
        sg = c.y / fmaxf(a.y, kEps);
        sb = c.z / fmaxf(a.z, kEps);
    }
    const float Y = lum(sr, sg, sb);
    const float Y2 = Y * Y;
    const float W = static_cast<float>(p.width), H = static_cast<float>(p.height);
    History acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (m.w >= 1.0f && m.x > -1.0f && m.x < W && m.y > -1.0f && m.y < H) {
        const float fx = floorf(m.x), fy = floorf(m.y);
        const float ax = m.x - fx, ay = m.y - fy;
        const float bx0 = 1.0f - ax, by0 = 1.0f - ay;
        const int32_t ix = static_cast<int32_t>(fx), iy = static_cast<int32_t>(fy);
        history_tap(p, m, bx0 * by0, ix, iy, acc);
        history_tap(p, m, ax * by0, ix + 1, iy, acc);
        history_tap(p, m, bx0 * ay, ix, iy + 1, acc);
        history_tap(p, m, ax * ay, ix + 1, iy + 1, acc);
    }
    const bool took = acc.w > 0.0f;
    float4 o = c;
    float n = 1.0f, M1 = Y, M2 = Y2;
    if (took) {
        const float hr = acc.r / acc.w, hg = acc.g / acc.w, hb = acc.b / acc.w;
        const float l = acc.l / acc.w;
        n = fminf(l + 1.0f, p.max_history);
        const float rn = 1.0f / n;
        const float a = fmaxf(p.alpha, rn);
        o.x = hr + a * (c.x - hr);
        o.y = hg + a * (c.y - hg);
        o.z = hb + a * (c.z - hb);
        const float h1 = acc.m1 / acc.w, h2 = acc.m2 / acc.w;
        const float am = fmaxf(p.alpha_moments, rn);
        M1 = h1 + am * (Y - h1);
        M2 = h2 + am * (Y2 - h2);
    }
    reinterpret_cast<float4*>(p.out)[gp] = o;
    p.out_length[gp] = n;
    reinterpret_cast<float4*>(p.out_moments)[gp] =
        make_float4(M1, M2, fmaxf(M2 - M1 * M1, 0.0f), n);
    if (p.tallies) {
        // per wave: the lanes inside the frame are here together, the first of them adds
        const unsigned long long live = __ballot(1), mask = __ballot(took);
        if ((threadIdx.x & 63u) == static_cast<uint32_t>(__ffsll(live) - 1) && mask)
            atomicAdd(&p.tallies[8u * (blockIdx.x % kMomentsTallySlots)],
                      static_cast<unsigned long long>(__popcll(mask)));
    }
}

extern "C" __global__ void __launch_bounds__(vcrt::kVarianceThreads)
vcrt_variance_pass(VarianceParams p) {
    const uint32_t bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const uint32_t x = bx * kVarianceRowW + (threadIdx.x % kVarianceRowW);
    const uint32_t y = by * kVarianceRowH + (threadIdx.x / kVarianceRowW);
    if (x >= p.width || y >= p.height) return;
    const size_t gp = static_cast<size_t>(y) * p.width + x;
    const float4 m_p = ld4(p.moments, gp);
    const float N = fmaxf(m_p.w, 1.0f);
    const bool spatial = !(m_p.w >= p.min_history);
    float v = m_p.z;
    if (spatial) {
        const int32_t W = static_cast<int32_t>(p.width), H = static_cast<int32_t>(p.height);
        const int32_t xi = static_cast<int32_t>(x), yi = static_cast<int32_t>(y);
        const float key = p.surface[4 * gp];
        float S1 = 0.0f, S2 = 0.0f, n = 0.0f;
        for (int32_t dy = -kVarianceRadius; dy <= kVarianceRadius; dy++) {
            const int32_t qy = yi + dy;
            if (qy < 0 || qy >= H) continue;
            const size_t row = static_cast<size_t>(qy) * p.width;
            for (int32_t dx = -kVarianceRadius; dx <= kVarianceRadius; dx++) {
                const int32_t qx = xi + dx;
                if (qx < 0 || qx >= W) continue;
                const size_t q = row + static_cast<size_t>(qx);
                // the centre always counts (a NaN key equals nothing, itself included)
                if (q != gp && !(p.surface[4 * q] == key)) continue;
                const float4 m_q = ld4(p.moments, q);
                S1 = S1 + m_q.x;
                S2 = S2 + m_q.y;
                n = n + 1.0f;
            }
        }
        const float a1 = S1 / n, a2 = S2 / n;
        const float sv = fmaxf(a2 - a1 * a1, 0.0f);
        const float boost = p.min_history / N;
        v = sv * boost;
    }
    const float rn = 1.0f / N;
    p.variance[gp] = v * fmaxf(p.alpha, rn);
    if (p.tallies) {
        const unsigned long long live = __ballot(1), mask = __ballot(spatial);
        if ((threadIdx.x & 63u) == static_cast<uint32_t>(__ffsll(live) - 1) && mask)
            atomicAdd(&p.tallies[8u * (blockIdx.x % kVarianceTallySlots)],
                      static_cast<unsigned long long>(__popcll(mask)));
    }
}

// The same with the workgroup's 32 x 8 pixels and their halo of 3 staged in LDS first: per entry
// (M1, M2, key, -), 38 x 14 entries, 8.3 KB. The default; same bits.
extern "C" __global__ void __launch_bounds__(vcrt::kVarianceThreads)
vcrt_variance_pass_lds(VarianceParams p) {
    extern __shared__ __align__(16) float4 l_var_planes[];
    constexpr uint32_t halo = static_cast<uint32_t>(kVarianceRadius);
    constexpr uint32_t tw = kVarianceTileW + 2u * halo, th = kVarianceTileH + 2u * halo;
    const uint32_t bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const int32_t x0 = static_cast<int32_t>(bx * kVarianceTileW) - static_cast<int32_t>(halo);
    const int32_t y0 = static_cast<int32_t>(by * kVarianceTileH) - static_cast<int32_t>(halo);
    const int32_t W = static_cast<int32_t>(p.width), H = static_cast<int32_t>(p.height);
    for (uint32_t i = threadIdx.x; i < tw * th; i += kVarianceThreads) {
        const int32_t gx = x0 + static_cast<int32_t>(i % tw);
        const int32_t gy = y0 + static_cast<int32_t>(i / tw);
        // entries outside the frame are never read as taps: zero, so that LDS holds no stale bits
        float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
            const size_t q = static_cast<size_t>(gy) * p.width + static_cast<size_t>(gx);
            const float4 m_q = ld4(p.moments, q);
            e = make_float4(m_q.x, m_q.y, p.surface[4 * q], 0.f);
        }
        l_var_planes[i] = e;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % kVarianceTileW, ly = threadIdx.x / kVarianceTileW;
    const uint32_t x = bx * kVarianceTileW + lx, y = by * kVarianceTileH + ly;
    if (x >= p.width || y >= p.height) return;
    const size_t gp = static_cast<size_t>(y) * p.width + x;
    const float4 m_p = ld4(p.moments, gp);
    const float N = fmaxf(m_p.w, 1.0f);
    const bool spatial = !(m_p.w >= p.min_history);
    float v = m_p.z;
    if (spatial) {
        const int32_t xi = static_cast<int32_t>(x), yi = static_cast<int32_t>(y);
        const uint32_t centre = (ly + halo) * tw + (lx + halo);
        const float key = l_var_planes[centre].z;
        float S1 = 0.0f, S2 = 0.0f, n = 0.0f;
        for (int32_t dy = -kVarianceRadius; dy <= kVarianceRadius; dy++) {
            const int32_t qy = yi + dy;
            if (qy < 0 || qy >= H) continue;
            for (int32_t dx = -kVarianceRadius; dx <= kVarianceRadius; dx++) {
                const int32_t qx = xi + dx;
                if (qx < 0 || qx >= W) continue;
                // inside the frame, so inside the staged footprint: the index is not negative
                const uint32_t q = static_cast<uint32_t>(
                    static_cast<int32_t>(centre) + dy * static_cast<int32_t>(tw) + dx);
                const float4 e = l_var_planes[q];
                if (q != centre && !(e.z == key)) continue;
                S1 = S1 + e.x;
                S2 = S2 + e.y;
                n = n + 1.0f;
            }
        }
        const float a1 = S1 / n, a2 = S2 / n;
        const float sv = fmaxf(a2 - a1 * a1, 0.0f);
        const float boost = p.min_history / N;
        v = sv * boost;
    }
    const float rn = 1.0f / N;
    p.variance[gp] = v * fmaxf(p.alpha, rn);
    if (p.tallies) {
        const unsigned long long live = __ballot(1), mask = __ballot(spatial);
        if ((threadIdx.x & 63u) == static_cast<uint32_t>(__ffsll(live) - 1) && mask)
            atomicAdd(&p.tallies[8u * (blockIdx.x % kVarianceTallySlots)],
                      static_cast<unsigned long long>(__popcll(mask)));
    }
}

extern "C" __global__ void __launch_bounds__(vcrt::kDenoiseThreads)
vcrt_denoise_var_pass(DenoiseVarParams p) {
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
vcrt_denoise_var_pass_lds(DenoiseVarParams p) {
    extern __shared__ __align__(16) float4 l_var_planes[];
    const uint32_t halo = 2u * p.step;
    const uint32_t tw = kDenoiseTileW + 2u * halo, th = kDenoiseTileH + 2u * halo;
    const uint32_t entries = tw * th;
    const bool stage_n = (p.flags & (kDenoiseNormal | kDenoiseDepth)) != 0;
    const bool stage_a = (p.flags & kDenoiseAlbedo) != 0;
    // the planes in the order s, albedo, normal_depth; a plane that is not staged takes no room
    float4* l_s = l_var_planes;
    float4* l_a = l_s + entries;
    float4* l_n = l_a + (stage_a ? entries : 0u);
    const uint32_t bx = blockIdx.x % p.tiles_x, by = blockIdx.x / p.tiles_x;
    const int32_t x0 = static_cast<int32_t>(bx * kDenoiseTileW) - static_cast<int32_t>(halo);
    const int32_t y0 = static_cast<int32_t>(by * kDenoiseTileH) - static_cast<int32_t>(halo);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const GlobalPlanes gl{p};
    for (uint32_t i = threadIdx.x; i < entries; i += kDenoiseThreads) {
        const int32_t gx = x0 + static_cast<int32_t>(i % tw);
        const int32_t gy = y0 + static_cast<int32_t>(i / tw);
        // entries outside the frame are never read as taps: zero, so that LDS holds no stale bits
        float4 s = zero, a = zero, n = zero;
        if (gx >= 0 && gy >= 0 && gx < static_cast<int32_t>(p.width) &&
            gy < static_cast<int32_t>(p.height)) {
            const size_t q = static_cast<size_t>(gy) * p.width + static_cast<size_t>(gx);
            s = gl.s(q);
            if (stage_a) a = ld4(p.albedo, q);
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
