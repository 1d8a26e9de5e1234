// reproject.cpp -- temporal accumulation's definition as code (include/vcrt.h vcrt_reproject):
// the parameter checks every form of the call shares, and vcrt_reproject_host, the reprojected
// blend on the host, one rounded fp32 operation per statement (built with -ffp-contract=off). The
// kernel of reproject.hip computes the same bits.
#include <cmath>
#include <cstdint>

#include "reproject_abi.h"
#include "vcrt.h"

namespace {

constexpr float kDepthEps = 0x1p-20f;  // the relative depth's denominator never vanishes
constexpr uint64_t kMaxPixels = uint64_t{1} << 26;

}  // namespace

vcrt_result vcrt_default_reproject_params(vcrt_reproject_params* params) {
    if (!params) return VCRT_ERROR_INITIALIZATION_FAILED;
    *params = vcrt_reproject_params{};
    params->struct_size = sizeof(vcrt_reproject_params);
    // tools/reproject_defaults.py's choice (profiles/reproject_defaults.json)
    params->alpha = 0.6f;
    params->max_history = 32.0f;
    params->depth_tolerance = 0.1f;
    return VCRT_SUCCESS;
}

int32_t vcrt::reproject_args(const float* colour, const float* motion, const float* history_colour,
                             const float* history_surface, const float* history_length,
                             int32_t width, int32_t height, const vcrt_reproject_params* params,
                             const float* out, const float* out_length,
                             vcrt_reproject_params* eff) {
    if (params) *eff = *params;
    else vcrt_default_reproject_params(eff);
    if (eff->struct_size != sizeof(vcrt_reproject_params)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    // written so that a NaN fails
    if (!(eff->alpha > 0.0f && eff->alpha <= 1.0f)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!(eff->max_history >= 1.0f && eff->max_history <= 65535.0f))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!(eff->depth_tolerance >= 0.0f)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (width < 1 || width > 65535 || height < 1 || height > 65535 ||
        static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > kMaxPixels)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    const float* in[5] = {colour, motion, history_colour, history_surface, history_length};
    if (!out || !out_length || out == out_length) return VCRT_ERROR_INITIALIZATION_FAILED;
    for (const float* p : in)
        if (!p || p == out || p == out_length) return VCRT_ERROR_INITIALIZATION_FAILED;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_reproject_host(const float* colour, const float* motion,
                                const float* history_colour, const float* history_surface,
                                const float* history_length, int32_t width, int32_t height,
                                const vcrt_reproject_params* params, float* out,
                                float* out_length) {
    vcrt_reproject_params pr;
    const int32_t a = vcrt::reproject_args(colour, motion, history_colour, history_surface,
                                           history_length, width, height, params, out, out_length,
                                           &pr);
    if (a != VCRT_SUCCESS) return a;
    const size_t Wn = static_cast<size_t>(width), Hn = static_cast<size_t>(height);
    const float W = static_cast<float>(width), H = static_cast<float>(height);
    for (size_t p = 0; p < Wn * Hn; p++) {
        const float* m = motion + 4 * p;
        const float* c = colour + 4 * p;
        float ar = 0.0f, ag = 0.0f, ab = 0.0f, lsum = 0.0f, wsum = 0.0f;
        if (m[3] >= 1.0f && m[0] > -1.0f && m[0] < W && m[1] > -1.0f && m[1] < H) {
            const float fx = std::floor(m[0]), fy = std::floor(m[1]);
            const float ax = m[0] - fx, ay = m[1] - fy;
            const int64_t ix = static_cast<int64_t>(fx), iy = static_cast<int64_t>(fy);
            for (int t = 0; t < 4; t++) {
                const int dx = t & 1, dy = t >> 1;
                const float bx = dx ? ax : 1.0f - ax;
                const float by = dy ? ay : 1.0f - ay;
                const float b = bx * by;
                const int64_t qx = ix + dx, qy = iy + dy;
                if (b == 0.0f || qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                const size_t q = static_cast<size_t>(qy) * Wn + static_cast<size_t>(qx);
                const float* s = history_surface + 4 * q;
                const float lq = history_length[q];
                if (!(s[0] == m[3])) continue;
                if (!(lq >= 1.0f)) continue;
                if (m[3] != 1.0f && pr.depth_tolerance != 0.0f) {
                    const float num = std::fabs(m[2] - s[1]);
                    float den = std::fabs(m[2]) + std::fabs(s[1]);
                    den = den + kDepthEps;
                    const float rz = num / den;
                    if (!(rz <= pr.depth_tolerance)) continue;
                }
                const float* hq = history_colour + 4 * q;
                ar = ar + b * hq[0];
                ag = ag + b * hq[1];
                ab = ab + b * hq[2];
                lsum = lsum + b * lq;
                wsum = wsum + b;
            }
        }
        if (wsum > 0.0f) {
            const float hr = ar / wsum, hg = ag / wsum, hb = ab / wsum;
            const float L = lsum / wsum;
            const float N = std::fmin(L + 1.0f, pr.max_history);
            const float al = std::fmax(pr.alpha, 1.0f / N);
            out[4 * p] = hr + al * (c[0] - hr);
            out[4 * p + 1] = hg + al * (c[1] - hg);
            out[4 * p + 2] = hb + al * (c[2] - hb);
            out[4 * p + 3] = c[3];
            out_length[p] = N;
        } else {
            out[4 * p] = c[0];
            out[4 * p + 1] = c[1];
            out[4 * p + 2] = c[2];
            out[4 * p + 3] = c[3];
            out_length[p] = 1.0f;
        }
    }
    return VCRT_SUCCESS;
}
