// denoise.cpp -- the denoiser's definition as code (include/vcrt.h vcrt_denoise): the parameter
// checks and scales every form of the call shares, and vcrt_denoise_host, the edge-avoiding
// a-trous filter on the host, one rounded fp32 operation per statement (built with
// -ffp-contract=off). The kernels of denoise.hip compute the same bits.
#include <cmath>
#include <cstdint>
#include <vector>

#include "denoise_abi.h"
#include "vcrt.h"

namespace {

constexpr float kEps = 0x1p-10f;       // the demodulation's floor on the albedo
constexpr float kDepthEps = 0x1p-20f;  // the relative depth's denominator never vanishes
constexpr float kK5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
constexpr int32_t kMaxLevels = 8;
constexpr uint64_t kMaxPixels = uint64_t{1} << 26;

// k = 1 / sigma^2, 0 for sigma == 0; false for a sigma the call refuses
bool scale_of(float sigma, float* k) {
    if (!(sigma >= 0.0f) || std::isinf(sigma)) return false;  // NaN, negative, infinite
    if (sigma == 0.0f) {
        *k = 0.0f;
        return true;
    }
    const float s2 = sigma * sigma;
    *k = 1.0f / s2;
    return std::isfinite(*k);
}

struct Rgb {
    float r, g, b;
};

}  // namespace

vcrt_result vcrt_default_denoise_params(vcrt_denoise_params* params) {
    if (!params) return VCRT_ERROR_INITIALIZATION_FAILED;
    *params = vcrt_denoise_params{};
    params->struct_size = sizeof(vcrt_denoise_params);
    params->levels = 5;
    // tools/denoise_defaults.py's choice (profiles/denoise_defaults.json)
    params->sigma_normal = 0.25f;
    params->sigma_depth = 0.05f;
    params->sigma_albedo = 0.125f;
    params->sigma_colour = 0.75f;
    params->demodulate = 1;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_denoise_scales(const vcrt_denoise_params* params, float k4[4]) {
    if (!params || !k4) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (params->struct_size != sizeof(vcrt_denoise_params)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (params->levels < 1 || params->levels > kMaxLevels) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!scale_of(params->sigma_normal, &k4[0]) || !scale_of(params->sigma_depth, &k4[1]) ||
        !scale_of(params->sigma_albedo, &k4[2]) || !scale_of(params->sigma_colour, &k4[3]))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    // kl of the last pass: a power of four times k_colour, exact unless it overflows
    float kl = k4[3];
    for (int32_t l = 1; l < params->levels; l++) kl = kl * 4.0f;
    if (!std::isfinite(kl)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    return VCRT_SUCCESS;
}

int32_t vcrt::denoise_args(const float* colour, const float* albedo, const float* normal_depth,
                           int32_t width, int32_t height, const vcrt_denoise_params* params,
                           const float* out, vcrt_denoise_params* eff, float k4[4]) {
    if (params) *eff = *params;
    else vcrt_default_denoise_params(eff);
    const vcrt_result s = vcrt_denoise_scales(eff, k4);
    if (s != VCRT_SUCCESS) return s;
    if (width < 1 || width > 65535 || height < 1 || height > 65535 ||
        static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > kMaxPixels)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!colour || !out) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (out == colour || out == albedo || out == normal_depth)
        return VCRT_ERROR_INITIALIZATION_FAILED;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_denoise_host(const float* colour, const float* albedo, const float* normal_depth,
                              int32_t width, int32_t height, const vcrt_denoise_params* params,
                              float* out) {
    vcrt_denoise_params pr;
    float k4[4];
    const int32_t a = vcrt::denoise_args(colour, albedo, normal_depth, width, height, params, out,
                                         &pr, k4);
    if (a != VCRT_SUCCESS) return a;
    const size_t W = static_cast<size_t>(width), H = static_cast<size_t>(height);
    const float* nd = normal_depth;
    const bool on_n = nd && k4[0] != 0.0f, on_z = nd && k4[1] != 0.0f;
    const bool on_a = albedo && k4[2] != 0.0f;
    const bool demod = pr.demodulate != 0 && albedo;

    // pass 0's input
    std::vector<Rgb> s(W * H), t(W * H);
    for (size_t p = 0; p < W * H; p++) {
        if (demod)
            s[p] = {colour[4 * p] / std::fmax(albedo[4 * p], kEps),
                    colour[4 * p + 1] / std::fmax(albedo[4 * p + 1], kEps),
                    colour[4 * p + 2] / std::fmax(albedo[4 * p + 2], kEps)};
        else
            s[p] = {colour[4 * p], colour[4 * p + 1], colour[4 * p + 2]};
    }

    float kl = k4[3];
    for (int32_t l = 0; l < pr.levels; l++) {
        const bool on_c = kl != 0.0f;
        const int64_t step = int64_t{1} << l;
        for (int64_t y = 0; y < height; y++) {
            for (int64_t x = 0; x < width; x++) {
                const size_t p = static_cast<size_t>(y) * W + static_cast<size_t>(x);
                float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
                for (int dy = -2; dy <= 2; dy++) {
                    const int64_t qy = y + step * dy;
                    if (qy < 0 || qy >= height) continue;
                    for (int dx = -2; dx <= 2; dx++) {
                        const int64_t qx = x + step * dx;
                        if (qx < 0 || qx >= width) continue;
                        const size_t q = static_cast<size_t>(qy) * W + static_cast<size_t>(qx);
                        const float h = kK5[dx + 2] * kK5[dy + 2];
                        float tn = 0.0f, tz = 0.0f, ta = 0.0f, tl = 0.0f;
                        if (on_n) {
                            const float d0 = nd[4 * p] - nd[4 * q];
                            const float d1 = nd[4 * p + 1] - nd[4 * q + 1];
                            const float d2 = nd[4 * p + 2] - nd[4 * q + 2];
                            float dn = d0 * d0;
                            dn = dn + d1 * d1;
                            dn = dn + d2 * d2;
                            tn = dn * k4[0];
                        }
                        if (on_z) {
                            const float zp = nd[4 * p + 3], zq = nd[4 * q + 3];
                            const float num = zp - zq;
                            float den = std::fabs(zp) + std::fabs(zq);
                            den = den + kDepthEps;
                            const float rz = num / den;
                            tz = (rz * rz) * k4[1];
                        }
                        if (on_a) {
                            const float d0 = albedo[4 * p] - albedo[4 * q];
                            const float d1 = albedo[4 * p + 1] - albedo[4 * q + 1];
                            const float d2 = albedo[4 * p + 2] - albedo[4 * q + 2];
                            const float d3 = albedo[4 * p + 3] - albedo[4 * q + 3];
                            float da = d0 * d0;
                            da = da + d1 * d1;
                            da = da + d2 * d2;
                            da = da + d3 * d3;
                            ta = da * k4[2];
                        }
                        if (on_c) {
                            const float d0 = s[p].r - s[q].r;
                            const float d1 = s[p].g - s[q].g;
                            const float d2 = s[p].b - s[q].b;
                            float dl = d0 * d0;
                            dl = dl + d1 * d1;
                            dl = dl + d2 * d2;
                            tl = dl * kl;
                        }
                        float X = tn + tz;
                        X = X + ta;
                        X = X + tl;
                        const float e = 1.0f - std::fmin(X, 1.0f);
                        const float w = h * (e * e);
                        ar = ar + w * s[q].r;
                        ag = ag + w * s[q].g;
                        ab = ab + w * s[q].b;
                        wsum = wsum + w;
                    }
                }
                t[p] = {ar / wsum, ag / wsum, ab / wsum};
            }
        }
        s.swap(t);
        kl = kl * 4.0f;
    }

    for (size_t p = 0; p < W * H; p++) {
        if (demod) {
            out[4 * p] = s[p].r * std::fmax(albedo[4 * p], kEps);
            out[4 * p + 1] = s[p].g * std::fmax(albedo[4 * p + 1], kEps);
            out[4 * p + 2] = s[p].b * std::fmax(albedo[4 * p + 2], kEps);
        } else {
            out[4 * p] = s[p].r;
            out[4 * p + 1] = s[p].g;
            out[4 * p + 2] = s[p].b;
        }
        out[4 * p + 3] = colour[4 * p + 3];
    }
    return VCRT_SUCCESS;
}
