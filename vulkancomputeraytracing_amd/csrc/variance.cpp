// variance.cpp -- variance-guided denoising's definitions as code (include/vcrt.h
// vcrt_reproject_moments, vcrt_variance, vcrt_denoise_variance): the parameter checks every form
// of the three calls shares, and the three _host functions, one rounded fp32 operation per
// statement (built with -ffp-contract=off). The kernels of variance.hip compute the same bits.
#include <cmath>
#include <cstdint>
#include <vector>

#include "denoise_abi.h"
#include "reproject_abi.h"
#include "variance_abi.h"
#include "vcrt.h"

namespace {

constexpr float kEps = 0x1p-10f;       // the demodulation's floor on the albedo
constexpr float kDepthEps = 0x1p-20f;  // the relative depth's denominator never vanishes
constexpr float kVarEps = 0x1p-20f;    // kv's denominator never vanishes
constexpr float kK5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
constexpr float kK3[3] = {0.25f, 0.5f, 0.25f};
constexpr uint64_t kMaxPixels = uint64_t{1} << 26;

inline float lum(float r, float g, float b) {
    float y = 0.2126f * r + 0.7152f * g;
    y = y + 0.0722f * b;
    return y;
}

struct Sig {
    float r, g, b, v;
};

}  // namespace

vcrt_result vcrt_default_reproject_moments_params(vcrt_reproject_moments_params* params) {
    if (!params) return VCRT_ERROR_INITIALIZATION_FAILED;
    *params = vcrt_reproject_moments_params{};
    params->struct_size = sizeof(vcrt_reproject_moments_params);
    // tools/variance_defaults.py's choice (profiles/variance_defaults.json)
    params->alpha = 0.6f;
    params->max_history = 32.0f;
    params->depth_tolerance = 0.1f;
    params->alpha_moments = 0.5f;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_default_variance_params(vcrt_variance_params* params) {
    if (!params) return VCRT_ERROR_INITIALIZATION_FAILED;
    *params = vcrt_variance_params{};
    params->struct_size = sizeof(vcrt_variance_params);
    // tools/variance_defaults.py's choice (profiles/variance_defaults.json)
    params->min_history = 8.0f;
    params->alpha = 0.6f;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_default_denoise_variance_params(vcrt_denoise_params* params) {
    const vcrt_result r = vcrt_default_denoise_params(params);
    if (r != VCRT_SUCCESS) return r;
    // tools/variance_defaults.py's choice (profiles/variance_defaults.json)
    params->sigma_colour = 1.0f;
    return VCRT_SUCCESS;
}

int32_t vcrt::reproject_moments_args(const float* colour, const float* motion,
                                     const float* history_colour, const float* history_surface,
                                     const float* history_length, const float* albedo,
                                     const float* history_moments, int32_t width, int32_t height,
                                     const vcrt_reproject_moments_params* params, const float* out,
                                     const float* out_length, const float* out_moments,
                                     vcrt_reproject_moments_params* eff) {
    if (params) *eff = *params;
    else vcrt_default_reproject_moments_params(eff);
    if (eff->struct_size != sizeof(vcrt_reproject_moments_params))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    // written so that a NaN fails
    if (!(eff->alpha_moments > 0.0f && eff->alpha_moments <= 1.0f))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    // the other parameters, the shape and the shared planes: vcrt_reproject's checks
    vcrt_reproject_params rp;
    rp.struct_size = sizeof(vcrt_reproject_params);
    rp.alpha = eff->alpha;
    rp.max_history = eff->max_history;
    rp.depth_tolerance = eff->depth_tolerance;
    vcrt_reproject_params rp_eff;
    const int32_t a = vcrt::reproject_args(colour, motion, history_colour, history_surface,
                                           history_length, width, height, &rp, out, out_length,
                                           &rp_eff);
    if (a != VCRT_SUCCESS) return a;
    if (!history_moments || !out_moments || out_moments == out || out_moments == out_length)
        return VCRT_ERROR_INITIALIZATION_FAILED;
    const float* in[7] = {colour, motion, history_colour, history_surface, history_length, albedo,
                          history_moments};
    for (const float* p : in)
        if (p && (p == out || p == out_length || p == out_moments))
            return VCRT_ERROR_INITIALIZATION_FAILED;
    return VCRT_SUCCESS;
}

int32_t vcrt::variance_args(const float* moments, const float* surface, int32_t width,
                            int32_t height, const vcrt_variance_params* params,
                            const float* variance, vcrt_variance_params* eff) {
    if (params) *eff = *params;
    else vcrt_default_variance_params(eff);
    if (eff->struct_size != sizeof(vcrt_variance_params)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!(eff->min_history >= 1.0f && eff->min_history <= 65535.0f))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!(eff->alpha > 0.0f && eff->alpha <= 1.0f)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (width < 1 || width > 65535 || height < 1 || height > 65535 ||
        static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > kMaxPixels)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!moments || !surface || !variance || variance == moments || variance == surface)
        return VCRT_ERROR_INITIALIZATION_FAILED;
    return VCRT_SUCCESS;
}

int32_t vcrt::denoise_variance_args(const float* colour, const float* albedo,
                                    const float* normal_depth, const float* variance,
                                    int32_t width, int32_t height,
                                    const vcrt_denoise_params* params, const float* out,
                                    const float* out_variance, vcrt_denoise_params* eff,
                                    float k4[4]) {
    vcrt_denoise_params def;
    if (!params) {
        vcrt_default_denoise_variance_params(&def);
        params = &def;
    }
    const int32_t a = vcrt::denoise_args(colour, albedo, normal_depth, width, height, params, out,
                                         eff, k4);
    if (a != VCRT_SUCCESS) return a;
    if (!variance || variance == out) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (out_variance) {
        const float* in[5] = {colour, albedo, normal_depth, variance, out};
        for (const float* p : in)
            if (p == out_variance) return VCRT_ERROR_INITIALIZATION_FAILED;
    }
    return VCRT_SUCCESS;
}

vcrt_result vcrt_reproject_moments_host(const float* colour, const float* motion,
                                        const float* history_colour, const float* history_surface,
                                        const float* history_length, const float* albedo,
                                        const float* history_moments, int32_t width,
                                        int32_t height,
                                        const vcrt_reproject_moments_params* params, float* out,
                                        float* out_length, float* out_moments) {
    vcrt_reproject_moments_params pr;
    const int32_t a = vcrt::reproject_moments_args(
        colour, motion, history_colour, history_surface, history_length, albedo, history_moments,
        width, height, params, out, out_length, out_moments, &pr);
    if (a != VCRT_SUCCESS) return a;
    const size_t Wn = static_cast<size_t>(width), Hn = static_cast<size_t>(height);
    const float W = static_cast<float>(width), H = static_cast<float>(height);
    for (size_t p = 0; p < Wn * Hn; p++) {
        const float* m = motion + 4 * p;
        const float* c = colour + 4 * p;
        float sr = c[0], sg = c[1], sb = c[2];
        if (albedo) {
            sr = c[0] / std::fmax(albedo[4 * p], kEps);
            sg = c[1] / std::fmax(albedo[4 * p + 1], kEps);
            sb = c[2] / std::fmax(albedo[4 * p + 2], kEps);
        }
        const float Y = lum(sr, sg, sb);
        const float Y2 = Y * Y;
        float ar = 0.0f, ag = 0.0f, ab = 0.0f, lsum = 0.0f, wsum = 0.0f, m1 = 0.0f, m2 = 0.0f;
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
                const float* mq = history_moments + 4 * q;
                ar = ar + b * hq[0];
                ag = ag + b * hq[1];
                ab = ab + b * hq[2];
                lsum = lsum + b * lq;
                wsum = wsum + b;
                m1 = m1 + b * mq[0];
                m2 = m2 + b * mq[1];
            }
        }
        float N = 1.0f, M1 = Y, M2 = Y2;
        out[4 * p] = c[0];
        out[4 * p + 1] = c[1];
        out[4 * p + 2] = c[2];
        out[4 * p + 3] = c[3];
        if (wsum > 0.0f) {
            const float hr = ar / wsum, hg = ag / wsum, hb = ab / wsum;
            const float L = lsum / wsum;
            N = std::fmin(L + 1.0f, pr.max_history);
            const float rn = 1.0f / N;
            const float al = std::fmax(pr.alpha, rn);
            out[4 * p] = hr + al * (c[0] - hr);
            out[4 * p + 1] = hg + al * (c[1] - hg);
            out[4 * p + 2] = hb + al * (c[2] - hb);
            const float h1 = m1 / wsum, h2 = m2 / wsum;
            const float am = std::fmax(pr.alpha_moments, rn);
            M1 = h1 + am * (Y - h1);
            M2 = h2 + am * (Y2 - h2);
        }
        out_length[p] = N;
        out_moments[4 * p] = M1;
        out_moments[4 * p + 1] = M2;
        out_moments[4 * p + 2] = std::fmax(M2 - M1 * M1, 0.0f);
        out_moments[4 * p + 3] = N;
    }
    return VCRT_SUCCESS;
}

vcrt_result vcrt_variance_host(const float* moments, const float* surface, int32_t width,
                               int32_t height, const vcrt_variance_params* params,
                               float* variance) {
    vcrt_variance_params pr;
    const int32_t a = vcrt::variance_args(moments, surface, width, height, params, variance, &pr);
    if (a != VCRT_SUCCESS) return a;
    const size_t W = static_cast<size_t>(width);
    for (int64_t y = 0; y < height; y++) {
        for (int64_t x = 0; x < width; x++) {
            const size_t p = static_cast<size_t>(y) * W + static_cast<size_t>(x);
            const float* mp = moments + 4 * p;
            const float N = std::fmax(mp[3], 1.0f);
            float v = mp[2];
            if (!(mp[3] >= pr.min_history)) {
                const float key = surface[4 * p];
                float S1 = 0.0f, S2 = 0.0f, n = 0.0f;
                for (int dy = -3; dy <= 3; dy++) {
                    const int64_t qy = y + dy;
                    if (qy < 0 || qy >= height) continue;
                    for (int dx = -3; dx <= 3; dx++) {
                        const int64_t qx = x + dx;
                        if (qx < 0 || qx >= width) continue;
                        const size_t q = static_cast<size_t>(qy) * W + static_cast<size_t>(qx);
                        // the centre always counts (a NaN key equals nothing, itself included)
                        if (q != p && !(surface[4 * q] == key)) continue;
                        S1 = S1 + moments[4 * q];
                        S2 = S2 + moments[4 * q + 1];
                        n = n + 1.0f;
                    }
                }
                const float a1 = S1 / n, a2 = S2 / n;
                const float sv = std::fmax(a2 - a1 * a1, 0.0f);
                const float boost = pr.min_history / N;
                v = sv * boost;
            }
            const float rn = 1.0f / N;
            variance[p] = v * std::fmax(pr.alpha, rn);
        }
    }
    return VCRT_SUCCESS;
}

int32_t vcrt::sample_count_args(const float* variance, uint64_t elements,
                                const vcrt_sample_count_params* params, const uint16_t* counts,
                                float* k) {
    if (!params) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (params->struct_size != sizeof(vcrt_sample_count_params))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!(params->target > 0.0f) || std::isinf(params->target))  // (a NaN fails)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (params->min_count > params->max_count || params->max_count > 256u)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (elements == 0 || elements > (uint64_t{1} << 31)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    const float tt = params->target * params->target;
    *k = 1.0f / tt;
    // a target whose square leaves fp32's range has no k to multiply by
    if (!(*k > 0.0f) || std::isinf(*k)) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!variance || !counts || static_cast<const void*>(variance) == counts)
        return VCRT_ERROR_INITIALIZATION_FAILED;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_sample_counts_host(const float* variance, uint32_t elements,
                                    const vcrt_sample_count_params* params, uint16_t* counts,
                                    vcrt_sample_count_stats* stats) {
    float k;
    const int32_t a = vcrt::sample_count_args(variance, elements, params, counts, &k);
    if (a != VCRT_SUCCESS) return a;
    uint64_t total = 0;
    for (size_t e = 0; e < elements; e++) {
        const uint32_t c = vcrt::sample_count_of_variance(variance[e], k, params->min_count,
                                                          params->max_count);
        counts[e] = static_cast<uint16_t>(c);
        total += c;
    }
    if (stats) {
        *stats = vcrt_sample_count_stats{};
        stats->total = total;
    }
    return VCRT_SUCCESS;
}

vcrt_result vcrt_denoise_variance_host(const float* colour, const float* albedo,
                                       const float* normal_depth, const float* variance,
                                       int32_t width, int32_t height,
                                       const vcrt_denoise_params* params, float* out,
                                       float* out_variance) {
    vcrt_denoise_params pr;
    float k4[4];
    const int32_t a = vcrt::denoise_variance_args(colour, albedo, normal_depth, variance, width,
                                                  height, params, out, out_variance, &pr, k4);
    if (a != VCRT_SUCCESS) return a;
    const size_t W = static_cast<size_t>(width), H = static_cast<size_t>(height);
    const float* nd = normal_depth;
    const bool on_n = nd && k4[0] != 0.0f, on_z = nd && k4[1] != 0.0f;
    const bool on_a = albedo && k4[2] != 0.0f;
    const bool on_c = pr.sigma_colour != 0.0f;
    const bool demod = pr.demodulate != 0 && albedo;
    const float sc2 = pr.sigma_colour * pr.sigma_colour;

    // pass 0's input: the signal, the variance in its fourth channel
    std::vector<Sig> s(W * H), t(W * H);
    for (size_t p = 0; p < W * H; p++) {
        if (demod)
            s[p] = {colour[4 * p] / std::fmax(albedo[4 * p], kEps),
                    colour[4 * p + 1] / std::fmax(albedo[4 * p + 1], kEps),
                    colour[4 * p + 2] / std::fmax(albedo[4 * p + 2], kEps), 0.0f};
        else
            s[p] = {colour[4 * p], colour[4 * p + 1], colour[4 * p + 2], 0.0f};
        s[p].v = std::fmax(variance[p], 0.0f);
    }

    for (int32_t l = 0; l < pr.levels; l++) {
        const int64_t step = int64_t{1} << l;
        for (int64_t y = 0; y < height; y++) {
            for (int64_t x = 0; x < width; x++) {
                const size_t p = static_cast<size_t>(y) * W + static_cast<size_t>(x);
                float kv = 0.0f, yp = 0.0f;
                if (on_c) {
                    float gsum = 0.0f, gw = 0.0f;
                    for (int dy = -1; dy <= 1; dy++) {
                        const int64_t qy = y + dy;
                        if (qy < 0 || qy >= height) continue;
                        for (int dx = -1; dx <= 1; dx++) {
                            const int64_t qx = x + dx;
                            if (qx < 0 || qx >= width) continue;
                            const size_t q = static_cast<size_t>(qy) * W + static_cast<size_t>(qx);
                            const float h3 = kK3[dx + 1] * kK3[dy + 1];
                            gsum = gsum + h3 * s[q].v;
                            gw = gw + h3;
                        }
                    }
                    const float g = gsum / gw;
                    float den = sc2 * g;
                    den = den + kVarEps;
                    kv = 1.0f / den;
                    yp = lum(s[p].r, s[p].g, s[p].b);
                }
                float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f, vacc = 0.0f;
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
                            const float dyl = yp - lum(s[q].r, s[q].g, s[q].b);
                            tl = (dyl * dyl) * kv;
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
                        vacc = vacc + (w * w) * s[q].v;
                    }
                }
                t[p] = {ar / wsum, ag / wsum, ab / wsum, vacc / (wsum * wsum)};
            }
        }
        s.swap(t);
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
        if (out_variance) out_variance[p] = s[p].v;
    }
    return VCRT_SUCCESS;
}
