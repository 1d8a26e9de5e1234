// image_pass_plan.hpp -- what each image-space pass launches, as data. Pure functions of the
// caller's planes, the frame size and the checked parameters: no HIP runtime and no renderer
// state, so the library (image_passes.cpp) and the CPU drivers that run the kernels on host
// threads (tests/*_host_driver.cpp) make the same launches from the same code. The tallies
// pointer of a params block is left null: whoever runs the launch points it at its counters.
#pragma once

#include <cstdint>

#include "denoise_abi.h"
#include "reproject_abi.h"
#include "variance_abi.h"
#include "vcrt.h"

namespace vcrt {

// One launch: the filled kernel params, which kernel of the pass's pair takes them (the one that
// stages its footprint in LDS, else the direct one), and the launch geometry.
template <typename Params>
struct PassLaunch {
    Params params;
    bool lds;
    uint32_t grid, block, lds_bytes;
};

// tiles_x of the params and the grid of w x h pixels in workgroups of tw x th
template <typename Params>
inline void tile_grid(PassLaunch<Params>& l, uint32_t tw, uint32_t th) {
    l.params.tiles_x = (l.params.width + tw - 1u) / tw;
    l.grid = l.params.tiles_x * ((l.params.height + th - 1u) / th);
}

inline PassLaunch<ReprojectParams> reproject_plan(
    const float* colour, const float* motion, const float* history_colour,
    const float* history_surface, const float* history_length, int32_t width, int32_t height,
    const vcrt_reproject_params& pr, float* out, float* out_length) {
    PassLaunch<ReprojectParams> l{};
    ReprojectParams& p = l.params;
    p.colour = colour;
    p.motion = motion;
    p.history_colour = history_colour;
    p.history_surface = history_surface;
    p.history_length = history_length;
    p.out = out;
    p.out_length = out_length;
    p.width = static_cast<uint32_t>(width);
    p.height = static_cast<uint32_t>(height);
    p.alpha = pr.alpha;
    p.max_history = pr.max_history;
    p.depth_tolerance = pr.depth_tolerance;
    l.block = kReprojectThreads;
    tile_grid(l, kReprojectRowW, kReprojectRowH);
    return l;
}

inline PassLaunch<ReprojectMomentsParams> reproject_moments_plan(
    const float* colour, const float* motion, const float* history_colour,
    const float* history_surface, const float* history_length, const float* albedo,
    const float* history_moments, int32_t width, int32_t height,
    const vcrt_reproject_moments_params& pr, float* out, float* out_length, float* out_moments) {
    PassLaunch<ReprojectMomentsParams> l{};
    ReprojectMomentsParams& p = l.params;
    p.colour = colour;
    p.motion = motion;
    p.history_colour = history_colour;
    p.history_surface = history_surface;
    p.history_length = history_length;
    p.albedo = albedo;
    p.history_moments = history_moments;
    p.out = out;
    p.out_length = out_length;
    p.out_moments = out_moments;
    p.width = static_cast<uint32_t>(width);
    p.height = static_cast<uint32_t>(height);
    p.alpha = pr.alpha;
    p.max_history = pr.max_history;
    p.depth_tolerance = pr.depth_tolerance;
    p.alpha_moments = pr.alpha_moments;
    l.block = kMomentsThreads;
    tile_grid(l, kMomentsRowW, kMomentsRowH);
    return l;
}

// lds: the taps read from a staged footprint (vcrt_variance_pass_lds), else directly. Same bits.
inline PassLaunch<VarianceParams> variance_plan(const float* moments, const float* surface,
                                                int32_t width, int32_t height,
                                                const vcrt_variance_params& pr, bool lds,
                                                float* variance) {
    PassLaunch<VarianceParams> l{};
    VarianceParams& p = l.params;
    p.moments = moments;
    p.surface = surface;
    p.variance = variance;
    p.width = static_cast<uint32_t>(width);
    p.height = static_cast<uint32_t>(height);
    p.min_history = pr.min_history;
    p.alpha = pr.alpha;
    l.lds = lds;
    l.block = kVarianceThreads;
    l.lds_bytes = lds ? kVarianceLdsBytes : 0u;
    tile_grid(l, lds ? kVarianceTileW : kVarianceRowW, lds ? kVarianceTileH : kVarianceRowH);
    return l;
}

// ---- the two a-trous filters: vcrt_denoise and vcrt_denoise_variance ---------------------------

constexpr int32_t kAtrousMaxLevels = 8;  // vcrt_denoise_params.levels at most; pass_ms[8]

template <typename Params>
struct AtrousPlan {
    PassLaunch<Params> pass[kAtrousMaxLevels];
    int32_t passes;      // pr.levels
    int32_t lds_passes;  // of them, the leading ones the LDS kernel takes
};

// What the passes of the two filters differ in: the colour term and the variance planes.
// vcrt_denoise's colour scale is kl = k4[3] * 4^pass, and the term is on while it is not 0.
inline void atrous_colour_term(DenoiseParams& p, const vcrt_denoise_params&, float kl,
                               const float*, float*) {
    p.kl = kl;
    if (kl != 0.0f) p.flags |= kDenoiseColour;
}
// vcrt_denoise_variance's is sigma_colour^2 in every pass (the variance carries the level's
// scale); pass 0 takes the variance plane in, the last pass writes it out.
inline void atrous_colour_term(DenoiseVarParams& p, const vcrt_denoise_params& pr, float,
                               const float* variance, float* out_variance) {
    p.variance = variance;
    p.out_variance = out_variance;
    p.sc2 = pr.sigma_colour * pr.sigma_colour;
    if (pr.sigma_colour != 0.0f) p.flags |= kDenoiseColour;
    if (p.step == 1u) p.flags |= kDenoiseVarIn;
}

// The passes of an a-trous filter of pr.levels levels: pass l reads the plane pass l - 1 wrote --
// the colour, the scratch planes in turn (scratch[0] is needed from two levels on, scratch[1]
// from three), the output. The first min(lds_passes, levels) passes, those of step 1 and 2 at
// most, stage their footprint in LDS. variance and out_variance: vcrt_denoise_variance's.
template <typename Params>
inline AtrousPlan<Params> atrous_plan(const float* colour, const float* albedo,
                                      const float* normal_depth, const float* variance,
                                      int32_t width, int32_t height, const vcrt_denoise_params& pr,
                                      const float k4[4], float* const scratch[2],
                                      int32_t lds_passes, float* out, float* out_variance) {
    AtrousPlan<Params> plan{};
    const int32_t levels = plan.passes = pr.levels;
    const bool demod = pr.demodulate != 0 && albedo;
    uint32_t terms = 0;
    if (normal_depth && k4[0] != 0.0f) terms |= kDenoiseNormal;
    if (normal_depth && k4[1] != 0.0f) terms |= kDenoiseDepth;
    if (albedo && k4[2] != 0.0f) terms |= kDenoiseAlbedo;
    const float* in = colour;
    float kl = k4[3];
    for (int32_t l = 0; l < levels; l++) {
        const bool last = l == levels - 1;
        PassLaunch<Params>& launch = plan.pass[l];
        Params& p = launch.params;
        p.in = in;
        p.colour = colour;
        p.albedo = albedo;
        p.normal_depth = normal_depth;
        p.out = last ? out : scratch[l & 1];
        p.width = static_cast<uint32_t>(width);
        p.height = static_cast<uint32_t>(height);
        p.step = 1u << l;
        p.flags = terms | (demod && l == 0 ? kDenoiseDemodIn : 0u) |
                  (demod && last ? kDenoiseModOut : 0u) | (last ? kDenoiseLast : 0u);
        p.k_normal = k4[0];
        p.k_depth = k4[1];
        p.k_albedo = k4[2];
        atrous_colour_term(p, pr, kl, variance, out_variance);
        launch.block = kDenoiseThreads;
        launch.lds = l < lds_passes && p.step <= kDenoiseLdsMaxStep;
        if (launch.lds) {
            plan.lds_passes++;
            const uint32_t halo = 2u * p.step;
            const uint32_t entries = (kDenoiseTileW + 2u * halo) * (kDenoiseTileH + 2u * halo);
            const bool guides = (terms & (kDenoiseNormal | kDenoiseDepth)) != 0;
            const uint32_t planes = 1u + ((terms & kDenoiseAlbedo) ? 1u : 0u) + (guides ? 1u : 0u);
            launch.lds_bytes = entries * planes * 16u;  // float4 entries
            tile_grid(launch, kDenoiseTileW, kDenoiseTileH);
        } else {
            tile_grid(launch, kDenoiseRowW, kDenoiseRowH);
        }
        in = p.out;
        kl = kl * 4.0f;
    }
    return plan;
}

inline AtrousPlan<DenoiseParams> denoise_plan(const float* colour, const float* albedo,
                                              const float* normal_depth, int32_t width,
                                              int32_t height, const vcrt_denoise_params& pr,
                                              const float k4[4], float* const scratch[2],
                                              int32_t lds_passes, float* out) {
    return atrous_plan<DenoiseParams>(colour, albedo, normal_depth, nullptr, width, height, pr, k4,
                                      scratch, lds_passes, out, nullptr);
}

inline AtrousPlan<DenoiseVarParams> denoise_variance_plan(
    const float* colour, const float* albedo, const float* normal_depth, const float* variance,
    int32_t width, int32_t height, const vcrt_denoise_params& pr, const float k4[4],
    float* const scratch[2], int32_t lds_passes, float* out, float* out_variance) {
    return atrous_plan<DenoiseVarParams>(colour, albedo, normal_depth, variance, width, height, pr,
                                         k4, scratch, lds_passes, out, out_variance);
}

}  // namespace vcrt
