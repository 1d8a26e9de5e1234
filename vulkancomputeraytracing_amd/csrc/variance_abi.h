// variance_abi.h -- the argument blocks of the variance-guided kernels (variance.hip), shared with
// the host (image_passes.cpp vcrt_reproject_moments, vcrt_variance, vcrt_denoise_variance; the
// launches: image_pass_plan.hpp), and the checks
// every form of the three calls shares (variance.cpp).
#pragma once

#include <cmath>
#include <cstdint>

struct vcrt_sample_count_params;
struct vcrt_reproject_moments_params;
struct vcrt_variance_params;
struct vcrt_denoise_params;

namespace vcrt {

// The checks of vcrt_reproject_moments{_host,,_device}: the format errors first, then the
// pointers. *eff receives the parameters in effect (the defaults for a null params). A VkResult.
int32_t reproject_moments_args(const float* colour, const float* motion,
                               const float* history_colour, const float* history_surface,
                               const float* history_length, const float* albedo,
                               const float* history_moments, int32_t width, int32_t height,
                               const vcrt_reproject_moments_params* params, const float* out,
                               const float* out_length, const float* out_moments,
                               vcrt_reproject_moments_params* eff);
// The checks of vcrt_variance{_host,,_device}, the same way.
int32_t variance_args(const float* moments, const float* surface, int32_t width, int32_t height,
                      const vcrt_variance_params* params, const float* variance,
                      vcrt_variance_params* eff);
// The checks of vcrt_denoise_variance{_host,,_device}: vcrt_denoise's (denoise_abi.h denoise_args,
// a null params taking vcrt_default_denoise_variance_params), then the two variance planes.
int32_t denoise_variance_args(const float* colour, const float* albedo, const float* normal_depth,
                              const float* variance, int32_t width, int32_t height,
                              const vcrt_denoise_params* params, const float* out,
                              const float* out_variance, vcrt_denoise_params* eff, float k4[4]);

// vcrt_reproject_moments_pass: vcrt_reproject_pass's workgroup (four waves, each a 64-pixel
// segment of a row) and tally slots.
constexpr uint32_t kMomentsThreads = 256;
constexpr uint32_t kMomentsRowW = 64, kMomentsRowH = 4;
constexpr uint32_t kMomentsTallySlots = 256;

struct ReprojectMomentsParams {
    const float* colour;           // [height][width][4] the new frame
    const float* motion;           // [height][width][4] (px, py, z', key), 0 key: no history
    const float* history_colour;   // [height][width][4] the previous call's out
    const float* history_surface;  // [height][width][4] (key, t, -, -) of the previous frame
    const float* history_length;   // [height][width]    the previous call's out_length
    const float* albedo;           // [height][width][4] may be null: the signal is the colour
    const float* history_moments;  // [height][width][4] the previous call's out_moments
    float* out;                    // [height][width][4]
    float* out_length;             // [height][width]
    float* out_moments;            // [height][width][4] (M1, M2, max(M2 - M1^2, 0), N)
    uint32_t width, height;
    float alpha, max_history, depth_tolerance, alpha_moments;
    uint32_t tiles_x;              // workgroups per row of workgroups
    unsigned long long* tallies;   // [kMomentsTallySlots][8]: per slot (64 B), [0] pixels that
                                   //   accepted history (per wave); null: not counted
};

// vcrt_variance_pass (VCRT_VARIANCE_LDS=0): the same workgroup shape; the 49 taps are read
// directly.
constexpr uint32_t kVarianceThreads = 256;
constexpr uint32_t kVarianceRowW = 64, kVarianceRowH = 4;
constexpr uint32_t kVarianceTallySlots = 256;
constexpr int32_t kVarianceRadius = 3;
// vcrt_variance_pass_lds (the default, by measurement: profiles/variance.json): a workgroup covers 32 x 8 pixels and stages them
// with their halo of 3, (32 + 6) x (8 + 6) float4 entries (M1, M2, key, -), in dynamic LDS.
constexpr uint32_t kVarianceTileW = 32, kVarianceTileH = 8;
constexpr uint32_t kVarianceLdsBytes =
    (kVarianceTileW + 2u * kVarianceRadius) * (kVarianceTileH + 2u * kVarianceRadius) * 16u;

struct VarianceParams {
    const float* moments;   // [height][width][4]
    const float* surface;   // [height][width][4] (key, t, -, -) of this frame
    float* variance;        // [height][width]
    uint32_t width, height;
    float min_history, alpha;
    uint32_t tiles_x;
    unsigned long long* tallies;  // [kVarianceTallySlots][8]: [0] pixels that took the spatial
                                  //   estimate (per wave); null: not counted
};

// vcrt_denoise_var_pass and vcrt_denoise_var_pass_lds: the workgroups, tiles and flags of
// denoise_abi.h (kDenoise*); kDenoiseColour means sigma_colour != 0. Further flags:
constexpr uint32_t kDenoiseVarIn = 128u;  // pass 0: s.w = fmaxf(variance[p], 0), in.w is alpha

struct DenoiseVarParams {
    const float* in;            // [height][width][4] this pass's input (pass 0: the colour plane)
    const float* colour;        // the caller's colour plane: the alpha the last pass carries
    const float* albedo;        // may be null (then no albedo flag is set)
    const float* normal_depth;  // may be null
    const float* variance;      // [height][width] pass 0's fourth channel
    float* out;                 // [height][width][4]
    float* out_variance;        // [height][width] the last pass's fourth channel; may be null
    uint32_t width, height;
    uint32_t step;              // 1 << pass
    uint32_t flags;
    float k_normal, k_depth, k_albedo;
    float sc2;                  // sigma_colour * sigma_colour: it does not halve
    uint32_t tiles_x;           // workgroups per row of workgroups
};

// The checks of vcrt_sample_counts{_host,,_device}: the format errors first, then the pointers.
// *k receives 1 / (target * target) (the product, then one correctly rounded division).
int32_t sample_count_args(const float* variance, uint64_t elements,
                          const vcrt_sample_count_params* params, const uint16_t* counts,
                          float* k);
// One element of vcrt_sample_counts (vcrt.h): the host function's and the kernel's statement.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t sample_count_of_variance(float variance, float k, uint32_t min_count,
                                         uint32_t max_count) {
    const float v = fmaxf(variance, 0.0f);  // (a NaN gives 0)
    const float t = v * k;
    const uint32_t c = t >= static_cast<float>(max_count) ? max_count
                                                          : static_cast<uint32_t>(ceilf(t));
    return c > min_count ? c : min_count;
}

// vcrt_sample_counts_pass: element-wise over a grid-stride loop; a wave adds its counts to the
// block's tally slot.
constexpr uint32_t kSampleCountThreads = 256;
constexpr uint32_t kSampleCountTallySlots = 256;
constexpr uint32_t kSampleCountMaxBlocks = 4096;

struct SampleCountParams {
    const float* variance;  // [elements]
    uint16_t* counts;       // [elements]
    uint32_t elements;      // <= 2^31
    float k;                // 1 / target^2
    uint32_t min_count, max_count;
    unsigned long long* tallies;  // [kSampleCountTallySlots][8]: [0] the sum of the counts
};

}  // namespace vcrt
