// denoise_abi.h -- the argument block of the denoise kernels (denoise.hip), shared with the host
// (image_passes.cpp vcrt_denoise; the launches: image_pass_plan.hpp). One struct for both kernels;
// one launch per pass.
#pragma once

#include <cstdint>

struct vcrt_denoise_params;

namespace vcrt {

// The checks vcrt_denoise_host, vcrt_denoise and vcrt_denoise_device share (denoise.cpp): the
// format errors first, then the pointers. *eff receives the parameters in effect (the defaults
// for a null params), k4 their scales. A VkResult.
int32_t denoise_args(const float* colour, const float* albedo, const float* normal_depth,
                     int32_t width, int32_t height, const vcrt_denoise_params* params,
                     const float* out, vcrt_denoise_params* eff, float k4[4]);

// The direct kernel's workgroup: four waves, each a 64-pixel segment of one row, so every tap is
// one coalesced 16-B load per plane. The LDS kernel's workgroup covers 32 x 8 pixels: its footprint
// with the halo of 2 step is (32 + 4 step) x (8 + 4 step) entries per staged plane.
constexpr uint32_t kDenoiseThreads = 256;
constexpr uint32_t kDenoiseRowW = 64, kDenoiseRowH = 4;
constexpr uint32_t kDenoiseTileW = 32, kDenoiseTileH = 8;
constexpr uint32_t kDenoiseLdsMaxStep = 2;  // the LDS kernel takes step 1 and 2

// DenoiseParams.flags
constexpr uint32_t kDenoiseNormal = 1u;      // the normal term is on (k_normal != 0, a plane)
constexpr uint32_t kDenoiseDepth = 2u;       // the depth term
constexpr uint32_t kDenoiseAlbedo = 4u;      // the albedo term
constexpr uint32_t kDenoiseColour = 8u;      // the colour term (kl != 0)
constexpr uint32_t kDenoiseDemodIn = 16u;    // pass 0: the input is colour / max(albedo, eps)
constexpr uint32_t kDenoiseModOut = 32u;     // the last pass: the output is s * max(albedo, eps)
constexpr uint32_t kDenoiseLast = 64u;       // the last pass: out.a = colour.a (else 0: scratch)

struct DenoiseParams {
    const float* in;            // [height][width][4] this pass's input (pass 0: the colour plane)
    const float* colour;        // the caller's colour plane: the alpha the last pass carries
    const float* albedo;        // may be null (then no albedo flag is set)
    const float* normal_depth;  // may be null
    float* out;                 // [height][width][4]
    uint32_t width, height;
    uint32_t step;              // 1 << pass
    uint32_t flags;
    float k_normal, k_depth, k_albedo, kl;  // kl = k_colour * 4^pass
    uint32_t tiles_x;           // workgroups per row of workgroups
};

}  // namespace vcrt
