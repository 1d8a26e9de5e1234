// reproject_abi.h -- the argument block of the temporal accumulation kernel (reproject.hip), shared
// with the host (image_passes.cpp vcrt_reproject; the launch: image_pass_plan.hpp). One launch per
// call.
#pragma once

#include <cstdint>

struct vcrt_reproject_params;

namespace vcrt {

// The checks vcrt_reproject_host, vcrt_reproject and vcrt_reproject_device share (reproject.cpp):
// the format errors first, then the pointers. *eff receives the parameters in effect (the defaults
// for a null params). A VkResult.
int32_t reproject_args(const float* colour, const float* motion, const float* history_colour,
                       const float* history_surface, const float* history_length, int32_t width,
                       int32_t height, const vcrt_reproject_params* params, const float* out,
                       const float* out_length, vcrt_reproject_params* eff);

// The workgroup: four waves, each a 64-pixel segment of one row, so the pixel's own planes are
// one coalesced 16-B load per lane and a tap's are nearly so (the motion of neighbours is close).
constexpr uint32_t kReprojectThreads = 256;
constexpr uint32_t kReprojectRowW = 64, kReprojectRowH = 4;
// ReprojectParams.tallies: block b adds to slot b % kReprojectTallySlots, each slot a cache line
// of its own (atomics on one address serialise: vcrt_kernel_abi.h kFeatureTallySlots).
constexpr uint32_t kReprojectTallySlots = 256;

struct ReprojectParams {
    const float* colour;           // [height][width][4] the new frame
    const float* motion;           // [height][width][4] (px, py, z', key), 0 key: no history
    const float* history_colour;   // [height][width][4] the previous call's out
    const float* history_surface;  // [height][width][4] (key, t, -, -) of the previous frame
    const float* history_length;   // [height][width]    the previous call's out_length
    float* out;                    // [height][width][4]
    float* out_length;             // [height][width]
    uint32_t width, height;
    float alpha, max_history, depth_tolerance;
    uint32_t tiles_x;              // workgroups per row of workgroups
    unsigned long long* tallies;   // [kReprojectTallySlots][8]: per slot (64 B), [0] pixels that
                                   //   accepted history (per wave); zeroed before the launch,
                                   //   summed over the slots by the host. Null: not counted
};

}  // namespace vcrt
