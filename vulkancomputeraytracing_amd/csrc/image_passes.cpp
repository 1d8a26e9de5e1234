// image_passes.cpp -- the host side of the passes over caller-supplied planes of width x height:
// vcrt_denoise, vcrt_reproject, vcrt_reproject_moments, vcrt_variance, vcrt_denoise_variance, and
// the element-wise vcrt_sample_counts. They touch neither the scene nor the frame. What a pass
// launches is image_pass_plan.hpp's; here are the executor that makes a plan's launches on the
// renderer's stream and one body per pass behind both exported forms (their staging:
// pass_staging.hpp). Every form checks in the same order, which the refused-call tests pin: the
// pass's own argument check (denoise.cpp, reproject.cpp, variance.cpp), for the device form the
// alignment, then the renderer and its module, then the kernel.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <iterator>
#include <vector>

#include "image_pass_plan.hpp"
#include "renderer_state.hpp"

namespace {

using vcrt::DeviceBuffer;
using vcrt::g;
using vcrt::in1;
using vcrt::in4;
using vcrt::misaligned;
using vcrt::name_stats;
using vcrt::out1;
using vcrt::out4;
using vcrt::pass_ready;
using vcrt::Plane;
using vcrt::plane_of;
using vcrt::Staging;
using Clock = std::chrono::steady_clock;

// ---- the executor ------------------------------------------------------------------------------

// A one-launch plan's launch, waited for. Without stats nothing is counted or timed (unless the
// kernel always tallies); with them the kernel's `slots` tally slots (64 B each, [0] counted) are
// zeroed, bound, read back and summed into *tally, and *ms is the kernel time.
template <typename Params>
VkResult run(hipFunction_t f, vcrt::PassLaunch<Params>& l,
             DeviceBuffer<unsigned long long>& counters, size_t slots, bool stats,
             bool always_tallies, unsigned long long* tally, float* ms) {
    if (!stats && !always_tallies) {
        const VkResult r = vcrt::launch(f, l.grid, l.block, l.lds_bytes, l.params);
        if (r != VK_SUCCESS) return r;
        VCRT_TRY(hipStreamSynchronize(g.stream));
        return VK_SUCCESS;
    }
    std::vector<unsigned long long> host(8 * slots);
    const VkResult r = vcrt::timed_launch(
        f, l.grid, l.block, l.lds_bytes, l.params, counters, host.size(),
        [&l](unsigned long long* c) { l.params.tallies = c; }, stats ? host.data() : nullptr, ms);
    if (r != VK_SUCCESS) return r;
    for (size_t s = 0; s < host.size(); s += 8) *tally += host[s];
    return VK_SUCCESS;
}

// VCRT_DENOISE_LDS: how many leading passes stage their footprint in LDS (at most the passes of
// step 1 and 2). Unset: both -- see tools/denoise_bench.py and profiles/denoise.json for the A/B.
int32_t denoise_lds_passes() {
    static_assert(vcrt::kDenoiseLdsMaxStep == 2, "the LDS kernel takes passes 0 and 1");
    int32_t n = 2;
    if (const char* e = std::getenv("VCRT_DENOISE_LDS")) n = std::atoi(e);
    return std::min(std::max(n, 0), 2);
}

// The scratch planes an a-trous filter of `levels` levels goes through between its first and its
// last pass (the denoiser's, kept and grown only).
VkResult atrous_scratch(int32_t levels, size_t pixels, float* scratch[2]) {
    for (int32_t b = 0; b < std::min(levels - 1, 2); b++)
        VCRT_TRY(g.d_dn_scratch[b].reserve(pixels));
    scratch[0] = plane_of(g.d_dn_scratch[0]);
    scratch[1] = plane_of(g.d_dn_scratch[1]);
    return VK_SUCCESS;
}

// An a-trous plan's launches, an event around each; returns when the last is done.
template <typename Params>
VkResult run(hipFunction_t direct, hipFunction_t lds, vcrt::AtrousPlan<Params>& plan,
             const char* name, vcrt_denoise_stats* stats) {
    VCRT_TRY(g.ev_dn[0].create());
    VCRT_TRY(hipEventRecord(g.ev_dn[0].get(), g.stream));
    for (int32_t l = 0; l < plan.passes; l++) {
        vcrt::PassLaunch<Params>& p = plan.pass[l];
        VCRT_TRY(g.ev_dn[l + 1].create());
        const VkResult r =
            vcrt::launch(p.lds ? lds : direct, p.grid, p.block, p.lds_bytes, p.params);
        if (r != VK_SUCCESS) return r;
        VCRT_TRY(hipEventRecord(g.ev_dn[l + 1].get(), g.stream));
    }
    VCRT_TRY(hipStreamSynchronize(g.stream));
    if (stats) {
        name_stats(stats, name);
        stats->passes = plan.passes;
        stats->lds_passes = plan.lds_passes;
        float ms = 0.f;
        VCRT_TRY(hipEventElapsedTime(&ms, g.ev_dn[0].get(), g.ev_dn[plan.passes].get()));
        stats->kernel_ms = ms;
        for (int32_t l = 0; l < plan.passes; l++) {
            VCRT_TRY(hipEventElapsedTime(&ms, g.ev_dn[l].get(), g.ev_dn[l + 1].get()));
            stats->pass_ms[l] = ms;
        }
    }
    return VK_SUCCESS;
}

// ---- the passes: host = the form that takes host planes ----------------------------------------

vcrt_result denoise(bool host, const float* colour, const float* albedo, const float* normal_depth,
                    int32_t width, int32_t height, const vcrt_denoise_params* params, float* out,
                    vcrt_denoise_stats* stats) {
    const auto t0 = Clock::now();
    vcrt_denoise_params pr;
    float k4[4];
    const vcrt_result a = vcrt::denoise_args(colour, albedo, normal_depth, width, height, params,
                                             out, &pr, k4);
    if (a != VCRT_SUCCESS) return a;
    // the kernels' 16-byte loads and stores
    const vcrt_result c = pass_ready(!host && misaligned({colour, albedo, normal_depth, out}, 15u),
                                     g.begun && g.stage.module, g.k_denoise_pass);
    if (c != VCRT_SUCCESS) return c;
    const size_t pixels = static_cast<size_t>(width) * static_cast<size_t>(height);
    Staging s(g.staging, g.stream);
    float* scratch[2];
    VkResult r = s.begin(host, pixels, {in4(colour), in4(albedo), in4(normal_depth), out4(out)});
    if (r == VK_SUCCESS) r = atrous_scratch(pr.levels, pixels, scratch);
    if (r != VK_SUCCESS) return r;
    auto plan = vcrt::denoise_plan(s.at(0), s.at(1), s.at(2), width, height, pr, k4, scratch,
                                   denoise_lds_passes(), s.at(3));
    r = run(g.k_denoise_pass, g.k_denoise_pass_lds, plan, "vcrt_denoise_pass", stats);
    return finish(r, s, stats, t0);
}

vcrt_result reproject(bool host, const float* colour, const float* motion,
                      const float* history_colour, const float* history_surface,
                      const float* history_length, int32_t width, int32_t height,
                      const vcrt_reproject_params* params, float* out, float* out_length,
                      vcrt_reproject_stats* stats) {
    const auto t0 = Clock::now();
    vcrt_reproject_params pr;
    const vcrt_result a = vcrt::reproject_args(colour, motion, history_colour, history_surface,
                                               history_length, width, height, params, out,
                                               out_length, &pr);
    if (a != VCRT_SUCCESS) return a;
    // the kernel's 16-byte loads and stores of the float4 planes, 4-byte ones of the lengths
    const vcrt_result c = pass_ready(
        !host && (misaligned({colour, motion, history_colour, history_surface, out}, 15u) ||
                  misaligned({history_length, out_length}, 3u)),
        g.begun && g.stage.module, g.k_reproject_pass);
    if (c != VCRT_SUCCESS) return c;
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, static_cast<size_t>(width) * static_cast<size_t>(height),
                         {in4(colour), in4(motion), in4(history_colour), in4(history_surface),
                          in1(history_length), out4(out), out1(out_length)});
    if (r != VK_SUCCESS) return r;
    auto l = vcrt::reproject_plan(s.at(0), s.at(1), s.at(2), s.at(3), s.at(4), width, height, pr,
                                  s.at(5), s.at(6));
    unsigned long long accepted = 0;
    float ms = 0.f;
    r = run(g.k_reproject_pass, l, g.d_rp_counters, vcrt::kReprojectTallySlots, stats != nullptr,
            false, &accepted, &ms);
    if (r == VK_SUCCESS && stats) {
        name_stats(stats, "vcrt_reproject_pass");
        stats->kernel_ms = ms;
        stats->accepted_pixels = accepted;
    }
    return finish(r, s, stats, t0);
}

vcrt_result reproject_moments(bool host, const float* colour, const float* motion,
                              const float* history_colour, const float* history_surface,
                              const float* history_length, const float* albedo,
                              const float* history_moments, int32_t width, int32_t height,
                              const vcrt_reproject_moments_params* params, float* out,
                              float* out_length, float* out_moments,
                              vcrt_reproject_stats* stats) {
    const auto t0 = Clock::now();
    vcrt_reproject_moments_params pr;
    const vcrt_result a = vcrt::reproject_moments_args(
        colour, motion, history_colour, history_surface, history_length, albedo, history_moments,
        width, height, params, out, out_length, out_moments, &pr);
    if (a != VCRT_SUCCESS) return a;
    // the kernel's 16-byte loads and stores of the float4 planes, 4-byte ones of the lengths
    const vcrt_result c = pass_ready(
        !host && (misaligned({colour, motion, history_colour, history_surface, albedo,
                              history_moments, out, out_moments}, 15u) ||
                  misaligned({history_length, out_length}, 3u)),
        g.begun && g.stage.module, g.k_reproject_moments_pass);
    if (c != VCRT_SUCCESS) return c;
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, static_cast<size_t>(width) * static_cast<size_t>(height),
                         {in4(colour), in4(motion), in4(history_colour), in4(history_surface),
                          in1(history_length), in4(albedo), in4(history_moments), out4(out),
                          out1(out_length), out4(out_moments)});
    if (r != VK_SUCCESS) return r;
    auto l = vcrt::reproject_moments_plan(s.at(0), s.at(1), s.at(2), s.at(3), s.at(4), s.at(5),
                                          s.at(6), width, height, pr, s.at(7), s.at(8), s.at(9));
    unsigned long long accepted = 0;
    float ms = 0.f;
    r = run(g.k_reproject_moments_pass, l, g.d_rp_counters, vcrt::kMomentsTallySlots,
            stats != nullptr, false, &accepted, &ms);
    if (r == VK_SUCCESS && stats) {
        name_stats(stats, "vcrt_reproject_moments_pass");
        stats->kernel_ms = ms;
        stats->accepted_pixels = accepted;
    }
    return finish(r, s, stats, t0);
}

vcrt_result variance(bool host, const float* moments, const float* surface, int32_t width,
                     int32_t height, const vcrt_variance_params* params, float* variance_out,
                     vcrt_variance_stats* stats) {
    const auto t0 = Clock::now();
    vcrt_variance_params pr;
    const vcrt_result a = vcrt::variance_args(moments, surface, width, height, params,
                                              variance_out, &pr);
    if (a != VCRT_SUCCESS) return a;
    const vcrt_result c = pass_ready(
        !host && (misaligned({moments, surface}, 15u) || misaligned({variance_out}, 3u)),
        g.begun && g.stage.module, g.k_variance_pass);
    if (c != VCRT_SUCCESS) return c;
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, static_cast<size_t>(width) * static_cast<size_t>(height),
                         {in4(moments), in4(surface), out1(variance_out)});
    if (r != VK_SUCCESS) return r;
    // VCRT_VARIANCE_LDS=0: the taps read directly; unset or 1, the measured choice
    // (tools/variance_bench.py, profiles/variance.json): from a staged footprint. Same bits.
    const char* e = std::getenv("VCRT_VARIANCE_LDS");
    const bool lds = !e || std::atoi(e) != 0;
    auto l = vcrt::variance_plan(s.at(0), s.at(1), width, height, pr, lds, s.at(2));
    unsigned long long spatial = 0;
    float ms = 0.f;
    r = run(lds ? g.k_variance_pass_lds : g.k_variance_pass, l, g.d_vr_counters,
            vcrt::kVarianceTallySlots, stats != nullptr, false, &spatial, &ms);
    if (r == VK_SUCCESS && stats) {
        name_stats(stats, lds ? "vcrt_variance_pass_lds" : "vcrt_variance_pass");
        stats->kernel_ms = ms;
        stats->spatial_pixels = spatial;
    }
    return finish(r, s, stats, t0);
}

vcrt_result denoise_variance(bool host, const float* colour, const float* albedo,
                             const float* normal_depth, const float* variance_in, int32_t width,
                             int32_t height, const vcrt_denoise_params* params, float* out,
                             float* out_variance, vcrt_denoise_stats* stats) {
    const auto t0 = Clock::now();
    vcrt_denoise_params pr;
    float k4[4];
    const vcrt_result a = vcrt::denoise_variance_args(colour, albedo, normal_depth, variance_in,
                                                      width, height, params, out, out_variance,
                                                      &pr, k4);
    if (a != VCRT_SUCCESS) return a;
    const vcrt_result c = pass_ready(
        !host && (misaligned({colour, albedo, normal_depth, out}, 15u) ||
                  misaligned({variance_in, out_variance}, 3u)),
        g.begun && g.stage.module, g.k_denoise_var_pass);
    if (c != VCRT_SUCCESS) return c;
    const size_t pixels = static_cast<size_t>(width) * static_cast<size_t>(height);
    Staging s(g.staging, g.stream);
    float* scratch[2];
    VkResult r = s.begin(host, pixels, {in4(colour), in4(albedo), in4(normal_depth),
                                        in1(variance_in), out4(out), out1(out_variance)});
    if (r == VK_SUCCESS) r = atrous_scratch(pr.levels, pixels, scratch);
    if (r != VK_SUCCESS) return r;
    auto plan = vcrt::denoise_variance_plan(s.at(0), s.at(1), s.at(2), s.at(3), width, height, pr,
                                            k4, scratch, denoise_lds_passes(), s.at(4), s.at(5));
    r = run(g.k_denoise_var_pass, g.k_denoise_var_pass_lds, plan, "vcrt_denoise_var_pass", stats);
    return finish(r, s, stats, t0);
}

// The count rule: element-wise, over a grid-stride loop. Its kernel always tallies.
vcrt_result sample_counts(bool host, const float* variance_in, uint32_t elements,
                          const vcrt_sample_count_params* params, uint16_t* counts,
                          vcrt_sample_count_stats* stats) {
    const auto t0 = Clock::now();
    float k;
    const vcrt_result a = vcrt::sample_count_args(variance_in, elements, params, counts, &k);
    if (a != VCRT_SUCCESS) return a;
    // the kernel's 4-byte loads of the variance, 2-byte stores of the counts
    const vcrt_result c = pass_ready(
        !host && (misaligned({variance_in}, 3u) || misaligned({counts}, 1u)),
        g.begun && g.stage.module, g.k_sample_counts_pass);
    if (c != VCRT_SUCCESS) return c;
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, elements, {in1(variance_in), Plane{counts, 2, true}});
    if (r != VK_SUCCESS) return r;
    vcrt::PassLaunch<vcrt::SampleCountParams> l{};
    l.params.variance = s.at(0);
    l.params.counts = s.at<uint16_t>(1);
    l.params.elements = elements;
    l.params.k = k;
    l.params.min_count = params->min_count;
    l.params.max_count = params->max_count;
    l.block = vcrt::kSampleCountThreads;
    l.grid = std::min<uint32_t>(
        (elements + vcrt::kSampleCountThreads - 1u) / vcrt::kSampleCountThreads,
        vcrt::kSampleCountMaxBlocks);
    unsigned long long total = 0;
    float ms = 0.f;
    r = run(g.k_sample_counts_pass, l, g.d_vr_counters, vcrt::kSampleCountTallySlots,
            stats != nullptr, true, &total, &ms);
    if (r == VK_SUCCESS && stats) {
        name_stats(stats, "vcrt_sample_counts_pass");
        stats->kernel_ms = ms;
        stats->total = total;
    }
    return finish(r, s, stats, t0);
}

}  // namespace

extern "C" {

vcrt_result vcrt_denoise(const float* colour, const float* albedo, const float* normal_depth,
                         int32_t width, int32_t height, const vcrt_denoise_params* params,
                         float* out, vcrt_denoise_stats* stats) {
    return denoise(true, colour, albedo, normal_depth, width, height, params, out, stats);
}

vcrt_result vcrt_denoise_device(const float* colour, const float* albedo,
                                const float* normal_depth, int32_t width, int32_t height,
                                const vcrt_denoise_params* params, float* out,
                                vcrt_denoise_stats* stats) {
    return denoise(false, colour, albedo, normal_depth, width, height, params, out, stats);
}

vcrt_result vcrt_reproject(const float* colour, const float* motion, const float* history_colour,
                           const float* history_surface, const float* history_length,
                           int32_t width, int32_t height, const vcrt_reproject_params* params,
                           float* out, float* out_length, vcrt_reproject_stats* stats) {
    return reproject(true, colour, motion, history_colour, history_surface, history_length, width,
                     height, params, out, out_length, stats);
}

vcrt_result vcrt_reproject_device(const float* colour, const float* motion,
                                  const float* history_colour, const float* history_surface,
                                  const float* history_length, int32_t width, int32_t height,
                                  const vcrt_reproject_params* params, float* out,
                                  float* out_length, vcrt_reproject_stats* stats) {
    return reproject(false, colour, motion, history_colour, history_surface, history_length, width,
                     height, params, out, out_length, stats);
}

vcrt_result vcrt_reproject_moments(const float* colour, const float* motion,
                                   const float* history_colour, const float* history_surface,
                                   const float* history_length, const float* albedo,
                                   const float* history_moments, int32_t width, int32_t height,
                                   const vcrt_reproject_moments_params* params, float* out,
                                   float* out_length, float* out_moments,
                                   vcrt_reproject_stats* stats) {
    return reproject_moments(true, colour, motion, history_colour, history_surface, history_length,
                             albedo, history_moments, width, height, params, out, out_length,
                             out_moments, stats);
}

vcrt_result vcrt_reproject_moments_device(const float* colour, const float* motion,
                                          const float* history_colour,
                                          const float* history_surface,
                                          const float* history_length, const float* albedo,
                                          const float* history_moments, int32_t width,
                                          int32_t height,
                                          const vcrt_reproject_moments_params* params, float* out,
                                          float* out_length, float* out_moments,
                                          vcrt_reproject_stats* stats) {
    return reproject_moments(false, colour, motion, history_colour, history_surface,
                             history_length, albedo, history_moments, width, height, params, out,
                             out_length, out_moments, stats);
}

vcrt_result vcrt_variance(const float* moments, const float* surface, int32_t width,
                          int32_t height, const vcrt_variance_params* params, float* variance,
                          vcrt_variance_stats* stats) {
    return ::variance(true, moments, surface, width, height, params, variance, stats);
}

vcrt_result vcrt_variance_device(const float* moments, const float* surface, int32_t width,
                                 int32_t height, const vcrt_variance_params* params,
                                 float* variance, vcrt_variance_stats* stats) {
    return ::variance(false, moments, surface, width, height, params, variance, stats);
}

vcrt_result vcrt_denoise_variance(const float* colour, const float* albedo,
                                  const float* normal_depth, const float* variance, int32_t width,
                                  int32_t height, const vcrt_denoise_params* params, float* out,
                                  float* out_variance, vcrt_denoise_stats* stats) {
    return denoise_variance(true, colour, albedo, normal_depth, variance, width, height, params,
                            out, out_variance, stats);
}

vcrt_result vcrt_denoise_variance_device(const float* colour, const float* albedo,
                                         const float* normal_depth, const float* variance,
                                         int32_t width, int32_t height,
                                         const vcrt_denoise_params* params, float* out,
                                         float* out_variance, vcrt_denoise_stats* stats) {
    return denoise_variance(false, colour, albedo, normal_depth, variance, width, height, params,
                            out, out_variance, stats);
}

vcrt_result vcrt_sample_counts(const float* variance, uint32_t elements,
                               const vcrt_sample_count_params* params, uint16_t* counts,
                               vcrt_sample_count_stats* stats) {
    return sample_counts(true, variance, elements, params, counts, stats);
}

vcrt_result vcrt_sample_counts_device(const float* variance, uint32_t elements,
                                      const vcrt_sample_count_params* params, uint16_t* counts,
                                      vcrt_sample_count_stats* stats) {
    return sample_counts(false, variance, elements, params, counts, stats);
}

}  // extern "C"
