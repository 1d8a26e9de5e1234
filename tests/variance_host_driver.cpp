// Runs the kernels of csrc/variance.hip on the host (tests/variance_host/hip/hip_runtime.h) over
// the launches the library makes (csrc/image_pass_plan.hpp's plans, as image_passes.cpp runs
// them), on planes read from a file and held in exactly sized heap blocks (so a sanitizer build
// sees any read outside them), and compares the results with the _host functions
// of csrc/variance.cpp word for word. The direct kernels run one thread at a time; the LDS kernel's
// workgroup runs as 256 threads around a barrier.
//   variance_host_driver PLANES W H moments  alpha max_history depth_tolerance alpha_moments albedo(0|1)
//   variance_host_driver PLANES W H variance min_history alpha lds(0|1)
//   variance_host_driver PLANES W H denoise  levels sn sd sa sc demodulate lds_passes albedo(0|1) guides(0|1)
// PLANES: raw float32 -- colour, motion, history colour, history surface [H][W][4], history length
// [H][W], albedo, normal_depth, history moments, moments, surface [H][W][4], variance [H][W].
// Prints "bad <words that differ> pixels <W H> tally <the kernel's tally> lds <LDS passes run>".
#include <algorithm>
#include <barrier>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "image_pass_plan.hpp"
#include "variance.hip"
#include "vcrt.h"

dim3e blockIdx{0, 0, 0};
thread_local dim3e threadIdx{0, 0, 0};
float4 l_var_planes[3 * (32 + 8) * (8 + 8)];
static std::barrier<> g_barrier(vcrt::kDenoiseThreads);
void __syncthreads() { g_barrier.arrive_and_wait(); }

namespace {

using Plane = std::unique_ptr<float[]>;

Plane filled(size_t words, float v) {
    Plane p(new float[words]);
    std::fill(p.get(), p.get() + words, v);
    return p;
}

size_t differing(const Plane& a, const Plane& b, size_t words) {
    size_t bad = 0;
    for (size_t i = 0; i < words; i++) bad += std::memcmp(&a[i], &b[i], 4) != 0;
    return bad;
}

// a direct kernel's launch, one thread at a time
template <class Kernel, class Params>
void run_rows(Kernel kernel, const vcrt::PassLaunch<Params>& l) {
    for (uint32_t b = 0; b < l.grid; b++)
        for (uint32_t t = 0; t < l.block; t++) {
            blockIdx.x = b;
            threadIdx.x = t;
            kernel(l.params);
        }
}

// an LDS kernel's launch: each workgroup as its threads around the barrier, over a stand-in for
// the dynamic LDS that the launch's byte count must fit
template <class Kernel, class Params>
void run_group(Kernel kernel, const vcrt::PassLaunch<Params>& l) {
    if (l.lds_bytes > sizeof(l_var_planes) || l.block != vcrt::kDenoiseThreads) std::exit(5);
    const Params p = l.params;
    for (uint32_t b = 0; b < l.grid; b++) {
        blockIdx.x = b;
        for (float4& v : l_var_planes) v = make_float4(-4.f, -4.f, -4.f, -4.f);
        std::vector<std::thread> group;
        for (uint32_t t = 0; t < l.block; t++)
            group.emplace_back([t, p, kernel] {
                threadIdx.x = t;
                kernel(p);
            });
        for (std::thread& t : group) t.join();
    }
}

enum { kColour, kMotion, kHcol, kHsurf, kHlen, kAlbedo, kNd, kHmom, kMoments, kSurface, kVar, kPlanes };

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    const std::string call = argv[4];
    const size_t pixels = static_cast<size_t>(w) * h;
    Plane in[kPlanes];
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    for (int k = 0; k < kPlanes; k++) {
        const size_t words = (k == kHlen || k == kVar) ? pixels : 4 * pixels;
        in[k].reset(new float[words]);
        if (std::fread(in[k].get(), sizeof(float), words, f) != words) return 3;
    }
    std::fclose(f);
    size_t bad = 0;
    unsigned long long tally = 0;
    int lds_run = 0;

    if (call == "moments") {
        if (argc != 10) return 2;
        vcrt_reproject_moments_params pr;
        vcrt_default_reproject_moments_params(&pr);
        pr.alpha = std::strtof(argv[5], nullptr);
        pr.max_history = std::strtof(argv[6], nullptr);
        pr.depth_tolerance = std::strtof(argv[7], nullptr);
        pr.alpha_moments = std::strtof(argv[8], nullptr);
        const float* albedo = std::atoi(argv[9]) ? in[kAlbedo].get() : nullptr;
        Plane want = filled(4 * pixels, -1.f), want_len = filled(pixels, -1.f),
              want_mom = filled(4 * pixels, -1.f);
        Plane got = filled(4 * pixels, -2.f), got_len = filled(pixels, -2.f),
              got_mom = filled(4 * pixels, -2.f);
        if (vcrt_reproject_moments_host(in[kColour].get(), in[kMotion].get(), in[kHcol].get(),
                                        in[kHsurf].get(), in[kHlen].get(), albedo,
                                        in[kHmom].get(), w, h, &pr, want.get(), want_len.get(),
                                        want_mom.get()) != VCRT_SUCCESS)
            return 4;
        std::unique_ptr<unsigned long long[]> tallies(
            new unsigned long long[8 * vcrt::kMomentsTallySlots]());
        vcrt::PassLaunch<vcrt::ReprojectMomentsParams> launch = vcrt::reproject_moments_plan(
            in[kColour].get(), in[kMotion].get(), in[kHcol].get(), in[kHsurf].get(),
            in[kHlen].get(), albedo, in[kHmom].get(), w, h, pr, got.get(), got_len.get(),
            got_mom.get());
        launch.params.tallies = tallies.get();
        run_rows(vcrt_reproject_moments_pass, launch);
        bad = differing(got, want, 4 * pixels) + differing(got_len, want_len, pixels) +
              differing(got_mom, want_mom, 4 * pixels);
        for (uint32_t s = 0; s < vcrt::kMomentsTallySlots; s++) tally += tallies[8 * s];
    } else if (call == "variance") {
        if (argc != 8) return 2;
        const bool lds = std::atoi(argv[7]) != 0;
        vcrt_variance_params pr;
        vcrt_default_variance_params(&pr);
        pr.min_history = std::strtof(argv[5], nullptr);
        pr.alpha = std::strtof(argv[6], nullptr);
        Plane want = filled(pixels, -1.f), got = filled(pixels, -2.f);
        if (vcrt_variance_host(in[kMoments].get(), in[kSurface].get(), w, h, &pr, want.get()) !=
            VCRT_SUCCESS)
            return 4;
        std::unique_ptr<unsigned long long[]> tallies(
            new unsigned long long[8 * vcrt::kVarianceTallySlots]());
        vcrt::PassLaunch<vcrt::VarianceParams> launch = vcrt::variance_plan(
            in[kMoments].get(), in[kSurface].get(), w, h, pr, lds, got.get());
        launch.params.tallies = tallies.get();
        lds_run = launch.lds;
        if (launch.lds)
            run_group(vcrt_variance_pass_lds, launch);
        else
            run_rows(vcrt_variance_pass, launch);
        bad = differing(got, want, pixels);
        for (uint32_t s = 0; s < vcrt::kVarianceTallySlots; s++) tally += tallies[8 * s];
    } else if (call == "denoise") {
        if (argc != 14) return 2;
        vcrt_denoise_params pr;
        vcrt_default_denoise_variance_params(&pr);
        pr.levels = std::atoi(argv[5]);
        pr.sigma_normal = std::strtof(argv[6], nullptr);
        pr.sigma_depth = std::strtof(argv[7], nullptr);
        pr.sigma_albedo = std::strtof(argv[8], nullptr);
        pr.sigma_colour = std::strtof(argv[9], nullptr);
        pr.demodulate = std::atoi(argv[10]);
        const int lds_passes = std::min(std::atoi(argv[11]), pr.levels);
        const float* colour = in[kColour].get();
        const float* albedo = std::atoi(argv[12]) ? in[kAlbedo].get() : nullptr;
        const float* guides = std::atoi(argv[13]) ? in[kNd].get() : nullptr;
        Plane want = filled(4 * pixels, -1.f), want_var = filled(pixels, -1.f);
        Plane got = filled(4 * pixels, -2.f), got_var = filled(pixels, -2.f);
        Plane scratch[2] = {filled(4 * pixels, -3.f), filled(4 * pixels, -3.f)};
        float k4[4];
        if (vcrt_denoise_scales(&pr, k4) != VCRT_SUCCESS) return 4;
        if (vcrt_denoise_variance_host(colour, albedo, guides, in[kVar].get(), w, h, &pr,
                                       want.get(), want_var.get()) != VCRT_SUCCESS)
            return 4;
        float* const planes[2] = {scratch[0].get(), scratch[1].get()};
        const vcrt::AtrousPlan<vcrt::DenoiseVarParams> plan = vcrt::denoise_variance_plan(
            colour, albedo, guides, in[kVar].get(), w, h, pr, k4, planes, lds_passes, got.get(),
            got_var.get());
        lds_run = plan.lds_passes;
        for (int l = 0; l < plan.passes; l++) {
            const vcrt::PassLaunch<vcrt::DenoiseVarParams>& launch = plan.pass[l];
            float* out = launch.params.out;
            if (out != got.get()) std::fill(out, out + 4 * pixels, -3.f);
            if (launch.lds)
                run_group(vcrt_denoise_var_pass_lds, launch);
            else
                run_rows(vcrt_denoise_var_pass, launch);
        }
        bad = differing(got, want, 4 * pixels) + differing(got_var, want_var, pixels);
    } else {
        return 2;
    }
    std::printf("bad %zu pixels %d tally %llu lds %d\n", bad, w * h, tally, lds_run);
    return 0;
}
