// Runs the kernels of csrc/variance.hip on the host (tests/variance_host/hip/hip_runtime.h) over
// the launches capi.cpp makes, on planes read from a file and held in exactly sized heap blocks (so
// a sanitizer build sees any read outside them), and compares the results with the _host functions
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

template <class Kernel, class Params>
void run_rows(Kernel kernel, const Params& p, uint32_t blocks, uint32_t threads) {
    for (uint32_t b = 0; b < blocks; b++)
        for (uint32_t t = 0; t < threads; t++) {
            blockIdx.x = b;
            threadIdx.x = t;
            kernel(p);
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
        vcrt::ReprojectMomentsParams p{};
        p.colour = in[kColour].get();
        p.motion = in[kMotion].get();
        p.history_colour = in[kHcol].get();
        p.history_surface = in[kHsurf].get();
        p.history_length = in[kHlen].get();
        p.albedo = albedo;
        p.history_moments = in[kHmom].get();
        p.out = got.get();
        p.out_length = got_len.get();
        p.out_moments = got_mom.get();
        p.width = static_cast<uint32_t>(w);
        p.height = static_cast<uint32_t>(h);
        p.alpha = pr.alpha;
        p.max_history = pr.max_history;
        p.depth_tolerance = pr.depth_tolerance;
        p.alpha_moments = pr.alpha_moments;
        p.tiles_x = (p.width + vcrt::kMomentsRowW - 1u) / vcrt::kMomentsRowW;
        p.tallies = tallies.get();
        const uint32_t tiles_y = (p.height + vcrt::kMomentsRowH - 1u) / vcrt::kMomentsRowH;
        run_rows(vcrt_reproject_moments_pass, p, p.tiles_x * tiles_y, vcrt::kMomentsThreads);
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
        vcrt::VarianceParams p{};
        p.moments = in[kMoments].get();
        p.surface = in[kSurface].get();
        p.variance = got.get();
        p.width = static_cast<uint32_t>(w);
        p.height = static_cast<uint32_t>(h);
        p.min_history = pr.min_history;
        p.alpha = pr.alpha;
        p.tiles_x = (p.width + vcrt::kVarianceRowW - 1u) / vcrt::kVarianceRowW;
        p.tallies = tallies.get();
        const uint32_t tiles_y = (p.height + vcrt::kVarianceRowH - 1u) / vcrt::kVarianceRowH;
        if (lds) {
            lds_run = 1;
            p.tiles_x = (p.width + vcrt::kVarianceTileW - 1u) / vcrt::kVarianceTileW;
            const uint32_t rows = (p.height + vcrt::kVarianceTileH - 1u) / vcrt::kVarianceTileH;
            for (uint32_t b = 0; b < p.tiles_x * rows; b++) {
                blockIdx.x = b;
                for (float4& v : l_var_planes) v = make_float4(-4.f, -4.f, -4.f, -4.f);
                std::vector<std::thread> group;
                for (uint32_t t = 0; t < vcrt::kVarianceThreads; t++)
                    group.emplace_back([t, p] {
                        threadIdx.x = t;
                        vcrt_variance_pass_lds(p);
                    });
                for (std::thread& t : group) t.join();
            }
        } else {
            run_rows(vcrt_variance_pass, p, p.tiles_x * tiles_y, vcrt::kVarianceThreads);
        }
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
        Plane scratch[2];
        float k4[4];
        if (vcrt_denoise_scales(&pr, k4) != VCRT_SUCCESS) return 4;
        if (vcrt_denoise_variance_host(colour, albedo, guides, in[kVar].get(), w, h, &pr,
                                       want.get(), want_var.get()) != VCRT_SUCCESS)
            return 4;
        const bool demod = pr.demodulate != 0 && albedo;
        uint32_t terms = 0;
        if (guides && k4[0] != 0.0f) terms |= vcrt::kDenoiseNormal;
        if (guides && k4[1] != 0.0f) terms |= vcrt::kDenoiseDepth;
        if (albedo && k4[2] != 0.0f) terms |= vcrt::kDenoiseAlbedo;
        if (pr.sigma_colour != 0.0f) terms |= vcrt::kDenoiseColour;
        const float* src = colour;
        for (int l = 0; l < pr.levels; l++) {
            const bool last = l == pr.levels - 1;
            if (!last) scratch[l & 1] = filled(4 * pixels, -3.f);
            vcrt::DenoiseVarParams p{};
            p.in = src;
            p.colour = colour;
            p.albedo = albedo;
            p.normal_depth = guides;
            p.variance = in[kVar].get();
            p.out = last ? got.get() : scratch[l & 1].get();
            p.out_variance = got_var.get();
            p.width = static_cast<uint32_t>(w);
            p.height = static_cast<uint32_t>(h);
            p.step = 1u << l;
            p.flags = terms | (l == 0 ? vcrt::kDenoiseVarIn : 0u) |
                      (demod && l == 0 ? vcrt::kDenoiseDemodIn : 0u) |
                      (demod && last ? vcrt::kDenoiseModOut : 0u) |
                      (last ? vcrt::kDenoiseLast : 0u);
            p.k_normal = k4[0];
            p.k_depth = k4[1];
            p.k_albedo = k4[2];
            p.sc2 = pr.sigma_colour * pr.sigma_colour;
            if (l < lds_passes && p.step <= vcrt::kDenoiseLdsMaxStep) {
                lds_run++;
                p.tiles_x = (p.width + vcrt::kDenoiseTileW - 1u) / vcrt::kDenoiseTileW;
                const uint32_t tiles_y =
                    (p.height + vcrt::kDenoiseTileH - 1u) / vcrt::kDenoiseTileH;
                for (uint32_t b = 0; b < p.tiles_x * tiles_y; b++) {
                    blockIdx.x = b;
                    for (float4& v : l_var_planes) v = make_float4(-4.f, -4.f, -4.f, -4.f);
                    std::vector<std::thread> group;
                    for (uint32_t t = 0; t < vcrt::kDenoiseThreads; t++)
                        group.emplace_back([t, p] {
                            threadIdx.x = t;
                            vcrt_denoise_var_pass_lds(p);
                        });
                    for (std::thread& t : group) t.join();
                }
            } else {
                p.tiles_x = (p.width + vcrt::kDenoiseRowW - 1u) / vcrt::kDenoiseRowW;
                const uint32_t tiles_y = (p.height + vcrt::kDenoiseRowH - 1u) / vcrt::kDenoiseRowH;
                run_rows(vcrt_denoise_var_pass, p, p.tiles_x * tiles_y, vcrt::kDenoiseThreads);
            }
            src = p.out;
        }
        bad = differing(got, want, 4 * pixels) + differing(got_var, want_var, pixels);
    } else {
        return 2;
    }
    std::printf("bad %zu pixels %d tally %llu lds %d\n", bad, w * h, tally, lds_run);
    return 0;
}
