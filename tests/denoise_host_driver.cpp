// Runs the kernels of csrc/denoise.hip on the host (tests/denoise_host/hip/hip_runtime.h) over
// seeded planes and compares the result with vcrt_denoise_host word for word. The launches are
// the library's own: csrc/image_pass_plan.hpp's denoise_plan, as image_passes.cpp runs it. The
// direct kernel runs one thread at a time; the LDS kernel's workgroup runs as 256 threads around a
// barrier.
//   denoise_host_driver W H levels sn sd sa sc demodulate lds_passes albedo(0|1) guides(0|1)
// prints "bad <words that differ> pixels <W H> lds <passes run by the LDS kernel>".
#include <algorithm>
#include <barrier>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "denoise.hip"
#include "image_pass_plan.hpp"
#include "vcrt.h"

dim3e blockIdx{0, 0, 0};
thread_local dim3e threadIdx{0, 0, 0};
float4 l_planes[3 * (32 + 8) * (8 + 8)];
static std::barrier<> g_barrier(vcrt::kDenoiseThreads);
void __syncthreads() { g_barrier.arrive_and_wait(); }

namespace {

uint32_t g_seed = 12345u;
float unit() {  // [0, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return static_cast<float>(g_seed >> 8) * 0x1p-24f;
}

// 5 x 5 blocks of constant values plus a little noise: weights all over [0, 1]
std::vector<float> plane(int w, int h, float lo, float hi, float noise) {
    const int bx = (w + 4) / 5, by = (h + 4) / 5;
    std::vector<float> b(static_cast<size_t>(bx) * by * 4), p(static_cast<size_t>(w) * h * 4);
    for (float& v : b) v = lo + (hi - lo) * unit();
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 4; c++)
                p[(static_cast<size_t>(y) * w + x) * 4 + c] =
                    b[(static_cast<size_t>(y / 5) * bx + x / 5) * 4 + c] + noise * (unit() - 0.5f);
    return p;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 12) return 2;
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
    vcrt_denoise_params pr;
    vcrt_default_denoise_params(&pr);
    pr.levels = std::atoi(argv[3]);
    pr.sigma_normal = std::strtof(argv[4], nullptr);
    pr.sigma_depth = std::strtof(argv[5], nullptr);
    pr.sigma_albedo = std::strtof(argv[6], nullptr);
    pr.sigma_colour = std::strtof(argv[7], nullptr);
    pr.demodulate = std::atoi(argv[8]);
    const int lds_passes = std::min(std::atoi(argv[9]), pr.levels);
    std::vector<float> colour = plane(w, h, 0.1f, 1.5f, 0.3f), alb = plane(w, h, 0.0f, 1.0f, 0.05f),
                       nd = plane(w, h, -1.0f, 1.0f, 0.1f);
    for (size_t i = 0; i < alb.size(); i += 7) alb[i] = 0.0f;  // below the demodulation's floor
    const float* albedo = std::atoi(argv[10]) ? alb.data() : nullptr;
    const float* guides = std::atoi(argv[11]) ? nd.data() : nullptr;
    const size_t words = static_cast<size_t>(w) * h * 4;
    std::vector<float> want(words), got(words, -1.0f), scratch[2];
    float k4[4];
    if (vcrt_denoise_scales(&pr, k4) != VCRT_SUCCESS) return 3;
    if (vcrt_denoise_host(colour.data(), albedo, guides, w, h, &pr, want.data()) != VCRT_SUCCESS)
        return 3;

    for (std::vector<float>& s : scratch) s.resize(words);
    float* const planes[2] = {scratch[0].data(), scratch[1].data()};
    const vcrt::AtrousPlan<vcrt::DenoiseParams> plan = vcrt::denoise_plan(
        colour.data(), albedo, guides, w, h, pr, k4, planes, lds_passes, got.data());
    for (int l = 0; l < plan.passes; l++) {
        const vcrt::PassLaunch<vcrt::DenoiseParams>& launch = plan.pass[l];
        const vcrt::DenoiseParams p = launch.params;
        if (p.out != got.data()) std::fill(p.out, p.out + words, -2.0f);
        if (launch.lds) {
            if (launch.lds_bytes > sizeof(l_planes)) return 5;
            for (uint32_t b = 0; b < launch.grid; b++) {
                blockIdx.x = b;
                for (float4& v : l_planes) v = make_float4(-3.f, -3.f, -3.f, -3.f);
                std::vector<std::thread> group;
                for (uint32_t t = 0; t < launch.block; t++)
                    group.emplace_back([t, p] {
                        threadIdx.x = t;
                        vcrt_denoise_pass_lds(p);
                    });
                for (std::thread& t : group) t.join();
            }
        } else {
            for (uint32_t b = 0; b < launch.grid; b++)
                for (uint32_t t = 0; t < launch.block; t++) {
                    blockIdx.x = b;
                    threadIdx.x = t;
                    vcrt_denoise_pass(p);
                }
        }
    }
    size_t bad = 0;
    for (size_t i = 0; i < words; i++) bad += std::memcmp(&got[i], &want[i], 4) != 0;
    std::printf("bad %zu pixels %d lds %d\n", bad, w * h, plan.lds_passes);
    return 0;
}
