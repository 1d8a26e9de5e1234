// Runs the kernel of csrc/reproject.hip on the host (tests/reproject_host/hip/hip_runtime.h), one
// thread at a time over the launch the library makes (csrc/image_pass_plan.hpp's reproject_plan,
// as image_passes.cpp runs it), on planes read from a file and held in exactly sized heap blocks
// (so a sanitizer build sees any read outside them), and compares the result with
// vcrt_reproject_host word for word.
//   reproject_host_driver PLANES W H alpha max_history depth_tolerance
// PLANES: raw float32 -- colour, motion, history colour, history surface [H][W][4] each, then
// history length [H][W]. Prints "bad <words that differ> pixels <W H> accepted <tally> want
// <pixels the host blended>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "image_pass_plan.hpp"
#include "reproject.hip"
#include "vcrt.h"

dim3e blockIdx{0, 0, 0};
dim3e threadIdx{0, 0, 0};

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    vcrt_reproject_params pr;
    vcrt_default_reproject_params(&pr);
    pr.alpha = std::strtof(argv[4], nullptr);
    pr.max_history = std::strtof(argv[5], nullptr);
    pr.depth_tolerance = std::strtof(argv[6], nullptr);
    const size_t pixels = static_cast<size_t>(w) * h;
    const size_t sizes[5] = {4 * pixels, 4 * pixels, 4 * pixels, 4 * pixels, pixels};
    std::unique_ptr<float[]> in[5];
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    for (int k = 0; k < 5; k++) {
        in[k].reset(new float[sizes[k]]);
        if (std::fread(in[k].get(), sizeof(float), sizes[k], f) != sizes[k]) return 3;
    }
    std::fclose(f);
    std::unique_ptr<float[]> want(new float[4 * pixels]), want_len(new float[pixels]);
    std::unique_ptr<float[]> got(new float[4 * pixels]), got_len(new float[pixels]);
    for (size_t i = 0; i < 4 * pixels; i++) got[i] = -1.0f;
    for (size_t i = 0; i < pixels; i++) got_len[i] = -1.0f;
    if (vcrt_reproject_host(in[0].get(), in[1].get(), in[2].get(), in[3].get(), in[4].get(), w, h,
                            &pr, want.get(), want_len.get()) != VCRT_SUCCESS)
        return 4;
    std::unique_ptr<unsigned long long[]> tallies(
        new unsigned long long[8 * vcrt::kReprojectTallySlots]());

    vcrt::PassLaunch<vcrt::ReprojectParams> launch =
        vcrt::reproject_plan(in[0].get(), in[1].get(), in[2].get(), in[3].get(), in[4].get(), w, h,
                             pr, got.get(), got_len.get());
    launch.params.tallies = tallies.get();
    for (uint32_t b = 0; b < launch.grid; b++)
        for (uint32_t t = 0; t < launch.block; t++) {
            blockIdx.x = b;
            threadIdx.x = t;
            vcrt_reproject_pass(launch.params);
        }
    size_t bad = 0, blended = 0;
    unsigned long long accepted = 0;
    for (size_t i = 0; i < 4 * pixels; i++) bad += std::memcmp(&got[i], &want[i], 4) != 0;
    for (size_t i = 0; i < pixels; i++) {
        bad += std::memcmp(&got_len[i], &want_len[i], 4) != 0;
        blended += want_len[i] != 1.0f || std::memcmp(&want[4 * i], &in[0][4 * i], 12) != 0;
    }
    for (uint32_t s = 0; s < vcrt::kReprojectTallySlots; s++) accepted += tallies[8 * s];
    std::printf("bad %zu pixels %d accepted %llu blended %zu\n", bad, w * h, accepted, blended);
    return 0;
}
