// frame_rays_check -- vcrt_frame_rays (host only, no GPU) under the host sanitizers: a program
// of its own that calls it for the cases of tests/test_features_cpu.py (44 x 20, every pixel,
// pinhole and lens radius 0.1, first 0 and 7, n = 5, two cameras) into exactly-sized heap
// buffers, checks what must hold without a reference (finite rays; the pinhole's origins are the
// camera centre; the argument errors), does the same for vcrt_ambient_dirs (the last 4096
// directions below 2^22, unit length) and exits 0. Build it with the library's host sources and
// -fsanitize=address,undefined, from the repository root (ROCM=/opt/rocm):
//   cd vulkancomputeraytracing_amd && g++ -O1 -g -std=c++17 -fsanitize=address,undefined \
//     -fno-sanitize-recover=undefined -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I../include \
//     -Icsrc -I$ROCM/include ../tools/frame_rays_check.cpp csrc/capi.cpp csrc/ray_passes.cpp \
//     csrc/image_passes.cpp csrc/denoise.cpp csrc/reproject.cpp csrc/variance.cpp csrc/cluster.cpp \
//     csrc/primary.cpp csrc/shader.cpp csrc/scene.cpp lib/obj/embed_code_object.o \
//     -L$ROCM/lib -Wl,-rpath,$ROCM/lib -lamdhip64 -lrccl -ldl -pthread -o frame_rays_check
#include <cmath>
#include <cstdio>
#include <vector>

#include "vcrt.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "frame_rays_check: %s\n", what);
        failures++;
    }
}

}  // namespace

int main() {
    const int w = 44, h = 20;
    const uint32_t n = 5;
    std::vector<int32_t> xy;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            xy.push_back(x);
            xy.push_back(y);
        }
    const vcrt_camera other = {{-6.5f, 3.25f, 9.0f}, {0.5f, 0.75f, -1.0f}, {0.1f, 1.0f, 0.05f}, 33.0f};
    for (int cam = 0; cam < 2; cam++)
        for (float radius : {0.0f, 0.1f})
            for (uint32_t first : {0u, 7u}) {
                vcrt_render_desc d;
                vcrt_default_desc(&d);
                d.width = w;
                d.height = h;
                d.lens_radius = radius;
                if (cam) d.camera = other;
                std::vector<float> o(static_cast<size_t>(w) * h * n * 3), dir(o.size());
                const int32_t r = vcrt_frame_rays(&d, xy.data(), w * h, first, n, o.data(), dir.data());
                expect(r == w * h, "the pixel count comes back");
                bool finite = true, centre = true;
                for (size_t i = 0; i < o.size(); i++) {
                    finite = finite && std::isfinite(o[i]) && std::isfinite(dir[i]);
                    centre = centre && o[i] == d.camera.lookfrom[i % 3];
                }
                expect(finite, "finite rays");
                expect(radius > 0.0f ? !centre : centre, "the pinhole starts at the camera centre");
            }
    vcrt_render_desc d;
    vcrt_default_desc(&d);
    d.width = w;
    d.height = h;
    float one[3];
    const int32_t at[2] = {w - 1, h - 1}, outside[2] = {w, 0};
    expect(vcrt_frame_rays(&d, at, 1, (1u << 19) - 1, 1, one, one) == 1, "the last index");
    expect(vcrt_frame_rays(&d, at, 1, (1u << 19) - 1, 2, one, one) ==
               VCRT_ERROR_FORMAT_NOT_SUPPORTED, "past the last index");
    expect(vcrt_frame_rays(&d, at, 1, 0xffffffffu, 2, one, one) == VCRT_ERROR_FORMAT_NOT_SUPPORTED,
           "no 32-bit wrap");
    expect(vcrt_frame_rays(&d, at, 1, 0, 0, one, one) == VCRT_ERROR_FORMAT_NOT_SUPPORTED, "n = 0");
    expect(vcrt_frame_rays(&d, outside, 1, 0, 1, one, one) == VCRT_ERROR_INITIALIZATION_FAILED,
           "a pixel outside the frame");
    expect(vcrt_frame_rays(&d, nullptr, 1, 0, 1, one, one) == VCRT_ERROR_INITIALIZATION_FAILED,
           "NULL pixels");
    expect(vcrt_frame_rays(&d, at, 0, 0, 1, nullptr, nullptr) == 0, "no pixels");
    // the feature call's argument errors need no renderer either
    expect(vcrt_draw_features(0, 4, one, nullptr, nullptr, nullptr) ==
               VCRT_ERROR_INITIALIZATION_FAILED, "before vcrt_begin");
    expect(vcrt_draw_features(0, 0, one, nullptr, nullptr, nullptr) ==
               VCRT_ERROR_FORMAT_NOT_SUPPORTED, "n = 0 samples");
    // the ambient visibility buffer's host-only table, into an exactly-sized heap buffer, and
    // its call's argument errors
    {
        const uint32_t first = (1u << 22) - 4096, count = 4096;
        std::vector<float> u(3 * static_cast<size_t>(count));
        expect(vcrt_ambient_dirs(first, count, u.data()) == static_cast<int32_t>(count),
               "the direction count comes back");
        bool unit = true;
        for (uint32_t k = 0; k < count; k++) {
            const double l2 = static_cast<double>(u[3 * k]) * u[3 * k] +
                              static_cast<double>(u[3 * k + 1]) * u[3 * k + 1] +
                              static_cast<double>(u[3 * k + 2]) * u[3 * k + 2];
            unit = unit && std::fabs(l2 - 1.0) <= 1e-6;
        }
        expect(unit, "unit directions");
        expect(vcrt_ambient_dirs(first + 1, count, u.data()) == VCRT_ERROR_FORMAT_NOT_SUPPORTED,
               "past the last direction");
        expect(vcrt_ambient_dirs(0, 1, nullptr) == VCRT_ERROR_INITIALIZATION_FAILED, "NULL table");
        expect(vcrt_draw_occlusion(0, 4, 8, 1e5f, one, nullptr) == VCRT_ERROR_INITIALIZATION_FAILED,
               "before vcrt_begin");
        expect(vcrt_draw_occlusion(0, 17, 256, 1e5f, one, nullptr) ==
                   VCRT_ERROR_FORMAT_NOT_SUPPORTED, "n m > 4096");
    }
    if (failures == 0) std::puts("frame_rays_check: ok");
    return failures == 0 ? 0 : 1;
}
