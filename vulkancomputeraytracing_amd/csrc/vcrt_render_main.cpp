// vcrt_render -- headless replacement of the reference's main()
// (VulkanComputeRayTracing.cpp:17-42): Begin -> DrawNextFrame x N -> End, then optionally writes
// the frame as PFM (linear rgba32f, as the compute image holds it) or PPM (sRGB8 encoded on the
// GPU, as the B8G8R8A8_SRGB swapchain shows it: Frontend.cpp:43). --features PREFIX adds the
// frame's guide buffers (vcrt_draw_features) as PREFIX_albedo.ppm and PREFIX_normal.ppm, --ao
// PREFIX its ambient visibility buffer (vcrt_draw_occlusion) as PREFIX_ao.ppm, sRGB8 as a frame.
// --denoise FILE writes the last frame put through the denoiser (vcrt_denoise over the framebuffer
// and the guide buffers of --feature-samples samples), PFM or PPM by FILE's suffix as --out.
// --temporal FILE accumulates the frames of an --orbit: every frame after the first is put through
// vcrt_reproject with the previous output as its history and the map of vcrt_draw_motion for the
// previous frame's camera; FILE receives the last accumulated frame, and --denoise then filters it.
// --variance (a flag; needs --temporal and --denoise) runs the variance-guided chain instead: every
// frame, the first included, goes through vcrt_reproject_moments with the frame's albedo, and the
// denoiser is vcrt_denoise_variance steered by vcrt_variance of the last frame's moments.
// --adaptive N0,TARGET,MAX with --adaptive-out FILE runs one adaptive-sampling loop on the last
// frame's camera (vcrt_draw_samples, vcrt_sample_counts) and writes its mean plane: two uniform
// rounds of N0 samples into one sums plane, the per-sample luminance variance estimated from the
// means after the first and after both rounds, then one round of the counts that variance asks for.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "Renderer.hpp"

namespace {

int usage() {
    std::fprintf(stderr,
                 "usage: vcrt_render [--width W] [--height H] [--spp N] [--depth D] "
                 "[--scene final|three|red|stress4096] [--frames F] [--progressive 0|1] [--device I] "
                 "[--lens-radius R] [--orbit DEG] [--out file.ppm|file.pfm] "
                 "[--features PREFIX] [--feature-samples N] [--ao PREFIX] [--ao-rays M] "
                 "[--denoise file.ppm|file.pfm] [--denoise-levels L] "
                 "[--temporal file.ppm|file.pfm] [--variance] "
                 "[--adaptive N0,TARGET,MAX --adaptive-out file.ppm|file.pfm]\n"
                 "  --adaptive: per pixel, two uniform rounds of N0 samples (sample indices 0 .. "
                 "2 N0 - 1), then up to MAX more.\n"
                 "    Variance estimator: with Y1 the luminance of the mean after round one and "
                 "Y12 after both,\n"
                 "    d = Y12 - Y1 estimates the deviation of the 2 N0-sample mean, so a sample's "
                 "variance is about\n"
                 "    v = d * d * (2 N0); the third round takes clamp(ceil(v / TARGET^2), 0, MAX) "
                 "samples per pixel:\n"
                 "    the count at which the mean's standard deviation reaches TARGET.\n");
    return 2;
}

// The frame as PFM (rgba, bottom row first) or PPM (rgba8, top row first), three channels.
bool write_image(const std::string& path, int width, int height, bool pfm,
                 const std::vector<float>& rgba, const std::vector<uint8_t>& rgba8) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, pfm ? "PF\n%d %d\n-1.0\n" : "P6\n%d %d\n255\n", width, height);
    for (int y = pfm ? height - 1 : 0; pfm ? y >= 0 : y < height; y += pfm ? -1 : 1) {
        for (int x = 0; x < width; x++) {
            const size_t i = static_cast<size_t>(y) * width + x;
            if (pfm) std::fwrite(&rgba[4 * i], sizeof(float), 3, f);
            else std::fwrite(&rgba8[4 * i], 1, 3, f);
        }
    }
    return std::fclose(f) == 0;
}

inline float lum(const float* c) {  // vcrt.h's lum, one rounded operation per step
    float y = 0.2126f * c[0] + 0.7152f * c[1];
    y = y + 0.0722f * c[2];
    return y;
}

uint8_t unit_byte(float v) {  // clamp to [0, 1] (NaN: 0), round to nearest of 255 v
    return static_cast<uint8_t>((v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f) * 255.0f + 0.5f);
}

}  // namespace

int main(int argc, char** argv) {
    vcrt_render_desc desc;
    vcrt_default_desc(&desc);
    int scene = VCRT_SCENE_FINAL, frames = 1;
    double orbit = 0.0;  // degrees about the world y axis through lookat, per frame
    std::string out, features, ao, denoise, temporal, adaptive_out;
    int adaptive_n0 = 0, adaptive_max = 0;  // --adaptive N0,TARGET,MAX (n0 0: off)
    float adaptive_target = 0.0f;
    int denoise_levels = 0;   // 0: vcrt_default_denoise_params'
    int feature_samples = 0;  // 0: the description's spp
    int ao_rays = 8;          // secondary rays per sample that hits
    bool configured = false;  // any option that changes the description or the scene
    bool variance = false;    // --variance: the variance-guided chain
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--variance") {  // the one option without a value
            variance = true;
            continue;
        }
        if (i + 1 >= argc) return usage();
        const char* v = argv[++i];
        configured = configured || (a != "--out" && a != "--frames" && a != "--features" &&
                                    a != "--feature-samples" && a != "--ao" && a != "--ao-rays" &&
                                    a != "--denoise" && a != "--denoise-levels" &&
                                    a != "--temporal" && a != "--adaptive" &&
                                    a != "--adaptive-out");
        if (a == "--width") desc.width = std::atoi(v);
        else if (a == "--height") desc.height = std::atoi(v);
        else if (a == "--spp") desc.samples_per_pixel = std::atoi(v);
        else if (a == "--depth") desc.max_depth = std::atoi(v);
        else if (a == "--frames") frames = std::atoi(v);
        else if (a == "--device") desc.device = std::atoi(v);
        else if (a == "--progressive") desc.progressive = std::atoi(v);
        else if (a == "--lens-radius") desc.lens_radius = std::strtof(v, nullptr);  // thin lens
        else if (a == "--orbit") orbit = std::strtod(v, nullptr);
        else if (a == "--out") out = v;
        else if (a == "--features") features = v;
        else if (a == "--feature-samples") feature_samples = std::atoi(v);
        else if (a == "--ao") ao = v;
        else if (a == "--ao-rays") ao_rays = std::atoi(v);
        else if (a == "--denoise") denoise = v;
        else if (a == "--denoise-levels") denoise_levels = std::atoi(v);
        else if (a == "--temporal") temporal = v;
        else if (a == "--adaptive-out") adaptive_out = v;
        else if (a == "--adaptive") {
            if (std::sscanf(v, "%d,%f,%d", &adaptive_n0, &adaptive_target, &adaptive_max) != 3 ||
                adaptive_n0 < 1 || adaptive_n0 > 256 || adaptive_max < 1 || adaptive_max > 256 ||
                !(adaptive_target > 0.0f))
                return usage();
        }
        else if (a == "--scene") {
            const std::string s = v;
            scene = s == "final" ? VCRT_SCENE_FINAL : s == "three" ? VCRT_SCENE_THREE
                  : s == "red" ? VCRT_SCENE_RED : s == "stress4096" ? VCRT_SCENE_STRESS4096 : -1;
            if (scene < 0) return usage();
        } else return usage();
    }
    if (variance && (temporal.empty() || denoise.empty())) {
        std::fprintf(stderr, "--variance needs --temporal and --denoise\n");
        return usage();
    }
    if ((adaptive_n0 != 0) != !adaptive_out.empty()) {
        std::fprintf(stderr, "--adaptive and --adaptive-out go together\n");
        return usage();
    }
    // Without options this is the reference's main() exactly: Begin/Draw/End with nothing set,
    // so BeginRenderingOperation takes the reference's compile-time configuration (1280x720,
    // 1 spp, depth 50, its camera: globals.glsl:9-24) and its world[] (the final scene).
    if (configured) {
        std::vector<vcrt_sphere> world(8192);
        const int n = vcrt_scene_builtin(scene, world.data(), static_cast<int32_t>(world.size()));
        if (n < 0) return 1;
        world.resize(n);
        SetRenderDescription(&desc);
        SetRenderScene(world.data(), n);
    }
    VkResult r = BeginRenderingOperation();
    if (r != VK_SUCCESS) {
        std::fprintf(stderr, "BeginRenderingOperation: %s\n", vcrt_result_string(r));
        return 1;
    }
    // --temporal: the accumulated output, this frame's planes and the previous frame's
    const size_t pixels = static_cast<size_t>(desc.width) * desc.height;
    std::vector<float> acc, acc_len, next, next_len, colour, motion, surface, prev_surface;
    // --variance: the moments carried with the accumulation, and this frame's guide buffers
    std::vector<float> mom, next_mom, v_albedo, v_normal;
    if (!temporal.empty()) {
        for (std::vector<float>* v : {&acc, &next, &colour, &motion, &surface, &prev_surface})
            v->assign(4 * pixels, 0.0f);
        acc_len.assign(pixels, 0.0f);
        next_len.assign(pixels, 0.0f);
    }
    if (variance)
        for (std::vector<float>* v : {&mom, &next_mom, &v_albedo, &v_normal})
            v->assign(4 * pixels, 0.0f);
    const uint32_t guide_samples = static_cast<uint32_t>(
        feature_samples > 0 ? feature_samples : desc.samples_per_pixel);
    vcrt_camera prev_cam = desc.camera;
    for (int f = 0; f < frames && r == VK_SUCCESS; f++) {
        vcrt_camera now_cam = f == 0 ? desc.camera : prev_cam;
        if (f >= 1 && orbit != 0.0) {
            // frame f looks from the command line's lookfrom turned by f * DEG about the y axis
            // through lookat (in double, rounded to float); the move rebuilds the lists on the GPU
            const double th = f * orbit * 3.14159265358979323846 / 180.0;
            const double dx = static_cast<double>(desc.camera.lookfrom[0]) - desc.camera.lookat[0];
            const double dz = static_cast<double>(desc.camera.lookfrom[2]) - desc.camera.lookat[2];
            vcrt_camera cam = desc.camera;
            cam.lookfrom[0] = static_cast<float>(desc.camera.lookat[0] + dx * std::cos(th) +
                                                 dz * std::sin(th));
            cam.lookfrom[2] = static_cast<float>(desc.camera.lookat[2] - dx * std::sin(th) +
                                                 dz * std::cos(th));
            if ((r = SetRenderCamera(&cam)) != VK_SUCCESS) break;
            now_cam = cam;
        }
        r = DrawNextFrame();
        vcrt_stats st;
        vcrt_get_stats(&st);
        const double msps = static_cast<double>(st.samples) / (st.frame_ms * 1e3);
        std::printf("frame %d: %s  %.3f ms (kernel %.3f ms)  %.2f Msamples/s  %llu segments\n",
                    f, vcrt_result_string(r), st.frame_ms, st.kernel_ms, msps,
                    static_cast<unsigned long long>(st.segments));
        if (r == VK_SUCCESS && !temporal.empty()) {
            // frame 0 starts the sequence (out = frame, every length 1); a later frame gathers
            // the previous output where the previous camera saw its surfaces
            r = ReadFramebuffer(colour.data(), colour.size());
            if (r == VK_SUCCESS)
                r = DrawMotion(f == 0 ? nullptr : &prev_cam, nullptr, 0, motion.data(),
                               surface.data());
            if (r == VK_SUCCESS && variance) {
                // the moments ride along from the first frame on: frame 0 runs on history planes
                // of zeros (every tap rejected: out = frame, every length 1, the moments Y, Y^2)
                r = DrawFeatures(0, guide_samples, v_albedo.data(), v_normal.data(), nullptr);
                if (r == VK_SUCCESS)
                    r = ReprojectMoments(colour.data(), motion.data(), acc.data(),
                                         prev_surface.data(), acc_len.data(), v_albedo.data(),
                                         mom.data(), desc.width, desc.height, nullptr, next.data(),
                                         next_len.data(), next_mom.data());
                acc.swap(next);
                acc_len.swap(next_len);
                mom.swap(next_mom);
            } else if (r == VK_SUCCESS && f == 0) {
                acc = colour;
                acc_len.assign(pixels, 1.0f);
            } else if (r == VK_SUCCESS) {
                r = Reproject(colour.data(), motion.data(), acc.data(), prev_surface.data(),
                              acc_len.data(), desc.width, desc.height, nullptr, next.data(),
                              next_len.data());
                acc.swap(next);
                acc_len.swap(next_len);
            }
            prev_surface = surface;
            if (r != VK_SUCCESS) std::fprintf(stderr, "temporal: %s\n", vcrt_result_string(r));
        }
        prev_cam = now_cam;
    }
    if (r == VK_SUCCESS && !temporal.empty()) {
        const bool pfm =
            temporal.size() > 4 && temporal.compare(temporal.size() - 4, 4, ".pfm") == 0;
        std::vector<uint8_t> c8(pfm ? 0 : 4 * pixels);
        if (!pfm) {
            float th[255];
            vcrt_srgb8_thresholds(th);
            for (size_t i = 0; i < 4 * pixels; i++)
                c8[i] = static_cast<uint8_t>(std::upper_bound(th, th + 255, acc[i]) - th);
        }
        if (!write_image(temporal, desc.width, desc.height, pfm, acc, c8)) {
            std::fprintf(stderr, "cannot write %s: %s\n", temporal.c_str(), std::strerror(errno));
            r = VK_ERROR_UNKNOWN;
        }
    }
    if (r == VK_SUCCESS && !out.empty()) {
        const bool pfm = out.size() > 4 && out.compare(out.size() - 4, 4, ".pfm") == 0;
        const size_t n = static_cast<size_t>(desc.width) * desc.height;
        std::vector<float> rgba(pfm ? n * 4 : 0);
        std::vector<uint8_t> srgb(pfm ? 0 : n * 4);
        r = pfm ? ReadFramebuffer(rgba.data(), rgba.size())
                : vcrt_read_framebuffer_srgb8(srgb.data(), srgb.size());  // GPU sRGB encode
        if (r != VK_SUCCESS || !write_image(out, desc.width, desc.height, pfm, rgba, srgb)) {
            std::fprintf(stderr, "cannot write %s: %s\n", out.c_str(),
                         r == VK_SUCCESS ? std::strerror(errno) : vcrt_result_string(r));
            if (r == VK_SUCCESS) r = VK_ERROR_UNKNOWN;
        }
    }
    if (r == VK_SUCCESS && !features.empty()) {
        // the guide buffers of the last frame's camera: albedo as it is (linear, clamped), the
        // averaged normal mapped (n + 1) / 2
        const size_t n = static_cast<size_t>(desc.width) * desc.height;
        const uint32_t samples = static_cast<uint32_t>(
            feature_samples > 0 ? feature_samples : desc.samples_per_pixel);
        std::vector<float> albedo(4 * n), normal(4 * n);
        r = DrawFeatures(0, samples, albedo.data(), normal.data(), nullptr);
        if (r == VK_SUCCESS) {
            std::vector<uint8_t> a8(4 * n), n8(4 * n);
            for (size_t i = 0; i < 4 * n; i++) {
                a8[i] = unit_byte(albedo[i]);
                n8[i] = unit_byte(0.5f * (normal[i] + 1.0f));
            }
            const std::vector<float> none;
            if (!write_image(features + "_albedo.ppm", desc.width, desc.height, false, none, a8) ||
                !write_image(features + "_normal.ppm", desc.width, desc.height, false, none, n8)) {
                std::fprintf(stderr, "cannot write %s_*.ppm: %s\n", features.c_str(),
                             std::strerror(errno));
                r = VK_ERROR_UNKNOWN;
            }
        } else {
            std::fprintf(stderr, "DrawFeatures: %s\n", vcrt_result_string(r));
        }
    }
    if (r == VK_SUCCESS && !ao.empty()) {
        // the ambient visibility of the last frame's camera, encoded as a frame's PPM is: byte =
        // the number of sRGB8 thresholds the channel reaches (vcrt_srgb8_thresholds)
        const size_t n = static_cast<size_t>(desc.width) * desc.height;
        const uint32_t samples = static_cast<uint32_t>(
            feature_samples > 0 ? feature_samples : desc.samples_per_pixel);
        std::vector<float> plane(4 * n);
        r = DrawOcclusion(0, samples, static_cast<uint32_t>(ao_rays > 0 ? ao_rays : 0), 1e5f,
                          plane.data());
        if (r == VK_SUCCESS) {
            float th[255];
            vcrt_srgb8_thresholds(th);
            std::vector<uint8_t> v8(4 * n);
            for (size_t i = 0; i < 4 * n; i++)
                v8[i] = static_cast<uint8_t>(std::upper_bound(th, th + 255, plane[i]) - th);
            const std::vector<float> none;
            if (!write_image(ao + "_ao.ppm", desc.width, desc.height, false, none, v8)) {
                std::fprintf(stderr, "cannot write %s_ao.ppm: %s\n", ao.c_str(),
                             std::strerror(errno));
                r = VK_ERROR_UNKNOWN;
            }
        } else {
            std::fprintf(stderr, "DrawOcclusion: %s\n", vcrt_result_string(r));
        }
    }
    if (r == VK_SUCCESS && !denoise.empty()) {
        // the last frame (with --temporal: the accumulated one) through the a-trous filter,
        // steered by its own guide buffers; a PPM is encoded as a frame's is: byte = the number
        // of sRGB8 thresholds the channel reaches
        const bool pfm = denoise.size() > 4 && denoise.compare(denoise.size() - 4, 4, ".pfm") == 0;
        const size_t n = static_cast<size_t>(desc.width) * desc.height;
        const uint32_t samples = static_cast<uint32_t>(
            feature_samples > 0 ? feature_samples : desc.samples_per_pixel);
        std::vector<float> frame(4 * n), albedo(4 * n), normal(4 * n), clean(4 * n);
        vcrt_denoise_params dp;
        if (variance) vcrt_default_denoise_variance_params(&dp);
        else vcrt_default_denoise_params(&dp);
        if (denoise_levels != 0) dp.levels = denoise_levels;
        if (temporal.empty()) r = ReadFramebuffer(frame.data(), frame.size());
        else frame = acc;  // the accumulated frame
        if (r == VK_SUCCESS) r = DrawFeatures(0, samples, albedo.data(), normal.data(), nullptr);
        if (r == VK_SUCCESS && variance) {
            // the last frame's moments and surfaces give the variance that steers the filter
            std::vector<float> var(n);
            r = Variance(mom.data(), prev_surface.data(), desc.width, desc.height, nullptr,
                         var.data());
            if (r == VK_SUCCESS)
                r = DenoiseVariance(frame.data(), albedo.data(), normal.data(), var.data(),
                                    desc.width, desc.height, &dp, clean.data(), nullptr);
        } else if (r == VK_SUCCESS) {
            r = Denoise(frame.data(), albedo.data(), normal.data(), desc.width, desc.height, &dp,
                        clean.data());
        }
        if (r == VK_SUCCESS) {
            std::vector<uint8_t> c8(pfm ? 0 : 4 * n);
            if (!pfm) {
                float th[255];
                vcrt_srgb8_thresholds(th);
                for (size_t i = 0; i < 4 * n; i++)
                    c8[i] = static_cast<uint8_t>(std::upper_bound(th, th + 255, clean[i]) - th);
            }
            if (!write_image(denoise, desc.width, desc.height, pfm, clean, c8)) {
                std::fprintf(stderr, "cannot write %s: %s\n", denoise.c_str(),
                             std::strerror(errno));
                r = VK_ERROR_UNKNOWN;
            }
        } else {
            std::fprintf(stderr, "Denoise: %s\n", vcrt_result_string(r));
        }
    }
    if (r == VK_SUCCESS && adaptive_n0 != 0) {
        const bool pfm = adaptive_out.size() > 4 &&
                         adaptive_out.compare(adaptive_out.size() - 4, 4, ".pfm") == 0;
        const size_t n = static_cast<size_t>(desc.width) * desc.height;
        const uint32_t n0 = static_cast<uint32_t>(adaptive_n0);
        std::vector<uint16_t> counts(n, static_cast<uint16_t>(n0));
        std::vector<float> sums(4 * n), mean1(4 * n), mean(4 * n), var(n);
        // two uniform rounds into one sums plane: the means after the first and after both
        r = DrawSamples(0, n0, counts.data(), 0, sums.data(), mean1.data());
        if (r == VK_SUCCESS) r = DrawSamples(n0, n0, counts.data(), 1, sums.data(), mean.data());
        uint64_t total = 0;
        if (r == VK_SUCCESS) {
            const float scale = 2.0f * static_cast<float>(n0);
            for (size_t i = 0; i < n; i++) {
                const float d = lum(&mean[4 * i]) - lum(&mean1[4 * i]);
                const float dd = d * d;
                var[i] = dd * scale;
            }
            vcrt_sample_count_params cp;
            cp.struct_size = sizeof(cp);
            cp.target = adaptive_target;
            cp.min_count = 0;
            cp.max_count = static_cast<uint32_t>(adaptive_max);
            r = SampleCounts(var.data(), static_cast<uint32_t>(n), &cp, counts.data(), &total);
        }
        if (r == VK_SUCCESS)
            r = DrawSamples(2u * n0, static_cast<uint32_t>(adaptive_max), counts.data(), 1,
                            sums.data(), mean.data());
        if (r == VK_SUCCESS) {
            std::printf("adaptive: %u + %u uniform samples per pixel, %llu adaptive samples "
                        "(%.2f per pixel)\n", n0, n0, static_cast<unsigned long long>(total),
                        static_cast<double>(total) / static_cast<double>(n));
            std::vector<uint8_t> c8(pfm ? 0 : 4 * n);
            if (!pfm) {
                float th[255];
                vcrt_srgb8_thresholds(th);
                for (size_t i = 0; i < 4 * n; i++)
                    c8[i] = static_cast<uint8_t>(std::upper_bound(th, th + 255, mean[i]) - th);
            }
            if (!write_image(adaptive_out, desc.width, desc.height, pfm, mean, c8)) {
                std::fprintf(stderr, "cannot write %s: %s\n", adaptive_out.c_str(),
                             std::strerror(errno));
                r = VK_ERROR_UNKNOWN;
            }
        } else {
            std::fprintf(stderr, "adaptive: %s\n", vcrt_result_string(r));
        }
    }
    EndRenderingOperation();
    return r == VK_SUCCESS ? 0 : 1;
}
