// Renderer.cpp -- the reference's Renderer lifecycle (include/Renderer.hpp:14-20) over the
// C ABI. Begin/Draw/End keep their names, signatures and VkResult convention; the reference's
// compile-time configuration becomes SetRenderDescription / SetRenderScene (optional: without
// them Begin uses the reference defaults of globals.glsl:9-24 and its final scene).
#include <vector>

#include "Renderer.hpp"

namespace {
vcrt_render_desc g_desc;
bool g_desc_set = false;
std::vector<vcrt_sphere> g_scene;
bool g_scene_set = false;
}  // namespace

VkResult SetRenderDescription(IN const vcrt_render_desc* desc) {
    if (!desc) return VK_ERROR_INITIALIZATION_FAILED;
    g_desc = *desc;
    g_desc_set = true;
    return VK_SUCCESS;
}

VkResult SetRenderScene(IN const vcrt_sphere* spheres, IN int32_t count) {
    if (count < 0 || (count > 0 && !spheres)) return VK_ERROR_INITIALIZATION_FAILED;
    g_scene.assign(spheres, spheres + count);
    g_scene_set = true;
    return VK_SUCCESS;
}

// Create pipeline, submit tasks...
VkResult BeginRenderingOperation(void) {
    if (!g_desc_set) vcrt_default_desc(&g_desc);
    VkResult r = vcrt_begin(&g_desc);
    if (r != VK_SUCCESS) return r;
    if (g_scene_set) {
        r = vcrt_set_scene(g_scene.data(), static_cast<int32_t>(g_scene.size()));
        if (r != VK_SUCCESS) {
            vcrt_end();
            return r;
        }
    }
    return VK_SUCCESS;
}

// Draw next frame: one full render, returns when the frame is complete.
VkResult DrawNextFrame(void) { return vcrt_draw_next_frame(); }

// End rendering & destroy allocated environments (idempotent).
VkResult EndRenderingOperation(void) { return vcrt_end(); }

VkResult ReadFramebuffer(OUT float* rgba, IN size_t count) {
    return vcrt_read_framebuffer(rgba, count);
}

VkResult SetRenderCamera(IN const vcrt_camera* camera) {
    const VkResult r = vcrt_set_camera(camera);
    if (r == VK_SUCCESS && g_desc_set) g_desc.camera = *camera;
    return r;
}

VkResult UpdateSpheres(IN const vcrt_sphere* spheres, IN int32_t count) {
    const VkResult r = vcrt_update_spheres(spheres, count);
    if (r == VK_SUCCESS && g_scene_set) g_scene.assign(spheres, spheres + count);
    return r;
}

VkResult DrawFeatures(IN uint32_t first, IN uint32_t n, OUT float* albedo, OUT float* normal_depth,
                      OUT int32_t* sphere) {
    return static_cast<VkResult>(
        vcrt_draw_features(first, n, albedo, normal_depth, sphere, nullptr));
}

VkResult DrawOcclusion(IN uint32_t first, IN uint32_t n, IN uint32_t m, IN float reach,
                       OUT float* visibility) {
    return static_cast<VkResult>(vcrt_draw_occlusion(first, n, m, reach, visibility, nullptr));
}

VkResult Denoise(IN const float* colour, IN const float* albedo, IN const float* normal_depth,
                 IN int32_t width, IN int32_t height, IN const vcrt_denoise_params* params,
                 OUT float* out) {
    return static_cast<VkResult>(
        vcrt_denoise(colour, albedo, normal_depth, width, height, params, out, nullptr));
}

VkResult DrawMotion(IN const vcrt_camera* prev_camera, IN const vcrt_sphere* prev_spheres,
                    IN int32_t count, OUT float* motion, OUT float* surface) {
    return static_cast<VkResult>(
        vcrt_draw_motion(prev_camera, prev_spheres, count, motion, surface, nullptr));
}

VkResult Reproject(IN const float* colour, IN const float* motion, IN const float* history_colour,
                   IN const float* history_surface, IN const float* history_length,
                   IN int32_t width, IN int32_t height, IN const vcrt_reproject_params* params,
                   OUT float* out, OUT float* out_length) {
    return static_cast<VkResult>(vcrt_reproject(colour, motion, history_colour, history_surface,
                                                history_length, width, height, params, out,
                                                out_length, nullptr));
}

VkResult ReprojectMoments(IN const float* colour, IN const float* motion,
                          IN const float* history_colour, IN const float* history_surface,
                          IN const float* history_length, IN const float* albedo,
                          IN const float* history_moments, IN int32_t width, IN int32_t height,
                          IN const vcrt_reproject_moments_params* params, OUT float* out,
                          OUT float* out_length, OUT float* out_moments) {
    return static_cast<VkResult>(vcrt_reproject_moments(
        colour, motion, history_colour, history_surface, history_length, albedo, history_moments,
        width, height, params, out, out_length, out_moments, nullptr));
}

VkResult Variance(IN const float* moments, IN const float* surface, IN int32_t width,
                  IN int32_t height, IN const vcrt_variance_params* params, OUT float* variance) {
    return static_cast<VkResult>(
        vcrt_variance(moments, surface, width, height, params, variance, nullptr));
}

VkResult DenoiseVariance(IN const float* colour, IN const float* albedo,
                         IN const float* normal_depth, IN const float* variance, IN int32_t width,
                         IN int32_t height, IN const vcrt_denoise_params* params, OUT float* out,
                         OUT float* out_variance) {
    return static_cast<VkResult>(vcrt_denoise_variance(colour, albedo, normal_depth, variance,
                                                       width, height, params, out, out_variance,
                                                       nullptr));
}

VkResult DrawSamples(IN uint32_t first, IN uint32_t max_count, IN const uint16_t* counts,
                     IN int32_t accumulate, OUT float* sums, OUT float* mean) {
    return static_cast<VkResult>(
        vcrt_draw_samples(first, max_count, counts, accumulate, sums, mean, nullptr));
}

VkResult SampleCounts(IN const float* variance, IN uint32_t elements,
                      IN const vcrt_sample_count_params* params, OUT uint16_t* counts,
                      OUT uint64_t* total) {
    vcrt_sample_count_stats st;
    const vcrt_result r = vcrt_sample_counts(variance, elements, params, counts, &st);
    if (r == VCRT_SUCCESS && total) *total = st.total;
    return static_cast<VkResult>(r);
}
