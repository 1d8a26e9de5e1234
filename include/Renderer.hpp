/* Renderer.hpp -- the reference's renderer lifecycle (include/Renderer.hpp:14-20) on MI355X.
 *
 * Same three entry points with the same meaning: Begin builds everything the frame loop
 * needs (device buffers, the tracer code object, the scene), DrawNextFrame renders one full
 * frame and returns when it is complete, End tears down and tolerates a partial Begin.
 * The reference's compile-time configuration (globals.glsl:9-24, Common.hpp:23-24) becomes a
 * vcrt_render_desc that may be set before Begin. */
#ifndef VCRT_RENDERER_HPP
#define VCRT_RENDERER_HPP

#include "Common.hpp"

// Create pipeline, submit tasks...
VkResult BeginRenderingOperation(void);

// Draw next frame, to be called by platform handlers (here: the headless frame loop).
VkResult DrawNextFrame(void);

// End rendering & destroy allocated environments.
VkResult EndRenderingOperation(void);

// Additions: configuration and output access (no counterpart in the reference).
VkResult SetRenderDescription(IN const vcrt_render_desc* desc);
VkResult SetRenderScene(IN const vcrt_sphere* spheres, IN int32_t count);
VkResult ReadFramebuffer(OUT float* rgba, IN size_t count);
// Moves the camera of the running renderer (vcrt_set_camera); a later Begin starts from it too.
VkResult SetRenderCamera(IN const vcrt_camera* camera);
// Moves the spheres of the running renderer (vcrt_update_spheres: same count, the tables refitted
// on the GPU); a later Begin starts from the new values too.
VkResult UpdateSpheres(IN const vcrt_sphere* spheres, IN int32_t count);
// The guide buffers of the frame's camera rays for sample indices first .. first + n - 1
// (vcrt_draw_features: host pointers in the framebuffer's layout; any may be NULL, not all).
VkResult DrawFeatures(IN uint32_t first, IN uint32_t n, OUT float* albedo, OUT float* normal_depth,
                      OUT int32_t* sphere);
// The ambient visibility buffer of the same rays (vcrt_draw_occlusion: m secondary rays of reach
// `reach` per sample that hits; a host pointer in the framebuffer's layout).
VkResult DrawOcclusion(IN uint32_t first, IN uint32_t n, IN uint32_t m, IN float reach,
                       OUT float* visibility);
// The denoised frame (vcrt_denoise: the edge-avoiding a-trous filter over a colour plane and
// DrawFeatures' albedo and normal_depth, host pointers, [height][width] float4 each; a guide may
// be NULL, which switches its terms off; params NULL takes vcrt_default_denoise_params).
VkResult Denoise(IN const float* colour, IN const float* albedo, IN const float* normal_depth,
                 IN int32_t width, IN int32_t height, IN const vcrt_denoise_params* params,
                 OUT float* out);
// The reprojection map of the frame's pixels (vcrt_draw_motion: where each pixel's surface lay in
// the frame of prev_camera and prev_spheres, NULL for the current ones; host pointers in the
// framebuffer's layout, float4 each; either plane may be NULL, not both).
VkResult DrawMotion(IN const vcrt_camera* prev_camera, IN const vcrt_sphere* prev_spheres,
                    IN int32_t count, OUT float* motion, OUT float* surface);
// Temporal accumulation (vcrt_reproject: the previous output gathered through DrawMotion's map and
// blended with the new frame; host pointers, [height][width] float4 each and float for the two
// lengths; params NULL takes vcrt_default_reproject_params).
VkResult Reproject(IN const float* colour, IN const float* motion, IN const float* history_colour,
                   IN const float* history_surface, IN const float* history_length,
                   IN int32_t width, IN int32_t height, IN const vcrt_reproject_params* params,
                   OUT float* out, OUT float* out_length);
// Variance-guided denoising (vcrt_reproject_moments, vcrt_variance, vcrt_denoise_variance; host
// pointers, [height][width] float4 each and float for the lengths and the variances).
// ReprojectMoments is Reproject with the luminance moments carried along: albedo may be NULL,
// history_moments is the previous call's out_moments. Variance turns out_moments and the frame's
// surface plane into the per-pixel variance DenoiseVariance steers its colour term with;
// out_variance may be NULL. params NULL takes the calls' defaults.
VkResult ReprojectMoments(IN const float* colour, IN const float* motion,
                          IN const float* history_colour, IN const float* history_surface,
                          IN const float* history_length, IN const float* albedo,
                          IN const float* history_moments, IN int32_t width, IN int32_t height,
                          IN const vcrt_reproject_moments_params* params, OUT float* out,
                          OUT float* out_length, OUT float* out_moments);
VkResult Variance(IN const float* moments, IN const float* surface, IN int32_t width,
                  IN int32_t height, IN const vcrt_variance_params* params, OUT float* variance);
VkResult DenoiseVariance(IN const float* colour, IN const float* albedo,
                         IN const float* normal_depth, IN const float* variance, IN int32_t width,
                         IN int32_t height, IN const vcrt_denoise_params* params, OUT float* out,
                         OUT float* out_variance);
// Adaptive sampling (vcrt_draw_samples, vcrt_sample_counts; host pointers in the framebuffer's
// layout). DrawSamples traces min(counts[p], max_count) further samples of the frame's own rays per
// pixel, the sample indices from `first` on, into sums (float4: radiance sum, sample count; added
// to when accumulate != 0) and mean (float4, may be NULL). SampleCounts turns a variance plane
// (float) into the count plane (uint16) that reaches the standard deviation params->target; total
// (may be NULL) receives the sum of the counts.
VkResult DrawSamples(IN uint32_t first, IN uint32_t max_count, IN const uint16_t* counts,
                     IN int32_t accumulate, OUT float* sums, OUT float* mean);
VkResult SampleCounts(IN const float* variance, IN uint32_t elements,
                      IN const vcrt_sample_count_params* params, OUT uint16_t* counts,
                      OUT uint64_t* total);

#endif
