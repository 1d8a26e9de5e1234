/* ref_shader_abi.h -- C ABI of oracle/_ref/libref_shader.so: the reference's compute shader,
 * compiled as C++ from the reference's own files at build time (oracle/Makefile `ref`), under the
 * canonical built-ins of DESIGN.md section 3. TEST INFRASTRUCTURE ONLY; independent of
 * oracle/vcrt_oracle.c, which the tests compare it with. Not thread-safe (the shader's state is
 * global). A null `world` means the reference's own scene array. */
#ifndef REF_SHADER_ABI_H
#define REF_SHADER_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ref_sphere { /* field order of the shader's struct: 40 bytes */
    float center[3];
    float radius;
    float colour[3];
    float texture[3];
} ref_sphere;

typedef struct ref_config {
    int32_t width, height, spp, max_depth;
    float lookfrom[3], lookat[3], vup[3];
    float vfov;
} ref_config;

/* The reference's own scene (returns its length; writes at most cap) and configuration. */
int32_t ref_default_world(ref_sphere* out, int32_t cap);
void ref_default_config(ref_config* cfg);

/* The shader's entry point once per pixel of xy (npixels (x, y) pairs): rgba = what it stores,
 * undefined[i] (optional) = how often ray_color flowed off its end for pixel i (each such sample
 * counted as the canonical vec3(0)). Returns their total, or < 0 on a bad argument. */
int64_t ref_render_pixels(const ref_config* cfg, const ref_sphere* world, int32_t n,
                          const int32_t* xy, int32_t npixels, float* rgba, int32_t* undefined);

/* ray_color of one ray at MAX_RECURSION_LEVEL = max_depth. Returns 1 if it flowed off its end. */
int32_t ref_ray_color(const ref_sphere* world, int32_t n, const float origin[3],
                      const float dir[3], int32_t max_depth, float rgb[3]);

/* hit_sphere over the array in index order on one hit_record that starts at (min_t, max_t).
 * Returns whether any sphere accepted; t = the record's max_t afterwards, index = the last
 * accepting sphere (-1), normal = the record's (0 when nothing accepted). */
int32_t ref_hit_scan(const ref_sphere* world, int32_t n, const float origin[3],
                     const float dir[3], float min_t, float max_t, float* t, int32_t* index,
                     float normal[3]);

float ref_rand(float x, float y);

#ifdef __cplusplus
}
#endif
#endif
