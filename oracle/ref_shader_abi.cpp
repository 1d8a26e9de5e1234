// C ABI over the reference's compute shader compiled as C++ (oracle/_ref/shader, produced from
// the reference's own files by glsl_rewrite.py at build time). TEST INFRASTRUCTURE ONLY.
// The shader's state is global, as in GLSL: one call at a time, no threads.
//
// Compile with -std=c++20 -ffp-contract=off -fsingle-precision-constant -I oracle/_ref.
#include "ref_shader_abi.h"

#include "glsl_shim.h"

namespace ref_glsl {
#include "shader/shader.comp"
}  // namespace ref_glsl

namespace {

using namespace ref_glsl;

constexpr int kDefaultWorldN = static_cast<int>(sizeof(ref_world_default) / sizeof(ref_world_default[0]));

sphere* g_world_copy = nullptr;
int g_world_cap = 0;

// Point the shader's `world` at the caller's spheres (copied field by field), or at the
// reference's own array when world is null.
void set_world(const ref_sphere* w, int32_t n) {
    if (w == nullptr) {
        world = ref_world_default;
        ref_world_n = kDefaultWorldN;
        return;
    }
    if (n > g_world_cap) {
        delete[] g_world_copy;
        g_world_copy = new sphere[n];
        g_world_cap = n;
    }
    for (int i = 0; i < n; i++) {
        g_world_copy[i].center = vec3(w[i].center[0], w[i].center[1], w[i].center[2]);
        g_world_copy[i].radius = w[i].radius;
        g_world_copy[i].colour = vec3(w[i].colour[0], w[i].colour[1], w[i].colour[2]);
        g_world_copy[i].texture = vec3(w[i].texture[0], w[i].texture[1], w[i].texture[2]);
    }
    world = g_world_copy;
    ref_world_n = n;
}

vec3 load3(const float* p) { return vec3(p[0], p[1], p[2]); }

}  // namespace

extern "C" {

int32_t ref_default_world(ref_sphere* out, int32_t cap) {
    for (int i = 0; i < kDefaultWorldN && i < cap; i++) {
        const sphere& s = ref_world_default[i];
        out[i] = ref_sphere{{s.center.x, s.center.y, s.center.z}, s.radius,
                            {s.colour.x, s.colour.y, s.colour.z},
                            {s.texture.x, s.texture.y, s.texture.z}};
    }
    return kDefaultWorldN;
}

void ref_default_config(ref_config* c) {
    c->width = IMAGE_WIDTH; c->height = IMAGE_HEIGHT;
    c->spp = SAMPLES_PER_PIXEL; c->max_depth = MAX_RECURSION_LEVEL;
    c->lookfrom[0] = camera_lookfrom.x; c->lookfrom[1] = camera_lookfrom.y; c->lookfrom[2] = camera_lookfrom.z;
    c->lookat[0] = camera_lookat.x; c->lookat[1] = camera_lookat.y; c->lookat[2] = camera_lookat.z;
    c->vup[0] = camera_vup.x; c->vup[1] = camera_vup.y; c->vup[2] = camera_vup.z;
    c->vfov = camera_vfov;
}

int64_t ref_render_pixels(const ref_config* cfg, const ref_sphere* w, int32_t n, const int32_t* xy,
                          int32_t npixels, float* rgba, int32_t* undefined) {
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->spp <= 0 || cfg->max_depth < 0) return -1;
    for (int i = 0; i < npixels; i++)
        if (xy[2 * i] < 0 || xy[2 * i] >= cfg->width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= cfg->height)
            return -1;
    set_world(w, n);
    IMAGE_WIDTH = cfg->width;
    IMAGE_HEIGHT = cfg->height;
    SAMPLES_PER_PIXEL = cfg->spp;
    MAX_RECURSION_LEVEL = cfg->max_depth;
    camera_lookfrom = load3(cfg->lookfrom);
    camera_lookat = load3(cfg->lookat);
    camera_vup = load3(cfg->vup);
    camera_vfov = cfg->vfov;
    int64_t total = 0;
    for (int i = 0; i < npixels; i++) {
        gl_GlobalInvocationID = uvec3(static_cast<uint32_t>(xy[2 * i]), static_cast<uint32_t>(xy[2 * i + 1]), 0u);
        ref_undefined_count = 0;
        ref_shader_main();
        if (ref_stored_coord.x != xy[2 * i] || ref_stored_coord.y != xy[2 * i + 1]) return -2;
        rgba[4 * i + 0] = ref_stored_color.x;
        rgba[4 * i + 1] = ref_stored_color.y;
        rgba[4 * i + 2] = ref_stored_color.z;
        rgba[4 * i + 3] = ref_stored_color.w;
        if (undefined) undefined[i] = static_cast<int32_t>(ref_undefined_count);
        total += ref_undefined_count;
    }
    return total;
}

int32_t ref_ray_color(const ref_sphere* w, int32_t n, const float origin[3], const float dir[3],
                      int32_t max_depth, float rgb[3]) {
    set_world(w, n);
    MAX_RECURSION_LEVEL = max_depth;
    ref_undefined_count = 0;
    const vec3 c = ray_color(ray(load3(origin), load3(dir)));
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    return static_cast<int32_t>(ref_undefined_count);
}

int32_t ref_hit_scan(const ref_sphere* w, int32_t n, const float origin[3], const float dir[3],
                     float min_t, float max_t, float* t, int32_t* index, float normal[3]) {
    set_world(w, n);
    const ray r = ray(load3(origin), load3(dir));
    hit_record rec;
    rec.min_t = min_t;
    rec.max_t = max_t;
    int32_t accepted = 0;
    *index = -1;
    for (int i = 0; i < ref_world_n; i++) {  // the loop is ours, hit_sphere the reference's
        if (hit_sphere(world[i], r, rec)) {
            accepted = 1;
            *index = i;
        }
    }
    *t = rec.max_t;
    normal[0] = rec.normal.x; normal[1] = rec.normal.y; normal[2] = rec.normal.z;
    return accepted;
}

float ref_rand(float x, float y) { return rand(vec2(x, y)); }

}  // extern "C"
