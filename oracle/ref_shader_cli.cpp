// ref_shader_cli -- stand-alone driver of the reference shader compiled as C++
// (ref_shader_abi.h). Reads commands from the file named on the command line (or stdin), floats as
// 8-digit hex bit patterns so that NaNs and signed zeros survive, and prints results the same way:
//
//   world N            then N x 10 words (centre, radius, colour, texture); N = -1: the reference's
//   frame W H SPP DEPTH  then 10 words (lookfrom, lookat, vup, vfov), NPIX and NPIX x y pairs
//                        (NPIX = -1: every pixel, row by row)   -> "p r g b a undefined" per pixel
//   ray DEPTH          then 6 words (origin, direction)        -> "c r g b undefined"
//   scan               then 8 words (origin, direction, min_t, max_t)
//                                                              -> "h accepted t index nx ny nz"
//   rand               then 2 words                            -> "r value"
// TEST INFRASTRUCTURE ONLY.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ref_shader_abi.h"

static bool word(FILE* f, float* out) {
    unsigned u;
    if (fscanf(f, "%x", &u) != 1) return false;
    uint32_t v = u;
    memcpy(out, &v, 4);
    return true;
}

static unsigned bits(float x) {
    uint32_t v;
    memcpy(&v, &x, 4);
    return v;
}

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<ref_sphere> world;
    bool own_world = false;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        const ref_sphere* w = own_world ? world.data() : nullptr;
        const int32_t n = own_world ? static_cast<int32_t>(world.size()) : 0;
        if (!strcmp(cmd, "world")) {
            int count;
            if (fscanf(f, "%d", &count) != 1) return 3;
            own_world = count >= 0;
            world.assign(own_world ? count : 0, ref_sphere{});
            for (auto& s : world) {
                float v[10];
                for (float& x : v)
                    if (!word(f, &x)) return 3;
                memcpy(s.center, v, 12);
                s.radius = v[3];
                memcpy(s.colour, v + 4, 12);
                memcpy(s.texture, v + 7, 12);
            }
        } else if (!strcmp(cmd, "frame")) {
            ref_config c;
            int npix;
            if (fscanf(f, "%d %d %d %d", &c.width, &c.height, &c.spp, &c.max_depth) != 4) return 3;
            float v[10];
            for (float& x : v)
                if (!word(f, &x)) return 3;
            memcpy(c.lookfrom, v, 12);
            memcpy(c.lookat, v + 3, 12);
            memcpy(c.vup, v + 6, 12);
            c.vfov = v[9];
            if (fscanf(f, "%d", &npix) != 1) return 3;
            std::vector<int32_t> xy;
            if (npix < 0) {
                if (c.width <= 0 || c.height <= 0 || c.width > 65535 || c.height > 65535) return 3;
                for (int y = 0; y < c.height; y++)
                    for (int x = 0; x < c.width; x++) {
                        xy.push_back(x);
                        xy.push_back(y);
                    }
            } else {
                xy.resize(2 * static_cast<size_t>(npix));
                for (int32_t& x : xy)
                    if (fscanf(f, "%d", &x) != 1) return 3;
            }
            const int32_t count = static_cast<int32_t>(xy.size() / 2);
            std::vector<float> rgba(4 * static_cast<size_t>(count) + 1);
            std::vector<int32_t> undef(static_cast<size_t>(count) + 1);
            if (ref_render_pixels(&c, w, n, xy.data(), count, rgba.data(), undef.data()) < 0) return 4;
            for (int i = 0; i < count; i++)
                printf("p %08x %08x %08x %08x %d\n", bits(rgba[4 * i]), bits(rgba[4 * i + 1]),
                       bits(rgba[4 * i + 2]), bits(rgba[4 * i + 3]), undef[i]);
        } else if (!strcmp(cmd, "ray")) {
            int depth;
            float v[6], rgb[3];
            if (fscanf(f, "%d", &depth) != 1) return 3;
            for (float& x : v)
                if (!word(f, &x)) return 3;
            const int u = ref_ray_color(w, n, v, v + 3, depth, rgb);
            printf("c %08x %08x %08x %d\n", bits(rgb[0]), bits(rgb[1]), bits(rgb[2]), u);
        } else if (!strcmp(cmd, "scan")) {
            float v[8], t, nrm[3];
            int32_t index;
            for (float& x : v)
                if (!word(f, &x)) return 3;
            const int acc = ref_hit_scan(w, n, v, v + 3, v[6], v[7], &t, &index, nrm);
            printf("h %d %08x %d %08x %08x %08x\n", acc, bits(t), index, bits(nrm[0]), bits(nrm[1]),
                   bits(nrm[2]));
        } else if (!strcmp(cmd, "rand")) {
            float v[2];
            if (!word(f, v) || !word(f, v + 1)) return 3;
            printf("r %08x\n", bits(ref_rand(v[0], v[1])));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd);
            return 3;
        }
    }
    if (f != stdin) fclose(f);
    return 0;
}
