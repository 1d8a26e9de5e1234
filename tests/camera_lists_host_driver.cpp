// camera_lists_host_driver.cpp -- csrc/camera_lists.hip compiled for the host (the stub runtime in
// tests/camera_lists_host) and run one thread at a time against primary.cpp's builders: the
// prepare, count and fill kernels as they are; the scan (one workgroup with barriers) replaced by
// its serial statement. Prints, per case, the sizes and the number of differences (bad).
#include "hip/hip_runtime.h"
#include "camera_lists.hip"
#include "cluster.hpp"
#include "scene.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace vcrt;
template <class K> void run(K k, CameraListParams& p, uint32_t threads) {
    gridDim.x = (threads + 255) / 256;
    for (uint32_t b = 0; b < gridDim.x; b++) for (uint32_t t = 0; t < 256; t++) { blockIdx.x = b; threadIdx.x = t; k(p); }
}
int check(int scene_id, int W, int H, int rank, int world, const float lf[3], const float la[3], float vfov) {
    std::vector<vcrt_sphere> world_s; builtin_scene(scene_id, world_s);
    CullTables ct; build_cull_tables(world_s.data(), (int)world_s.size(), ct);
    if (ct.ngroups == 0) { printf("no tables\n"); return 0; }
    Camera cam = make_camera(W, H, mk(lf[0], lf[1], lf[2]), mk(la[0], la[1], la[2]), mk(0, 1, 0), vfov, [](double x) { return std::tan(x); });
    const f3 v[4] = {cam.pixel00, cam.delta_u, cam.delta_v, cam.center};
    float c[12]; for (int i = 0; i < 4; i++) { c[3*i] = v[i].x; c[3*i+1] = v[i].y; c[3*i+2] = v[i].z; }
    PrimaryLists pl; build_primary_lists(ct, c, W, H, rank, world, pl);
    PrimarySphereLists sl; build_primary_sphere_lists(ct, world_s.data(), c, W, H, rank, world, sl);
    std::vector<float> crec; build_camera_records(ct, c, crec); crec.resize((size_t)ct.nbig * 16);
    // device inputs
    const int nall = ct.nbig + ct.ngroups;
    std::vector<float> rec((size_t)nall * 20);
    for (int gi = 0; gi < nall; gi++) { memcpy(&rec[gi*20], &ct.geom[gi*16], 64); memcpy(&rec[gi*20+16], &ct.index[gi*4], 16); }
    std::vector<float> cr(world_s.size() * 4);
    for (size_t i = 0; i < world_s.size(); i++) { cr[4*i] = world_s[i].center[0]; cr[4*i+1] = world_s[i].center[1]; cr[4*i+2] = world_s[i].center[2]; cr[4*i+3] = world_s[i].radius; }
    CameraListParams p{};
    for (int i = 0; i < 12; i++) p.cam[i] = c[i];
    const double* o = &p.cam[9];
    const double on = std::sqrt(o[0]*o[0] + o[1]*o[1] + o[2]*o[2]);
    p.Q = (on + ct.margin[0]) * (on + ct.margin[0]) + ct.margin[1];
    const double* du = &p.cam[3]; const double* dv = &p.cam[6];
    p.ex = 1e-3 / std::sqrt(du[0]*du[0] + du[1]*du[1] + du[2]*du[2]);
    p.ey = 1e-3 / std::sqrt(dv[0]*dv[0] + dv[1]*dv[1] + dv[2]*dv[2]);
    for (int a = 0; a < 3; a++) p.o[a] = c[9+a];
    p.n = (uint32_t)pl.info.size(); p.ngroups = ct.ngroups; p.nnodes = ct.ngroups / 8; p.ntops = (ct.ngroups + 63) / 64;
    p.nbig = ct.nbig; p.nspheres = (uint32_t)world_s.size(); p.rank = rank; p.world = world; p.tiles_x = (W + 7) / 8; p.ids_ok = 1;
    p.ctop = ct.top.data(); p.cnode = ct.node.data(); p.cbound = ct.bound.data(); p.cgroup = rec.data(); p.center_radius = cr.data();
    std::vector<double> boxes((size_t)(p.ngroups + p.nnodes + p.ntops) * 8), sph((size_t)p.nspheres * 8);
    std::vector<uint32_t> counts(4 * (size_t)p.n + 2), info(2 * (size_t)p.n);
    p.boxes = boxes.data(); p.spheres = sph.data(); p.counts = counts.data(); p.offsets = p.counts + 2 * p.n; p.totals = p.offsets + 2 * p.n; p.prim_info = info.data();
    blockDim.x = 256;
    run(vcrt_camlist_prepare, p, 256 * 8);
    run(vcrt_camlist_count, p, p.n);
    uint32_t a = 0, b = 0;
    for (uint32_t e = 0; e < p.n; e++) { p.offsets[2*e] = a; p.offsets[2*e+1] = b; if (p.counts[2*e] != kCamListNone) a += p.counts[2*e]; if (p.counts[2*e+1] != kCamListNone) b += (p.counts[2*e+1] + 1) / 2; }
    p.totals[0] = a; p.totals[1] = b;
    std::vector<uint16_t> ids(a + 1); std::vector<float> cam_rec((size_t)p.nbig * 16 + (size_t)b * 12 + 12, 7.0f);
    p.prim_ids = ids.data(); p.cam_rec = cam_rec.data();
    run(vcrt_camlist_fill, p, std::max(std::max(p.n, p.nbig), 12u));
    int bad = 0;
    if (a != pl.ids.size() || b != sl.rec.size() / 12) { printf("  totals differ %u/%zu %u/%zu\n", a, pl.ids.size(), b, sl.rec.size()/12); return 1; }
    for (uint32_t e = 0; e < p.n; e++) if (info[2*e] != pl.info[e] || info[2*e+1] != sl.info[e]) bad++;
    if (a && memcmp(ids.data(), pl.ids.data(), a * 2)) bad++, printf("  ids differ\n");
    if (b && memcmp(&cam_rec[(size_t)p.nbig*16], sl.rec.data(), (size_t)b * 48)) bad++, printf("  rec differ\n");
    if (p.nbig && memcmp(cam_rec.data(), crec.data(), (size_t)p.nbig * 64)) bad++, printf("  big rec differ\n");
    for (int i = 0; i < 12; i++) if (cam_rec[(size_t)p.nbig*16 + (size_t)b*12 + i] != 0.0f) bad++;
    uint32_t gl = 0, sl_n = 0; for (uint32_t e = 0; e < p.n; e++) { gl += pl.info[e] != 15; sl_n += sl.info[e] != 15; }
    printf("n %u ids %u pairs %u glisted %u slisted %u bad %d\n", p.n, a, b, gl, sl_n, bad);
    return bad;
}
int main(int argc, char** argv) {
    // scene id, width, height, rank, world, lookfrom (3), lookat (3), vfov
    if (argc != 13) return 2;
    const float lf[3] = {strtof(argv[6], nullptr), strtof(argv[7], nullptr), strtof(argv[8], nullptr)};
    const float la[3] = {strtof(argv[9], nullptr), strtof(argv[10], nullptr), strtof(argv[11], nullptr)};
    return check(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), lf, la,
                 strtof(argv[12], nullptr)) != 0;
}
