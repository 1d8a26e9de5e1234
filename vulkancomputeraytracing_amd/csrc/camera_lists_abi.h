// camera_lists_abi.h -- the argument block of the camera-list kernels (camera_lists.hip), shared
// with the host (capi.cpp vcrt_set_camera). One struct for the four kernels; each reads what it
// needs.
#pragma once

#include <cstdint>

namespace vcrt {

constexpr uint32_t kCamListNone = 0xFFFFFFFFu;  // a quarter's count: no list
constexpr uint32_t kCamListBox = 8;             // doubles per grown box / per sphere entry
constexpr uint32_t kCamListScanThreads = 1024;  // the scan's one workgroup

struct CameraListParams {
    // the scene's tables as vcrt_set_scene uploaded them
    const float* ctop;            // chunk-pair boxes, 16 floats per pair (CullTables::top)
    const float* cnode;           // node-pair boxes
    const float* cbound;          // group-pair boxes
    const float* cgroup;          // [nbig + ngroups][20]: pair-SoA geometry, 4 member indices
    const float* center_radius;   // [nspheres][4]
    // per camera, from vcrt_camlist_prepare
    double* boxes;    // [ngroups + nnodes + ntops][8]: c - o (3), half extent (3), always, real
    double* spheres;  // [nspheres][8]: c - o (3), R = r + M_s + 1e-3, always
    // per quarter e = 4 lt + 2 qy + qx
    uint32_t* counts;   // [2 n]: groups, spheres (kCamListNone: no list)
    uint32_t* offsets;  // [2 n]: first id, first pair
    uint32_t* totals;   // [2]: ids, pairs
    // the lists a frame reads (TraceParams.prim_info / prim_ids / cam_rec)
    uint32_t* prim_info;  // [2 n] interleaved
    uint16_t* prim_ids;
    float* cam_rec;       // [nbig][16], then the pair records [pairs][12], then 12 zeros
    double cam[12];       // pixel00, delta_u, delta_v, centre: the fp32 camera widened
    double Q;             // (|o| + c_max)^2 + r_max^2
    double ex, ey;        // 1e-3 / |delta_u|, 1e-3 / |delta_v|
    float o[3];           // the centre in fp32 (the records' arithmetic)
    uint32_t n;           // quarters: 4 x local tiles
    uint32_t ngroups, nnodes, ntops, nbig, nspheres;
    uint32_t rank, world, tiles_x;
    uint32_t ids_ok;      // group ids fit uint16
};

}  // namespace vcrt
