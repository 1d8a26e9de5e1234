// scene_update_abi.h -- the argument block and the summary of the scene-refit kernels
// (scene_update.hip), shared with the host (capi.cpp vcrt_update_spheres, cluster.cpp). One
// struct for the four kernels; each reads what it needs.
#pragma once

#include <cstdint>

namespace vcrt {

constexpr uint32_t kSceneSummaryThreads = 1024;  // the levels-and-summary kernel's one workgroup

// What the host needs of a refitted scene to compute every scalar of CullTables
// (cluster.cpp scalars_of_summary): maxima and minima only, so any order of reduction gives the
// same bits. Floats travel as ordered keys (float_order_key below: the key rises with the value,
// -0 below +0) or, where they are never negative, as their bits.
struct SceneSummary {
    double c2max, rmax, lam;  // the hierarchy's spheres: max |c|^2, max |r|, max (|c_a| + |r|)
    uint32_t lo_min[3], hi_max[3];  // keys: the extent of the group boxes that have members
    uint32_t ylo_max, yhi_min;      // keys: with lo_min[1], hi_max[1] the "one y extent" decision
    uint32_t boxes;                 // group boxes that have members
    uint32_t node_kmax;             // bits: the largest finite K of the node boxes with members
    uint32_t node_always;           // nodes (below 32) whose K is +inf
    uint32_t node_real;             // nodes (below 32) that have members
    uint32_t group_kmax;            // bits: the largest finite K of those group boxes
    uint32_t group_always[4];       // groups (below 128) whose K is +inf
    uint32_t group_real[4];         // groups (below 128) that have members
    uint32_t bounded, radii_safe;   // every sphere: |centre|, |radius| <= 2^30; 2^-40 <= |radius|
};
static_assert(sizeof(SceneSummary) <= 256, "one small read-back");

inline constexpr uint32_t kKeyNegInf = 0x007fffffu, kKeyPosInf = 0xff800000u;

// floats in order: key(x) rises with x (-inf .. +inf, -0 below +0); cluster.cpp float_key
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t float_order_key(uint32_t bits) {
    return (bits & 0x80000000u) ? 0x7fffffffu - (bits & 0x7fffffffu) : 0x80000000u + bits;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t float_order_bits(uint32_t key) {
    return key >= 0x80000000u ? key - 0x80000000u : 0x80000000u | (0x7fffffffu - key);
}

struct SceneUpdateParams {
    const float* spheres;  // [nspheres][10]: vcrt_sphere
    // the tables vcrt_set_scene allocated, rewritten in place
    float* geom;           // [nspheres / 4 rounded up + 1][16] the linear pair-SoA table
    float* center_radius;  // [nspheres][4]
    float* shade;          // [nspheres][4]
    float* material;       // [nspheres][4]
    float* cgroup;         // [nbig + ngroups][20]: geometry rewritten, the 4 index words kept
    float* cbound;         // [ngroups / 2][16]
    float* cbound_nf;      // [ngroups / 2][20]
    float* cnode;          // [nnodes / 2][16]
    float* cnode_nf;       // [nnodes / 2 rounded up to 4][20], the padding left zero
    float* ctop;           // [ntops rounded up to even / 2][16]
    uint32_t* fp_tab;      // the node footprint tables, packed (capi.cpp pack_footprint)
    uint32_t* gf_tab;      // [4][gf_n][4] the group footprint tables (null: none)
    SceneSummary* summary;
    uint32_t nspheres, nbig, ngroups, nnodes, ntops;
    // vcrt_scene_footprint: the scalars the host computed from the summary
    float fp_x[2], fp_z[2], gf_x[2], gf_z[2];
    uint32_t fp_ok;        // 1: masks by the rule; 0: all-ones
    uint32_t gf_n;         // cells per group table (0: no group tables)
    uint32_t gf_keep_all;  // 1: every cell keeps the groups that have members
};

}  // namespace vcrt
