// cluster.hpp -- spatial grouping of the sphere list for the culled scan (variant CULL).
//
// The reference scans world[] linearly for every ray (functions.glsl:77-81). Because that scan
// picks the smallest accepted t with ties to the earliest index (tracer.hip, scan_culled), the
// spheres can be visited in any order; this module reorders them into spatially compact groups
// of four with conservative axis-aligned boxes so a wave can skip groups no lane's ray comes
// near.
#pragma once

#include <cstdint>
#include <vector>

#include "scene_update_abi.h"
#include "vcrt.h"

namespace vcrt {

constexpr int kNodeGroups = 8;  // groups per node of the box hierarchy
constexpr size_t kFlatGroups16 = 1024;  // = vcrt::kFlatMaxGroups (10-bit entry fields)

struct CullTables {
    int32_t nbig = 0;             // big-sphere groups, first in geom/index, tested for every ray
    int32_t ngroups = 0;          // hierarchy groups after them, a multiple of 2 * kNodeGroups
    std::vector<float> geom;      // [nbig + ngroups][16] pair-SoA, same values as the linear table
    std::vector<int32_t> index;   // [nbig + ngroups][4] world[] index of each member, -1 = padding
    std::vector<float> bound;     // [ngroups / 2][16] hierarchy group-pair boxes (TraceParams)
    std::vector<float> node;      // [ngroups / kNodeGroups / 2][16] node-pair boxes, same form
    std::vector<float> top;       // [ceil(ngroups / 64) rounded up to even / 2][16] boxes of
                                  // each 64-group chunk (8 nodes), same form
    float margin[4] = {0, 0, 0, 0};  // box-test constants over the hierarchy: max |centre|,
                                     // r_max^2, max |coordinate| of a box (rounded up), 0
    // The shared y slab (tracer.hip "Culled scan", fact (3a)): set when every non-padding group,
    // node and chunk box has the same finite lo[1] and hi[1], bit for bit (the generated scenes:
    // every hierarchy sphere at one height with one radius). The flat scans then evaluate the
    // y planes once per ray instead of once per box. VCRT_SLAB=0 leaves it unset (A/B).
    bool slab = false;
    float slab_lohi[2] = {0, 0};  // that lo[1], hi[1] (slab only)
    // The footprint tables of the LDS-table flat scan (tracer.hip "Culled scan", fact (5)): node
    // bit masks by the cell of one x or z coordinate, cell(X) = trunc(med3(fma(X, scale, offset),
    // 0, kFootprintCells - 1)) in fp32. With ue(i) the largest and le(i) the smallest float of
    // cell i (found with that very function; -+inf at the ends) and g = 8u |e| + 2^-100:
    //   fp_tab[0][i] = nodes with lo.x <= ue(i) + g,   fp_tab[1][i] = nodes with hi.x >= le(i) - g,
    // [2] and [3] the same for z; over the node boxes that have members (bit = node index, at most
    // 32 nodes; a padding node has no bit). A scene they cannot describe (more than 32 nodes, a
    // degenerate extent, a coordinate bound below 2^-20) gets all-ones masks. They do not depend
    // on VCRT_SLAB.
    std::vector<uint32_t> fp_tab;  // [4][kFootprintCells]
    float fp_x[2] = {1, 0};        // scale, offset of the x cells
    float fp_z[2] = {1, 0};
    float fp_y[2] = {0, 0};        // y extent of all those node boxes (= slab_lohi on a slab scene)
    float fp_k2 = 0;               // 2 x the largest finite K of those boxes, rounded up
    uint32_t fp_always = 0;        // nodes whose K is +inf: every ray keeps them
    // The group-level footprint tables (tracer.hip fact (5g)): the same rule over the group boxes
    // that have members, bit = hierarchy group index, masks of 128 bits (four words, low first);
    // gf_cells cells per table (group_footprint_cells: the LDS bytes of the group boxes and node
    // tables they replace). Built for every scene of at most 128 groups whose extent the cells
    // can describe (else gf_cells = 0); gf_ok says whether a frame may use them in place of the
    // node level: additionally every group box with members has one y extent, bit for bit (the
    // geometric condition: it does not depend on VCRT_SLAB), and VCRT_GROUP_FOOT is not 0. The
    // renderer further needs the camera-ray lists (capi.cpp).
    std::vector<uint32_t> gf_tab;  // [4][gf_cells][4]
    int32_t gf_cells = 0;
    float gf_x[2] = {1, 0};        // scale, offset of the x cells
    float gf_z[2] = {1, 0};
    float gf_k2 = 0;               // 2 x the largest finite K of those boxes, rounded up
    uint32_t gf_always[4] = {0, 0, 0, 0};  // groups whose K is +inf
    bool gf_one_height = false;    // every group box with members has the y extent fp_y
    bool gf_ok = false;
    // how scalars_of_summary left the two levels for fill_footprints and the refit kernels:
    // the node masks follow the rule (else all-ones); every group cell keeps gf_always
    bool fp_ok = false;
    bool gf_keep_all = false;
};

constexpr int kFootprintCells = 84;  // = vcrt::kFootCells (vcrt_kernel_abi.h)
constexpr int kGroupFootprintMaxGroups = 128;  // = vcrt::kGroupFootMaxGroups

// Cells per group-level table for a hierarchy of ngroups (= vcrt::group_foot_cells).
int group_footprint_cells(int32_t ngroups);

// The cell of coordinate x among n cells, as the kernel computes it.
int footprint_cell_n(float x, const float scale_offset[2], int n);

// The cell of coordinate x, as the kernel computes it.
int footprint_cell(float x, const float scale_offset[2]);

// Builds the grouped tables. Returns false (tables empty) when culling does not apply: fewer
// than 16 spheres or any centre/radius outside +-2^30 (or not finite).
bool build_cull_tables(const vcrt_sphere* spheres, int32_t count, CullTables& out);

// Its two halves. choose_grouping fills nbig, ngroups and index alone (false as above);
// tables_of_grouping fills everything else of `out` from the values of `spheres` and the
// grouping `out` holds, which need not be the one choose_grouping gives for these values
// (vcrt_update_spheres keeps a scene's grouping while its spheres move): the boxes are the
// members' whatever the members are, so the culled scans stay exact and only get slower as the
// groups spread. Every |centre|, |radius| must be <= 2^30.
bool choose_grouping(const vcrt_sphere* spheres, int32_t count, CullTables& out);
void tables_of_grouping(const vcrt_sphere* spheres, int32_t count, CullTables& out);

// tables_of_grouping's steps after the boxes, apart so the device refit (scene_update.hip) can
// take the middle one with a summary it reduced itself: the maxima and minima of the spheres and
// boxes (scene_update_abi.h); every scalar of `out` from them (out.ngroups set, the scalars at
// their defaults); the footprint tables from out's boxes and scalars.
void summary_of_tables(const vcrt_sphere* spheres, int32_t count, const CullTables& ct,
                       SceneSummary& m);
void scalars_of_summary(const SceneSummary& m, CullTables& out);
void fill_footprints(CullTables& out);

// Primary-ray lists (the flat scan's camera rays skip the node level): for every 4x4-pixel
// quarter of every local 8x8 tile, the hierarchy groups a camera ray through it may need, by a
// conservative pyramid-box test in double (primary.cpp). info[4 lt + 2 qy + qx] =
// offset << 4 | count, count <= 8, or kPrimaryNone (those camera rays take the hierarchy).
constexpr uint32_t kPrimaryMax = 8;
constexpr uint32_t kPrimaryNone = 15;

struct PrimaryLists {
    std::vector<uint32_t> info;  // [4 x local tiles]
    std::vector<uint16_t> ids;   // hierarchy group indices, by tile
};

// cam: pixel00, delta_u, delta_v, centre (shader.comp:18-43) as the kernels get them.
void build_primary_lists(const CullTables& ct, const float cam[12], int32_t width,
                         int32_t height, int32_t rank, int32_t world, PrimaryLists& out);

// Per-sphere camera lists (round 3) for the camera fast trace: for every 4x4-pixel quarter of
// every local tile, the hierarchy's spheres a camera ray through it may need (the members of its
// group list whose sphere, grown by its own margin M_s = 8.1u (|oc|^2 + r^2) / r and 1e-3, no
// side plane of the quarter's pyramid separates: primary.cpp), as camera-relative pair records:
// per pair of spheres (ocx0,ocx1,ocy0,ocy1) (ocz0,ocz1,cc0,cc1) (index0,index1 as int bits,0,0),
// evaluated as pair_disc_cc would (an odd count pads its last pair with oc = 0, cc = 3e38, index
// -1: never a candidate). info[4 lt + 2 qy + qx] = first pair << 4 | spheres (<= 14), or
// kPrimaryNone. On average ~1.1 spheres per quarter at the final scene's 1080p camera, against
// ~10.6 members of the listed groups.
constexpr uint32_t kPrimarySphereMax = 14;

struct PrimarySphereLists {
    std::vector<uint32_t> info;  // [4 x local tiles]
    std::vector<float> rec;      // [pairs][12]
};

void build_primary_sphere_lists(const CullTables& ct, const vcrt_sphere* spheres,
                                const float cam[12], int32_t width, int32_t height, int32_t rank,
                                int32_t world, PrimarySphereLists& out);

// Camera-relative group records for the camera fast trace: for every group of ct.geom (big
// groups first), the members' oc = camera centre - centre and cc = |oc|^2 - r^2 in the group
// record's pair-SoA form, (ocx0,ocx1,ocy0,ocy1) (ocz0,ocz1,cc0,cc1) per pair, evaluated in fp32
// with the kernel's operations and order (tracer.hip pair_disc_cc), so a camera ray's hb and
// discriminant from them carry the same bits. [nbig + ngroups][16] floats.
void build_camera_records(const CullTables& ct, const float cam[12], std::vector<float>& out);

}  // namespace vcrt
