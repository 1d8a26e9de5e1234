// scene_update.hip -- the scene's tables refitted on the device (part 7 of vcrt_tracer.hsaco;
// vcrt_update_spheres). The grouping of a scene (the index words of its group records) is kept;
// every table that depends on the spheres' values is rewritten in place with the very bytes
// cluster.cpp's tables_of_grouping and vcrt_set_scene's row formulas give for the new values:
// every decision below is the host's IEEE fp32 / fp64 operation in the host's order (contraction
// off, correctly rounded divides), restated here. cluster.hpp says why any grouping with
// conservative boxes keeps the culled scans exact; this file only has to repeat the arithmetic.
//
//   vcrt_scene_rows       a lane per entry of the linear table (its padding and prefetch group
//                         included): the pair-SoA entry and the sphere's three rows
//   vcrt_scene_groups     a lane per group, big groups first: the geometry record through the
//                         kept index words; a hierarchy group's box in both layouts
//   vcrt_scene_levels     one workgroup: the node and chunk boxes from the group boxes, and the
//                         summary (scene_update_abi.h) the host computes every scalar from
//   vcrt_scene_footprint  after the host has the scalars: a lane per word of the packed node
//                         tables and per cell of the group tables
//
// The work is a few thousand lanes; the kernels are launches and one read-back of about a hundred bytes, not
// throughput. All reductions are maxima, minima and ors (any order gives the same bits), taken
// per lane first and then with LDS atomics inside the one workgroup of vcrt_scene_levels: no
// global atomics and nothing crosses workgroups inside a kernel.
//
// Levels from group boxes: round_down and round_up rise with their argument, so the outward-
// rounded minimum over a node's members is the minimum of its groups' outward-rounded minima
// (and likewise the maxima); K = round_up(min(8.1u / r_min (1 + 1e-5), 1e38)) falls as r_min
// rises through correctly rounded, hence monotone, steps (+inf at r_min = 0), so a node's K is
// the largest K of its groups. A node's box over its members is therefore the union of its
// groups' boxes that have members, bit for bit, and a chunk's likewise.
#include <hip/hip_runtime.h>

#include "scene_update_abi.h"

#pragma clang fp contract(off)

namespace {

using vcrt::SceneSummary;
using vcrt::SceneUpdateParams;

constexpr uint32_t kNodeGroups = 8;      // cluster.hpp kNodeGroups
constexpr uint32_t kFootCells = 84;      // cluster.hpp kFootprintCells
constexpr double kU = 0x1p-24;           // fp32 unit roundoff
constexpr float kFar = 1e20f;            // cluster.cpp Box: a box without members
constexpr float kPadR2 = -3.0e38f;       // r^2 of a padding entry

__device__ float next_up(float f) {
    const uint32_t b = __float_as_uint(f);
    if (f == 0.0f) return __uint_as_float(1u);
    return __uint_as_float((b & 0x80000000u) ? b - 1u : b + 1u);
}

__device__ float next_down(float f) {
    const uint32_t b = __float_as_uint(f);
    if (f == 0.0f) return __uint_as_float(0x80000001u);
    return __uint_as_float((b & 0x80000000u) ? b + 1u : b - 1u);
}

// cluster.cpp round_up / round_down: the smallest float >= x, the largest <= x (x finite)
__device__ float round_up(double x) {
    float f = static_cast<float>(x);
    if (static_cast<double>(f) < x) f = next_up(f);
    return f;
}

__device__ float round_down(double x) {
    float f = static_cast<float>(x);
    if (static_cast<double>(f) > x) f = next_down(f);
    return f;
}

struct Box {
    float lo[3], hi[3], K;
};

__device__ Box empty_box() { return Box{{kFar, kFar, kFar}, {kFar, kFar, kFar}, 0.0f}; }

// element i of a pair-SoA box table (cluster.cpp put_box)
__device__ void put_box(float* table, uint32_t i, const Box& b) {
    float* t = table + static_cast<size_t>(i / 2u) * 16u;
    const uint32_t e = i % 2u;
    for (int a = 0; a < 3; a++) {
        t[2 * a + e] = b.lo[a];
        t[6 + 2 * a + e] = b.hi[a];
    }
    t[12 + e] = b.K;
}

__device__ Box get_box(const float* table, uint32_t i) {
    const float* t = table + static_cast<size_t>(i / 2u) * 16u;
    const uint32_t e = i % 2u;
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = t[2 * a + e];
        b.hi[a] = t[6 + 2 * a + e];
    }
    b.K = t[12 + e];
    return b;
}

// the same element in the near/far layout (capi.cpp near_far: 20 floats per pair, per axis
// lo0 lo1 hi0 hi1 lo0 lo1, then K0 K1)
__device__ void put_box_nf(float* table, uint32_t i, const Box& b) {
    float* o = table + static_cast<size_t>(i / 2u) * 20u;
    const uint32_t e = i % 2u;
    for (int a = 0; a < 3; a++) {
        o[6 * a + e] = o[6 * a + 4 + e] = b.lo[a];
        o[6 * a + 2 + e] = b.hi[a];
    }
    o[18 + e] = b.K;
}

__device__ bool has_members(const float* cgroup, uint32_t nbig, uint32_t gi) {
    const int32_t* idx =
        reinterpret_cast<const int32_t*>(cgroup + static_cast<size_t>(nbig + gi) * 20u + 16u);
    return idx[0] >= 0 || idx[1] >= 0 || idx[2] >= 0 || idx[3] >= 0;
}

// the union of the boxes of groups g0 .. g1 - 1 that have members (see the header comment)
__device__ Box union_box(const SceneUpdateParams& p, uint32_t g0, uint32_t g1) {
    Box u = empty_box();
    bool any = false;
    for (uint32_t gi = g0; gi < g1 && gi < p.ngroups; gi++) {
        if (!has_members(p.cgroup, p.nbig, gi)) continue;
        const Box b = get_box(p.cbound, gi);
        if (!any) {
            u = b;
            any = true;
            continue;
        }
        for (int a = 0; a < 3; a++) {
            // (ties keep the earlier value, as std::min / std::max over the members in group
            // order do: the sign of a zero edge is the host's)
            u.lo[a] = b.lo[a] < u.lo[a] ? b.lo[a] : u.lo[a];
            u.hi[a] = b.hi[a] > u.hi[a] ? b.hi[a] : u.hi[a];
        }
        u.K = b.K > u.K ? b.K : u.K;
    }
    return u;
}

__device__ uint32_t key_of(float x) { return vcrt::float_order_key(__float_as_uint(x)); }

// cluster.cpp footprint_cell_n: the cell of coordinate x among n cells, as the kernels compute it
__device__ int cell_of(float x, const float so[2], int n) {
    const float f = fmaf(x, so[0], so[1]);
    const float c = fminf(fmaxf(f, 0.0f), static_cast<float>(n - 1));
    return static_cast<int>(c);
}

// the largest float whose cell is <= i (i < n - 1): the cell never falls as x rises
__device__ float cell_upper(int i, const float so[2], int n) {
    int64_t lo = vcrt::kKeyNegInf, hi = vcrt::kKeyPosInf;
    while (hi - lo > 1) {  // cell(lo) <= i < cell(hi)
        const int64_t mid = lo + (hi - lo) / 2;
        const float x = __uint_as_float(vcrt::float_order_bits(static_cast<uint32_t>(mid)));
        if (cell_of(x, so, n) <= i)
            lo = mid;
        else
            hi = mid;
    }
    return __uint_as_float(vcrt::float_order_bits(static_cast<uint32_t>(lo)));
}

// The edge a table of cell i compares with (cluster.cpp fill_masks): for an A table
// up = ue(i) + g, for a B table dn = le(i) - g with le the largest float of the cell before.
__device__ double cell_edge(bool is_b, int i, const float so[2], int n) {
    const double inf = __builtin_inf();
    if (!is_b) {
        const double ue = i < n - 1 ? static_cast<double>(cell_upper(i, so, n)) : inf;
        return ue + (8.0 * kU * fabs(ue) + 0x1p-100);
    }
    const double le = i > 0 ? static_cast<double>(cell_upper(i - 1, so, n)) : -inf;
    return le - (8.0 * kU * fabs(le) + 0x1p-100);
}

// one 32-bit mask of a node table: flat cell c of [4][kFootCells]
__device__ uint32_t node_cell_mask(const SceneUpdateParams& p, uint32_t c) {
    if (!p.fp_ok) return 0xffffffffu;
    const uint32_t t = c / kFootCells;
    const int i = static_cast<int>(c % kFootCells);
    const int a = t < 2u ? 0 : 2;
    const bool is_b = (t & 1u) != 0u;
    const double edge = cell_edge(is_b, i, a == 0 ? p.fp_x : p.fp_z, kFootCells);
    const uint32_t real = p.summary->node_real;
    uint32_t m = 0u;
    for (uint32_t ni = 0; ni < p.nnodes && ni < 32u; ni++) {
        if (!((real >> ni) & 1u)) continue;
        const float* bt = p.cnode + static_cast<size_t>(ni / 2u) * 16u;
        const uint32_t e = ni % 2u;
        const bool in = is_b ? static_cast<double>(bt[6 + 2 * a + e]) >= edge
                             : static_cast<double>(bt[2 * a + e]) <= edge;
        if (in) m |= 1u << ni;
    }
    return m;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) vcrt_scene_rows(SceneUpdateParams p) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nlin = (p.nspheres + 3u) / 4u + 1u;  // groups of four, one more for the prefetch
    if (j >= 4u * nlin) return;
    const float* sp = p.spheres + static_cast<size_t>(j) * 10u;
    const bool real = j < p.nspheres;
    float cx = 0.f, cy = 0.f, cz = 0.f, r2 = kPadR2;
    if (real) {
        cx = sp[0];
        cy = sp[1];
        cz = sp[2];
        r2 = sp[3] * sp[3];
    }
    float* base = p.geom + static_cast<size_t>(j / 4u) * 16u + 8u * ((j % 4u) / 2u);
    const uint32_t e = j % 2u;
    base[0 + e] = cx;
    base[2 + e] = cy;
    base[4 + e] = cz;
    base[6 + e] = r2;
    if (!real) return;
    reinterpret_cast<float4*>(p.center_radius)[j] = make_float4(sp[0], sp[1], sp[2], sp[3]);
    reinterpret_cast<float4*>(p.shade)[j] = make_float4(sp[4], sp[5], sp[6], sp[8]);
    // the glass scatter's two per-sphere quotients, fp32 and correctly rounded (vcrt_set_scene)
    const float ior = sp[8];
    float r0 = (1.0f - ior) / (1.0f + ior);
    r0 = r0 * r0;
    reinterpret_cast<float4*>(p.material)[j] = make_float4(sp[7], 1.0f / ior, r0, 0.0f);
}

extern "C" __global__ void __launch_bounds__(256) vcrt_scene_groups(SceneUpdateParams p) {
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= p.nbig + p.ngroups) return;
    float* rec = p.cgroup + static_cast<size_t>(gi) * 20u;
    const int32_t* idx = reinterpret_cast<const int32_t*>(rec + 16);
    int32_t member[4];
    for (int k = 0; k < 4; k++) {
        member[k] = idx[k];
        // (an index outside the scene cannot come from vcrt_set_scene; never read past the array)
        if (member[k] >= static_cast<int32_t>(p.nspheres)) member[k] = -1;
    }
    Box b = empty_box();
    double rmin = __builtin_inf(), lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = __builtin_inf();
        hi[a] = -lo[a];
    }
    bool any = false;
    for (int k = 0; k < 4; k++) {
        float cx = 0.f, cy = 0.f, cz = 0.f, r2 = kPadR2;
        if (member[k] >= 0) {
            const float* sp = p.spheres + static_cast<size_t>(member[k]) * 10u;
            cx = sp[0];
            cy = sp[1];
            cz = sp[2];
            r2 = sp[3] * sp[3];
            // cluster.cpp box_of: centre -+ |radius| in fp64
            const double r = fabs(static_cast<double>(sp[3]));
            rmin = r < rmin ? r : rmin;
            for (int a = 0; a < 3; a++) {
                const double l = sp[a] - r, h = sp[a] + r;
                lo[a] = l < lo[a] ? l : lo[a];
                hi[a] = h > hi[a] ? h : hi[a];
            }
            any = true;
        }
        float* base = rec + 8 * (k / 2);
        const int e = k % 2;
        base[0 + e] = cx;
        base[2 + e] = cy;
        base[4 + e] = cz;
        base[6 + e] = r2;
    }
    if (gi < p.nbig) return;
    if (any) {
        if (rmin > 0.0) {
            const double k = 8.1 * kU / rmin * (1.0 + 1e-5);
            b.K = round_up(1e38 < k ? 1e38 : k);
        } else {
            b.K = __builtin_inff();
        }
        for (int a = 0; a < 3; a++) {
            b.lo[a] = round_down(lo[a]);
            b.hi[a] = round_up(hi[a]);
        }
    }
    put_box(p.cbound, gi - p.nbig, b);
    put_box_nf(p.cbound_nf, gi - p.nbig, b);
}

extern "C" __global__ void __launch_bounds__(vcrt::kSceneSummaryThreads)
vcrt_scene_levels(SceneUpdateParams p) {
    __shared__ unsigned long long s_f64[3];  // c2max, rmax, lam: the bits of doubles >= 0
    __shared__ uint32_t s_min[5], s_max[7];
    __shared__ uint32_t s_or[10], s_and[2];
    const uint32_t tid = threadIdx.x, nth = blockDim.x;
    if (tid == 0) {
        for (int k = 0; k < 3; k++) s_f64[k] = 0ull;
        for (int k = 0; k < 5; k++) s_min[k] = vcrt::kKeyPosInf;
        for (int k = 0; k < 7; k++) s_max[k] = k < 4 ? vcrt::kKeyNegInf : 0u;
        for (int k = 0; k < 10; k++) s_or[k] = 0u;
        s_and[0] = s_and[1] = 1u;
    }
    __syncthreads();
    // the node and chunk boxes; the nodes' part of the summary
    uint32_t node_kmax = 0u, node_always = 0u, node_real = 0u;
    for (uint32_t ni = tid; ni < p.nnodes; ni += nth) {
        const Box b = union_box(p, ni * kNodeGroups, (ni + 1u) * kNodeGroups);
        put_box(p.cnode, ni, b);
        put_box_nf(p.cnode_nf, ni, b);
        bool members = false;
        for (uint32_t gi = ni * kNodeGroups; gi < (ni + 1u) * kNodeGroups; gi++)
            members = members || has_members(p.cgroup, p.nbig, gi);
        if (!members) continue;
        if (ni < 32u) node_real |= 1u << ni;
        if (isinf(b.K)) {
            if (ni < 32u) node_always |= 1u << ni;
        } else {
            node_kmax = max(node_kmax, __float_as_uint(b.K));
        }
    }
    const uint32_t ntops2 = p.ntops + (p.ntops & 1u);
    for (uint32_t ti = tid; ti < ntops2; ti += nth)
        put_box(p.ctop, ti, union_box(p, ti * 64u, ti * 64u + 64u));
    // the group boxes with members
    uint32_t lo_min[3] = {vcrt::kKeyPosInf, vcrt::kKeyPosInf, vcrt::kKeyPosInf};
    uint32_t hi_max[3] = {vcrt::kKeyNegInf, vcrt::kKeyNegInf, vcrt::kKeyNegInf};
    uint32_t ylo_max = vcrt::kKeyNegInf, yhi_min = vcrt::kKeyPosInf, boxes = 0u, group_kmax = 0u;
    double c2max = 0.0, rmax = 0.0, lam = 0.0;
    const bool masks = p.ngroups <= 128u;
    for (uint32_t gi = tid; gi < p.ngroups; gi += nth) {
        if (!has_members(p.cgroup, p.nbig, gi)) continue;
        const Box b = get_box(p.cbound, gi);
        boxes++;
        for (int a = 0; a < 3; a++) {
            lo_min[a] = min(lo_min[a], key_of(b.lo[a]));
            hi_max[a] = max(hi_max[a], key_of(b.hi[a]));
        }
        ylo_max = max(ylo_max, key_of(b.lo[1]));
        yhi_min = min(yhi_min, key_of(b.hi[1]));
        if (masks) atomicOr(&s_or[2 + (gi >> 5)], 1u << (gi & 31u));
        if (isinf(b.K)) {
            if (masks) atomicOr(&s_or[6 + (gi >> 5)], 1u << (gi & 31u));
        } else {
            group_kmax = max(group_kmax, __float_as_uint(b.K));
        }
        // the margin constants over the hierarchy's spheres (cluster.cpp summary_of_tables)
        const int32_t* idx = reinterpret_cast<const int32_t*>(
            p.cgroup + static_cast<size_t>(p.nbig + gi) * 20u + 16u);
        for (int k = 0; k < 4; k++) {
            const int32_t j = idx[k];
            if (j < 0 || j >= static_cast<int32_t>(p.nspheres)) continue;
            const float* sp = p.spheres + static_cast<size_t>(j) * 10u;
            const double r = fabs(static_cast<double>(sp[3]));
            rmax = r > rmax ? r : rmax;
            double c2 = 0.0;
            for (int a = 0; a < 3; a++) {
                const double c = sp[a];
                c2 += c * c;
                const double l = fabs(c) + r;
                lam = l > lam ? l : lam;
            }
            c2max = c2 > c2max ? c2 : c2max;
        }
    }
    // the two flags over every sphere (NaN fails both)
    bool bounded = true, radii_safe = true;
    for (uint32_t j = tid; j < p.nspheres; j += nth) {
        const float* sp = p.spheres + static_cast<size_t>(j) * 10u;
        for (int a = 0; a < 4; a++)
            if (!(fabsf(sp[a]) <= 0x1p30f)) bounded = false;
        if (!(fabsf(sp[3]) >= 0x1p-40f && fabsf(sp[3]) <= 0x1p30f)) radii_safe = false;
    }
    if (boxes > 0u) {
        for (int a = 0; a < 3; a++) {
            atomicMin(&s_min[a], lo_min[a]);
            atomicMax(&s_max[a], hi_max[a]);
        }
        atomicMax(&s_max[3], ylo_max);
        atomicMin(&s_min[3], yhi_min);
        atomicAdd(&s_max[6], boxes);
        atomicMax(&s_max[5], group_kmax);
        atomicMax(&s_f64[0], static_cast<unsigned long long>(__double_as_longlong(c2max)));
        atomicMax(&s_f64[1], static_cast<unsigned long long>(__double_as_longlong(rmax)));
        atomicMax(&s_f64[2], static_cast<unsigned long long>(__double_as_longlong(lam)));
    }
    if (node_real != 0u) {
        atomicMax(&s_max[4], node_kmax);
        atomicOr(&s_or[0], node_always);
        atomicOr(&s_or[1], node_real);
    }
    if (!bounded) atomicAnd(&s_and[0], 0u);
    if (!radii_safe) atomicAnd(&s_and[1], 0u);
    __syncthreads();
    if (tid == 0) {
        SceneSummary m;
        m.c2max = __longlong_as_double(static_cast<long long>(s_f64[0]));
        m.rmax = __longlong_as_double(static_cast<long long>(s_f64[1]));
        m.lam = __longlong_as_double(static_cast<long long>(s_f64[2]));
        for (int a = 0; a < 3; a++) {
            m.lo_min[a] = s_min[a];
            m.hi_max[a] = s_max[a];
        }
        m.ylo_max = s_max[3];
        m.yhi_min = s_min[3];
        m.boxes = s_max[6];
        m.node_kmax = s_max[4];
        m.node_always = s_or[0];
        m.node_real = s_or[1];
        m.group_kmax = s_max[5];
        for (int k = 0; k < 4; k++) {
            m.group_real[k] = s_or[2 + k];
            m.group_always[k] = s_or[6 + k];
        }
        m.bounded = s_and[0];
        m.radii_safe = s_and[1];
        *p.summary = m;
    }
}

extern "C" __global__ void __launch_bounds__(256) vcrt_scene_footprint(SceneUpdateParams p) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    // the node tables as capi.cpp pack_footprint packs them: two 16-bit masks per word up to 128
    // groups (kFootCells is even, so a word never straddles two tables), else one mask per word
    const bool packed = p.ngroups <= 128u;
    const uint32_t node_words = packed ? 2u * kFootCells : 4u * kFootCells;
    if (t < node_words) {
        p.fp_tab[t] = packed ? (node_cell_mask(p, 2u * t) & 0xffffu) | (node_cell_mask(p, 2u * t + 1u) << 16)
                             : node_cell_mask(p, t);
        return;
    }
    const uint32_t c = t - node_words;  // flat cell of [4][gf_n]
    if (p.gf_n == 0u || p.gf_tab == nullptr || c >= 4u * p.gf_n) return;
    uint32_t real[4], m[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < 4; k++) real[k] = p.summary->group_real[k];
    if (p.gf_keep_all) {
        for (int k = 0; k < 4; k++) m[k] = real[k];
    } else {
        const uint32_t tb = c / p.gf_n;
        const int i = static_cast<int>(c % p.gf_n);
        const int a = tb < 2u ? 0 : 2;
        const bool is_b = (tb & 1u) != 0u;
        const double edge = cell_edge(is_b, i, a == 0 ? p.gf_x : p.gf_z, static_cast<int>(p.gf_n));
        for (uint32_t gi = 0; gi < p.ngroups && gi < 128u; gi++) {
            if (!((real[gi >> 5] >> (gi & 31u)) & 1u)) continue;
            const float* bt = p.cbound + static_cast<size_t>(gi / 2u) * 16u;
            const uint32_t e = gi % 2u;
            const bool in = is_b ? static_cast<double>(bt[6 + 2 * a + e]) >= edge
                                 : static_cast<double>(bt[2 * a + e]) <= edge;
            if (in) m[gi >> 5] |= 1u << (gi & 31u);
        }
    }
    reinterpret_cast<uint4*>(p.gf_tab)[c] = make_uint4(m[0], m[1], m[2], m[3]);
}
