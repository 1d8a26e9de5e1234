// camera_lists.hip -- the camera-ray lists of primary.cpp, built on the device (part 6 of
// vcrt_tracer.hsaco; vcrt_set_camera). The lists are what primary.cpp's build_primary_lists,
// build_primary_sphere_lists and build_camera_records write, byte for byte: every decision below
// is the host's IEEE fp64 operation in the host's order (contraction off), restated here because
// the host's walker keeps std::vector state. primary.cpp's header comment says why the test is
// conservative; this file only has to repeat it.
//
//   vcrt_camlist_prepare   per box / sphere / big group: the values that depend on the camera but
//                          not on the quarter (grown_box, the member's radius r + M_s + 1e-3)
//   vcrt_camlist_count     a lane per quarter: walks chunks -> nodes -> groups in hierarchy order
//                          and the found groups' members; writes the quarter's two counts
//   vcrt_camlist_scan      one workgroup: exclusive scan of the counts in entry order, which is
//                          the host's serial concatenation; the two totals
//   vcrt_camlist_fill      the same walk again, writing ids, pair records and prim_info at the
//                          scanned offsets; the big groups' records and the 12 trailing zeros
//
// A lane per quarter: a wave's 64 quarters are 16 neighbouring tiles, so its lanes descend into
// much the same boxes and the box loads coalesce to a few lines. Every loop runs over a table
// size; a camera with NaN or infinite components makes every comparison false, so every box is
// kept and the walk ends at the 65th group (or at the table's end) with "no list".
#include <hip/hip_runtime.h>

#include "camera_lists_abi.h"
#include "vcrt_math.h"

#pragma clang fp contract(off)

namespace {

using vcrt::CameraListParams;
using vcrt::kCamListBox;
using vcrt::kCamListNone;

constexpr double kExtra = 1e-3;          // primary.cpp QuarterWalker::kExtra
constexpr uint32_t kGroupCap = 8;        // cluster.hpp kPrimaryMax
constexpr uint32_t kWalkCap = 64;        // the sphere lists' group walk
constexpr uint32_t kSphereCap = 14;      // cluster.hpp kPrimarySphereMax
constexpr uint32_t kInfoNone = 15;       // cluster.hpp kPrimaryNone
constexpr uint32_t kNodeGroups = 8;      // cluster.hpp kNodeGroups

// primary.cpp grown_box for element i of a pair-SoA table, with c - o in place of c.
__device__ void grown_box(const float* table, uint32_t i, double Q, const double* o, double* out) {
    const float* t = table + static_cast<size_t>(i / 2u) * 16u;
    const uint32_t e = i % 2u;
    const double K = t[12 + e];
    const double g = K * Q * (1.0 + 1e-6) + kExtra;
    for (int a = 0; a < 3; a++) {
        const double lo = t[2 * a + e], hi = t[6 + 2 * a + e];
        const double c = 0.5 * (lo + hi);
        out[a] = c - o[a];
        out[3 + a] = 0.5 * (hi - lo) + g;
    }
    out[6] = !(g < 1e30) ? 1.0 : 0.0;  // K = inf: never ruled out
    out[7] = 0.0;
}

struct Pyramid {
    double n[4][3];  // inward side-plane normals
    double len[4];   // sqrt(n . n)
};

// primary.cpp QuarterWalker::pyramid
__device__ Pyramid make_pyramid(const CameraListParams& p, uint32_t e) {
    const uint32_t lt = e >> 2, qx = e & 1u, qy = (e >> 1) & 1u;
    uint32_t tx, ty;
    vcrt::tile_of(lt, p.rank, p.world, p.tiles_x, &tx, &ty);
    const double x0 = 8.0 * tx + 4.0 * qx, y0 = 8.0 * ty + 4.0 * qy;
    const double X0 = x0 - 0.5 - p.ex, X1 = x0 + 3.5 + p.ex;
    const double Y0 = y0 - 0.5 - p.ey, Y1 = y0 + 3.5 + p.ey;
    const double XY[4][2] = {{X0, Y0}, {X1, Y0}, {X1, Y1}, {X0, Y1}};
    double D[4][3], mid[3] = {0, 0, 0};
    for (int k = 0; k < 4; k++)
        for (int a = 0; a < 3; a++) {
            D[k][a] = p.cam[a] + XY[k][0] * p.cam[3 + a] + XY[k][1] * p.cam[6 + a] - p.cam[9 + a];
            mid[a] += 0.25 * D[k][a];
        }
    Pyramid P;
    for (int k = 0; k < 4; k++) {
        const double* u = D[k];
        const double* v = D[(k + 1) % 4];
        const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2],
                             u[0] * v[1] - u[1] * v[0]};
        const double s = n[0] * mid[0] + n[1] * mid[1] + n[2] * mid[2];
        double nn = 0.0;
        for (int a = 0; a < 3; a++) {
            P.n[k][a] = s < 0.0 ? -n[a] : n[a];
            nn += P.n[k][a] * P.n[k][a];
        }
        P.len[k] = sqrt(nn);
    }
    return P;
}

// primary.cpp outside(): a side plane separates the grown box from the pyramid
__device__ bool box_outside(const Pyramid& P, const double* b) {
    if (b[6] != 0.0) return false;
    for (int k = 0; k < 4; k++) {
        double s = 0.0, r = 0.0;
        for (int a = 0; a < 3; a++) {
            s += P.n[k][a] * b[a];
            r += fabs(P.n[k][a]) * b[3 + a];
        }
        if (s + r < 0.0) return true;
    }
    return false;
}

// primary.cpp sphere_outside() with R = r + M_s + 1e-3
__device__ bool sphere_outside(const Pyramid& P, const double* sp) {
    for (int k = 0; k < 4; k++) {
        double s = 0.0;
        for (int a = 0; a < 3; a++) s += P.n[k][a] * sp[a];
        if (s + P.len[k] * sp[3] < 0.0) return true;
    }
    return false;
}

// Member m of a quarter's sphere list into its pair record (primary.cpp, pair_disc_cc's fp32
// operations and order). The first of a pair also writes the pad an odd list ends with.
__device__ void write_member(const CameraListParams& p, float* rec, uint32_t m, int32_t j) {
    // (bit patterns through one integer type: the indices are not floats)
    uint32_t* r = reinterpret_cast<uint32_t*>(rec) + static_cast<size_t>(m / 2u) * 12u;
    const uint32_t e2 = m & 1u;
    const float* sp = p.center_radius + static_cast<size_t>(j) * 4u;
    const float ocx = p.o[0] - sp[0], ocy = p.o[1] - sp[1], ocz = p.o[2] - sp[2];
    const float r2 = sp[3] * sp[3];
    if (e2 == 0u) {
        r[1] = r[3] = r[5] = 0u;
        r[7] = __float_as_uint(3.0e38f);
        r[9] = 0xFFFFFFFFu;  // index -1
        r[10] = r[11] = 0u;
    }
    r[0 + e2] = __float_as_uint(ocx);
    r[2 + e2] = __float_as_uint(ocy);
    r[4 + e2] = __float_as_uint(ocz);
    r[6 + e2] = __float_as_uint(((ocx * ocx + ocy * ocy) + ocz * ocz) - r2);
    r[8 + e2] = static_cast<uint32_t>(j);
}

// The walk of quarter e. Counting: *groups and *members receive the quarter's counts
// (kCamListNone: no list). Filling: want_ids / want_rec say which lists the quarter has; ids and
// rec point at its first id and first pair record.
template <bool kFill>
__device__ void walk(const CameraListParams& p, uint32_t e, uint32_t* groups, uint32_t* members,
                     bool want_ids, bool want_rec, uint16_t* ids, float* rec) {
    const Pyramid P = make_pyramid(p, e);
    const double* gbox = p.boxes;
    const double* nbox = gbox + static_cast<size_t>(p.ngroups) * kCamListBox;
    const double* tbox = nbox + static_cast<size_t>(p.nnodes) * kCamListBox;
    uint32_t nf = 0, nm = 0;
    bool over = false, many = false;
    for (uint32_t ci = 0; ci < p.ntops && !many; ci++) {
        if (box_outside(P, tbox + static_cast<size_t>(ci) * kCamListBox)) continue;
        const uint32_t n_end = min(p.nnodes, ci * 8u + 8u);
        for (uint32_t ni = ci * 8u; ni < n_end && !many; ni++) {
            if (box_outside(P, nbox + static_cast<size_t>(ni) * kCamListBox)) continue;
            for (uint32_t gi = ni * kNodeGroups; gi < ni * kNodeGroups + kNodeGroups; gi++) {
                const double* b = gbox + static_cast<size_t>(gi) * kCamListBox;
                if (b[7] == 0.0 || box_outside(P, b)) continue;
                if (nf == kWalkCap) {  // the 65th group: neither list
                    many = true;
                    break;
                }
                if (kFill && want_ids && nf < kGroupCap) ids[nf] = static_cast<uint16_t>(gi);
                nf++;
                if (kFill ? !want_rec : over) {
                    // no sphere list: past the group list's cap nothing is left to find out
                    if (nf > kGroupCap) {
                        many = true;
                        break;
                    }
                    continue;
                }
                const int32_t* idx = reinterpret_cast<const int32_t*>(p.cgroup) +
                                     static_cast<size_t>(p.nbig + gi) * 20u + 16u;
                for (int k = 0; k < 4 && !over; k++) {
                    const int32_t j = idx[k];
                    if (j < 0 || static_cast<uint32_t>(j) >= p.nspheres) continue;
                    const double* sp = p.spheres + static_cast<size_t>(j) * kCamListBox;
                    if (sp[4] != 0.0 || !sphere_outside(P, sp)) {
                        if (nm == kSphereCap) {
                            over = true;
                        } else {
                            if (kFill) write_member(p, rec, nm, j);
                            nm++;
                        }
                    }
                }
            }
        }
    }
    if (!kFill) {
        *groups = (nf <= kGroupCap && !many && p.ids_ok != 0u) ? nf : kCamListNone;
        *members = (!many && !over && nf <= kWalkCap) ? nm : kCamListNone;
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void vcrt_camlist_prepare(CameraListParams p) {
    const uint32_t nbox = p.ngroups + p.nnodes + p.ntops;
    const uint32_t total = nbox + p.nspheres;
    const double o[3] = {p.cam[9], p.cam[10], p.cam[11]};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gridDim.x * blockDim.x) {
        if (i < nbox) {
            double* out = p.boxes + static_cast<size_t>(i) * kCamListBox;
            if (i < p.ngroups) {
                grown_box(p.cbound, i, p.Q, o, out);
                const int32_t* idx = reinterpret_cast<const int32_t*>(p.cgroup) +
                                     static_cast<size_t>(p.nbig + i) * 20u + 16u;
                bool real = false;
                for (int k = 0; k < 4; k++) real = real || idx[k] >= 0;
                out[7] = real ? 1.0 : 0.0;
            } else if (i < p.ngroups + p.nnodes) {
                grown_box(p.cnode, i - p.ngroups, p.Q, o, out);
            } else {
                grown_box(p.ctop, i - p.ngroups - p.nnodes, p.Q, o, out);
            }
        } else {
            // build_primary_sphere_lists: the member's own margin and the rounding of the rays
            const uint32_t j = i - nbox;
            const float* sp = p.center_radius + static_cast<size_t>(j) * 4u;
            const double c[3] = {sp[0], sp[1], sp[2]};
            const double r = fabs(static_cast<double>(sp[3]));
            double oc2 = 0.0;
            for (int a = 0; a < 3; a++) oc2 += (o[a] - c[a]) * (o[a] - c[a]);
            const double Ms = r > 0.0 ? 8.1 * 0x1p-24 * (oc2 + r * r) / r * (1.0 + 1e-5)
                                      : __builtin_inf();
            double* out = p.spheres + static_cast<size_t>(j) * kCamListBox;
            for (int a = 0; a < 3; a++) out[a] = c[a] - o[a];
            out[3] = r + Ms + kExtra;
            out[4] = !(Ms < 1e30) ? 1.0 : 0.0;
            out[5] = out[6] = out[7] = 0.0;
        }
    }
}

extern "C" __global__ __launch_bounds__(256) void vcrt_camlist_count(CameraListParams p) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.n) return;
    uint32_t groups, members;
    walk<false>(p, e, &groups, &members, false, false, nullptr, nullptr);
    p.counts[2u * e] = groups;
    p.counts[2u * e + 1u] = members;
}

// One workgroup. Thread t sums a contiguous run of quarters, the runs' sums are scanned in LDS,
// and the thread then hands out its run's offsets: entry order throughout.
extern "C" __global__ __launch_bounds__(vcrt::kCamListScanThreads) void vcrt_camlist_scan(
    CameraListParams p) {
    __shared__ uint32_t sums[2][vcrt::kCamListScanThreads];
    const uint32_t t = threadIdx.x, nt = vcrt::kCamListScanThreads;
    const uint32_t per = (p.n + nt - 1u) / nt;
    const uint32_t b = min(p.n, t * per), e_end = min(p.n, b + per);
    uint32_t ids = 0, pairs = 0;
    for (uint32_t e = b; e < e_end; e++) {
        const uint32_t cg = p.counts[2u * e], cs = p.counts[2u * e + 1u];
        if (cg != kCamListNone) ids += cg;
        if (cs != kCamListNone) pairs += (cs + 1u) / 2u;
    }
    sums[0][t] = ids;
    sums[1][t] = pairs;
    __syncthreads();
    for (uint32_t d = 1; d < nt; d <<= 1) {  // inclusive scan over the threads
        const uint32_t a0 = t >= d ? sums[0][t - d] : 0u, a1 = t >= d ? sums[1][t - d] : 0u;
        __syncthreads();
        sums[0][t] += a0;
        sums[1][t] += a1;
        __syncthreads();
    }
    uint32_t off_ids = sums[0][t] - ids, off_pairs = sums[1][t] - pairs;
    for (uint32_t e = b; e < e_end; e++) {
        const uint32_t cg = p.counts[2u * e], cs = p.counts[2u * e + 1u];
        p.offsets[2u * e] = off_ids;
        p.offsets[2u * e + 1u] = off_pairs;
        if (cg != kCamListNone) off_ids += cg;
        if (cs != kCamListNone) off_pairs += (cs + 1u) / 2u;
    }
    if (t == nt - 1u) {
        p.totals[0] = sums[0][t];
        p.totals[1] = sums[1][t];
    }
}

extern "C" __global__ __launch_bounds__(256) void vcrt_camlist_fill(CameraListParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float* rec = p.cam_rec + static_cast<size_t>(p.nbig) * 16u;
    if (i < p.nbig) {
        // build_camera_records for big group i
        const float* g = p.cgroup + static_cast<size_t>(i) * 20u;
        float* c = p.cam_rec + static_cast<size_t>(i) * 16u;
        for (int pair = 0; pair < 2; pair++)
            for (int e = 0; e < 2; e++) {
                const float* q = g + 8 * pair;
                float* w = c + 8 * pair;
                const float ocx = p.o[0] - q[0 + e], ocy = p.o[1] - q[2 + e],
                            ocz = p.o[2] - q[4 + e];
                const float cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - q[6 + e];
                w[0 + e] = ocx;
                w[2 + e] = ocy;
                w[4 + e] = ocz;
                w[6 + e] = cc;
            }
    }
    if (i < 12u) rec[static_cast<size_t>(p.totals[1]) * 12u + i] = 0.0f;  // never empty
    if (i >= p.n) return;
    const uint32_t cg = p.counts[2u * i], cs = p.counts[2u * i + 1u];
    const uint32_t og = p.offsets[2u * i], os = p.offsets[2u * i + 1u];
    // offsets are 28-bit: beyond that a quarter keeps no list (its ids and records stay)
    p.prim_info[2u * i] =
        cg == kCamListNone || og + cg >= (1u << 28) ? kInfoNone : og << 4 | cg;
    p.prim_info[2u * i + 1u] = cs == kCamListNone || os >= (1u << 28) ? kInfoNone : os << 4 | cs;
    if (cg == kCamListNone && cs == kCamListNone) return;
    walk<true>(p, i, nullptr, nullptr, cg != kCamListNone, cs != kCamListNone, p.prim_ids + og,
               rec + static_cast<size_t>(os) * 12u);
}
