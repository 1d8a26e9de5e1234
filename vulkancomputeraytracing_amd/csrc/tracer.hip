// tracer.hip -- the hot path: per-pixel ray generation -> sphere-list intersection ->
// Lambertian / metal / glass scatter -> multi-bounce radiance accumulation, written for
// gfx950 (CDNA4, wave64) as a persistent-lanes wavefront tracer.
//
// Reference semantics (quirks kept):
//   shaders/shader.comp:16-58            camera ray per sample, accumulate, divide, store
//   shaders/include/functions.glsl:14-40 hit_sphere (strict <, index-order tie break)
//   shaders/include/functions.glsl:65-92 ray_color bounce loop, sky on miss
//   shaders/include/textures.glsl:19-71  lambertian / metal / glass scatter
//
// MI355X design:
//   * Work items are (pixel, chunk of K samples): a block of 64 items holds all the chunks of a
//     few pixels of one 8x8 tile (chunk-minor), and a wave takes a whole block with one atomic on
//     its XCD's work queue and hands its items to lanes as they free up; a lane whose path ends
//     starts its next sample at once (path regeneration). A lane sums its samples in fp32 in
//     quanta of G (vcrt_math.h "Accumulation"); each quantum sum, quantized by the scene's scale
//     2^s, is added exactly to the pixel's sums (LDS atomics into the wave's accumulation ring,
//     flushed to global memory per pixel) and vcrt_resolve divides: the image depends on G and s
//     only, not on the work items, the schedule or the number of GPUs. One quantum per pixel:
//     the lane writes the pixel.
//   * Ray state lives in VGPRs. Sphere tests run two spheres per packed-fp32 instruction
//     (v_pk_add_f32 / v_pk_mul_f32 on pair-SoA groups of four: 2 lane-ops per issue, the only
//     way gfx950 reaches its fp32 peak).
//   * The sphere-list scan is either the reference's linear scan (wave-uniform groups through
//     the scalar cache or LDS) or an exact culled scan over a spatial hierarchy (groups of 4,
//     nodes of 8 groups, chunks of 64 groups), wave-uniform or per lane on an LDS copy of the
//     tables; see "Culled scan" below for why it returns the same sphere and t. In the flat
//     culled scan a camera ray starts from its pixel quarter's precomputed group list
//     (csrc/primary.cpp) instead of the hierarchy.
//   * Only fp32 add/sub/mul plus correctly rounded div/sqrt, no contraction, in everything
//     that reaches the image: results are bit-identical to the CPU oracle for the same
//     accumulation order. No MFMA.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vcrt_kernel_abi.h"
#include "vcrt_math.h"

#pragma clang fp contract(off)

using namespace vcrt;

// A/B builds: 1 makes the boxes-in-LDS flat kernel branch on the slab flag once per segment (the
// scan instantiated twice, as the LDS-table kernel does) instead of around each run of four box
// pairs; one more SGPR spill than the parent's, see trace_impl (profiles/r07_ab_log.md).
#ifndef VCRT_SLAB_BOXES_SCAN
#define VCRT_SLAB_BOXES_SCAN 0
#endif

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Issued-work tallies (TraceParams.work_done): a wave-uniform count x is credited to the wave's
// first active lane, so the sum over the lanes is the wave's total. (A per-wave 64-bit counter
// is per lane under SIMT all the same -- lanes that skip a region keep their old value -- and
// lived in VGPR pairs that spilled, with a full vmcnt wait at every update.)
__device__ __forceinline__ void tally(uint32_t& t, uint32_t x) {
    const uint32_t first = (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec());
    t += (threadIdx.x & 63u) == first ? x : 0u;
}

// tally into a per-wave LDS counter (the flat scans' WaveScratch::work): one LDS add from the
// first active lane, nothing held in VGPRs across the loop
__device__ __forceinline__ void tally_lds(uint32_t* slot, uint32_t x) {
    const uint32_t first = (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec());
    if ((threadIdx.x & 63u) == first) atomicAdd(slot, x);
}

// Region counters of the stats builds (tools/valu_attrib.py): one global atomic by the wave's
// first active lane into the wave's own row of TraceParams.region ([waves][kRegions]) each time
// the wave enters a counted region with some lane active. The product kernels pass a null row,
// which folds every call away.
namespace reg {
enum : uint32_t {
    kIter = 0, kRetire, kRetireNan, kRetireRing, kRetireGlobal, kNewRay, kFetchTrip, kBlock,
    kBlockRing, kItem, kCam, kCamBig, kCamBigM0, kCamBigM1, kCamBigM2, kCamBigM3, kCamListTrip,
    kCamRootTrip, kShadeCam, kScan, kScanLinear, kMainBig, kMainBigM0, kMainBigM1, kMainBigM2,
    kMainBigM3, kListed, kLevelChunk, kLevelNodes, kDrainTrip, kPassCand, kPassGroup, kPassNode,
    kPassChunk, kShadeSkyMain, kSqrtFallback, kDivFallback, kSteal,
    kUnitFallback,  // unit_of's full division (a scatter vector outside its guard)
    kShadeBase0 = 40, kShadeBase1 = 56,  // the shading's regions, per call site (camera phase,
                                         // main-scan sky), at these offsets:
    kShEntry = 0, kShHit, kShNormalDiv, kShSinFallback, kShLamMetal, kShLam, kShMetal, kShGlass,
    kShGlassIn, kShGlassOut, kShGlassRefract, kShSky, kShEnded, kShNewRay, kShItemEnd,
    // sub-blocks of the flat scan's regions that run only on some of their entries
    kPrefixSlow = 72, kLevelTop, kPushNode, kPushGroup, kPushLevel, kListedTrip,
    // the group-footprint level (fact (5g)): entries, push trips, slices of the rare sliced push
    kLevelGroups, kPushGroups0, kPushGroups1, kPushGroups2, kPushGroups3, kSliceGroups, kPushSlice,
    kPushHeavy,  // the level's heavy-lane loop: one per lane whose groups the wave deals out
    kGroupPass2,  // a group pass that took a second entry per lane (flat_group_pass2)
    kCount = 88
};
}  // namespace reg
constexpr uint32_t kRegions = 88;  // the host's row size (vcrt_kernel_abi.h TraceParams.region)

__device__ __forceinline__ void region(uint32_t* row, uint32_t k) {
    if (row) {
        const uint32_t first = (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec());
        if ((threadIdx.x & 63u) == first) atomicAdd(row + k, 1u);
    }
}

typedef __attribute__((address_space(4))) const float4 cfloat4;

// A 32-bit constant materialized in a VGPR where it is used: the asm is volatile, so it is not
// hoisted out of the persistent loop. Left to itself the compiler keeps constant pairs such as a
// scan's initial (max_t, best) = (kInfinity, -1) live across the loop, and under the flat
// kernel's register pressure spills them to scratch: a scratch load and a vmcnt wait per use.
static_assert(__builtin_bit_cast(uint32_t, kInfinity) == 0x47c35000u, "vconst<kInfinity bits>");
template <uint32_t kC>
__device__ __forceinline__ uint32_t vconst() {
    uint32_t r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "i"(kC));
    return r;
}

// One group = four spheres in pair-SoA form: q[0] = (cx0,cx1,cy0,cy1), q[1] = (cz0,cz1,r0²,r1²),
// q[2] = (cx2,cx3,cy2,cy3), q[3] = (cz2,cz3,r2²,r3²).
struct Group {
    float4 q[4];
};

template <bool kLds>
__device__ __forceinline__ Group load_group(const float4* lds, const TraceParams& p, int gi) {
    Group g;
    if constexpr (kLds) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g.q[k] = lds[4 * gi + k];
    } else {
        cfloat4* s = (cfloat4*)p.geom;  // wave-uniform index -> s_load through the scalar cache
#pragma unroll
        for (int k = 0; k < 4; ++k) g.q[k] = s[4 * gi + k];
    }
    return g;
}

// hit_sphere (functions.glsl:14-40) after the discriminant test passed: nearest root in
// (min_t, max_t), strict comparisons, max_t shrinks on acceptance.
__device__ __forceinline__ void accept_root(float hb, float disc, float a, float& max_t, int& best,
                                            int j) {
    const float min_t = kMinT;
    const float sq = __builtin_sqrtf(disc);
    float root = (-hb - sq) / a;
    bool ok = true;
    if (root <= min_t || max_t <= root) {
        root = (-hb + sq) / a;
        ok = !(root <= min_t || max_t <= root);
    }
    if (ok) {
        max_t = root;
        best = j;
    }
}

// Conservative pre-filter for the root path: false only when hit_sphere would certainly reject
// the sphere, decided without the correctly rounded sqrt/divisions.
//   sq_hi >= RN(sqrt(disc)): hardware v_sqrt_f32 (~1 ulp) plus 4 ulp;
//   x1_lo = RN(-hb - sq_hi) <= x1 and x2_hi = RN(-hb + sq_hi) >= x2 (rounding is monotone);
//   "beyond": x1_lo - max_t*a >= 0 (the sign of the fused fma is exact: every operand is a
//   multiple of >= 2^-76 in the guarded ranges, so nothing underflows) => x1/a >= max_t =>
//   root1 = RN(x1/a) >= max_t and root2 >= root1: both rejected;
//   "behind": x2_hi - min_t*a <= 0 => root2 <= min_t and root1 <= root2: both rejected.
// Outside the guarded ranges (tiny/huge/NaN values) it answers true and the exact path decides.
__device__ __forceinline__ bool may_accept(float hb, float disc, float a, float max_t,
                                           bool ray_ok) {
    const float min_t = kMinT;
    const bool ok = ray_ok && disc >= 0x1p-100f && disc <= 0x1p100f && hb >= -0x1p60f &&
                    hb <= 0x1p60f;
    const float sq_hi = __uint_as_float(__float_as_uint(__builtin_amdgcn_sqrtf(disc)) + 4u);
    const float x1_lo = -hb - sq_hi;
    const float x2_hi = -hb + sq_hi;
    const bool beyond = __builtin_fmaf(-max_t, a, x1_lo) >= 0.0f;
    const bool behind = __builtin_fmaf(-min_t, a, x2_hi) <= 0.0f;
    return !ok || !(beyond || behind);
}

// Discriminants of two spheres at once (hit_sphere's first half, element-wise exact):
// oc = o - c; half_b = dot(oc, d); c = dot(oc, oc) - r²; disc = half_b² - a·c.
__device__ __forceinline__ void pair_disc(const v2f ox, const v2f oy, const v2f oz, const v2f dx,
                                          const v2f dy, const v2f dz, const v2f a2, float4 xy,
                                          float4 zr, v2f& hb, v2f& disc) {
    const v2f cx = {xy.x, xy.y}, cy = {xy.z, xy.w}, cz = {zr.x, zr.y}, r2 = {zr.z, zr.w};
    const v2f ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;
    hb = ocx * dx + ocy * dy + ocz * dz;
    const v2f cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
    disc = hb * hb - a2 * cc;
}

// The sphere-list scan of one ray segment (functions.glsl:77-81): four spheres per step as two
// packed pairs, the next group prefetched, one wave-uniform branch into the rare root path,
// which then visits the four candidates in index order so ties resolve to the earlier sphere.
template <bool kLds>
__device__ __forceinline__ void scan_spheres(const TraceParams& p, const float4* lds, int n,
                                             const f3 o, const f3 d, float& max_t, int& best,
                                             uint32_t& hit_groups) {
    const float a = dot(d, d);  // loop-invariant in hit_sphere: hoisting is exact
    // the pre-filter's guarded range: a in [2^-20, 2^60] (and not NaN)
    const bool ray_ok = a >= 0x1p-20f && a <= 0x1p60f;
    // |o| <= 2^30 and a <= 2^60 (|d| <= 2^30) with the host-checked scene bound |c|, r <= 2^30
    // keep every discriminant finite (hb^2, a*c < 2^127): no NaN can reach the max test
    const bool finite_ok = (p.flags & kFlagSceneBounded) != 0 && a <= 0x1p60f &&
                           fabsf(o.x) <= 0x1p30f && fabsf(o.y) <= 0x1p30f &&
                           fabsf(o.z) <= 0x1p30f;
    const uint64_t unguarded = __ballot(!finite_ok);
    const v2f ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
    const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {a, a};
    const int ngroups = (n + 3) >> 2;
    Group g = load_group<kLds>(lds, p, 0);
    for (int gi = 0; gi < ngroups; ++gi) {
        const Group nx = load_group<kLds>(lds, p, gi + 1);  // table padded by one group
        v2f hb01, d01, hb23, d23;
        pair_disc(ox, oy, oz, dx, dy, dz, a2, g.q[0], g.q[1], hb01, d01);
        pair_disc(ox, oy, oz, dx, dy, dz, a2, g.q[2], g.q[3], hb23, d23);
        // Any of the four not negative? For finite discriminants this is !(max < 0): one
        // v_max3 + v_max + compare instead of four compares. Lanes whose ray is outside the
        // guarded range (where a discriminant could be NaN, which max would drop) always take
        // the exact per-sphere test below.
        const float m4 = fmaxf(fmaxf(d01.x, d01.y), fmaxf(d23.x, d23.y));
        if (__ballot(!(m4 < 0.0f)) | unguarded) {
            const bool h0 = !(d01.x < 0.0f), h1 = !(d01.y < 0.0f), h2 = !(d23.x < 0.0f),
                       h3 = !(d23.y < 0.0f);
            ++hit_groups;
            const int j = 4 * gi;  // padding spheres (index >= n) are never accepted
            // pre-filter against the max_t at group entry: a rejection stays valid as max_t
            // only shrinks; survivors go through hit_sphere's exact logic in index order
            const float mt = max_t;
            const bool e0 = h0 && may_accept(hb01.x, d01.x, a, mt, ray_ok);
            const bool e1 = h1 && j + 1 < n && may_accept(hb01.y, d01.y, a, mt, ray_ok);
            const bool e2 = h2 && j + 2 < n && may_accept(hb23.x, d23.x, a, mt, ray_ok);
            const bool e3 = h3 && j + 3 < n && may_accept(hb23.y, d23.y, a, mt, ray_ok);
            if (__ballot(e0) | __ballot(e1) | __ballot(e2) | __ballot(e3)) {
                if (e0) accept_root(hb01.x, d01.x, a, max_t, best, j + 0);
                if (e1) accept_root(hb01.y, d01.y, a, max_t, best, j + 1);
                if (e2) accept_root(hb23.x, d23.x, a, max_t, best, j + 2);
                if (e3) accept_root(hb23.y, d23.y, a, max_t, best, j + 3);
            }
        }
        g = nx;
    }
}

// ---------------------------------------------------------------------------------------------
// Culled scan (variant CULL). Exact for waves whose rays are all in the guarded finite range
// (|o| <= 2^30, a in [2^-20, 2^60], scene bounded), by two facts:
//  (1) hit_sphere's sequential scan with strict < (functions.glsl:27-29,77-81) selects the
//      candidate with the smallest t, earliest index on ties, where t = root1 if root1 > min_t
//      else root2, kept if min_t < t < max_t -- so spheres may be visited in any order;
//  (2) a margin. With u = 2^-24, disc_f >= 0 (pair_disc's rounded oc, hb, cc, products and
//      difference) implies that the ray line passes within r + M_s of the centre,
//      M_s = 8.1u (|oc|^2 + r^2) / r: the roundings move hb^2 - a*cc by at most ~15u a |oc|^2
//      and the rounded oc moves the centre by u |oc|. For a bound (C, R) of members with
//      box's members (radius >= r_b, all |c| <= c_max, r <= r_max) M_s <= M_b = K_b Q with
//      K_b = 8.1u / r_b and Q = (|o| + c_max)^2 + r_max^2.
//  (3) the box test. Group, node and chunk bounds are axis-aligned boxes B = [lo, hi] of their
//      members (rounded outwards) with their K_b. Per axis the lane computes the plane
//      parameters fma(lo, inv, c), fma(hi, inv, c) with inv = v_rcp(d') (1 ulp), c = -o inv,
//      d' = d with components below 2^-40 raised to 2^-40; tnear = max of the per-axis minima,
//      tfar = min of the maxima, and rules B out when
//        gap = fma(K_b, c2, (tfar - tnear) + c1) < 0,
//        c1 = 1.001 J 5.1u (L + |o|_inf),  c2 = 1.001 J Q,  J = 2 max_i |inv_i|,
//      L = max |box coordinate|. Why: if the real line met B grown by M_b at t*, every exact
//      per-axis interval of B would reach within (M_b + dc) / |d'_i| of t*, where dc <=
//      sqrt(3) 2^-30 (L + M_b + |o|_inf) bounds the shift from d to d' (a >= 2^-20); each
//      computed end lies within 4.02u (L + |o_i|) / |d'_i| of its exact value (rcp 2u, two
//      roundings); and 1 / |d'_i| <= (1 + 2.01u) J / 2. So tfar - tnear >= -(M_b + dc + 4.02u
//      (L + |o|_inf)) (1 + 2.01u) J, which c1 + K_b c2 exceeds by more than the last three
//      roundings: gap >= 0, the box is kept. Hence a ruled-out box holds no member with
//      disc_f >= 0. (Q and the 1.001 factors absorb the per-ray roundings; K_b = inf, a zero
//      radius, keeps its box.) The host passes K_b, c_max, r_max^2 and L rounded up.
//  (4) behind the origin. A member is accepted only if hb_f < 0 or cc_f < 0 (may_hit). If the
//      line meets the member's sphere grown by M_s only at t < -tau (or not at all), with
//      tau^2 = 5.02u Q / a, then exactly hb = -a t_c > a tau >= 4.02u |oc| |d| (t_c: the
//      centre's parameter) and cc = |oc|^2 - r^2 > a tau^2 >= 5.02u (|oc|^2 + r^2), which
//      the roundings of hb_f (4.02u |oc| |d|: oc and the dot) and of cc_f (5.02u |oc|^2 and u r^2)
//      cannot flip: hb_f >= 0 and cc_f >= 0, rejected. So an accepted member's grown sphere,
//      inside the grown box, meets the line at some t* >= -tau, and the computed far end is at
//      least t* - (c1 + K_b c2) / 2 by (3). The kernels shift every plane by tau (c = fma(-o,
//      inv, tau): t' = t + tau, gaps unchanged; the shift's roundings, below 4.1u tau, fit in
//      c1's spare) and clamp the near end at 0: gap = fma(K_b, c2, (tf' - max(tn', 0)) + c1)
//      rules a box out when its whole stretch of the line lies behind -tau as well.
//      (tau = sqrt(3.2e-7 Q / a), 7% above 5.02u Q / a for the roundings of Q, 1/a and sqrt.)
//  (3a) the shared slab (flat scans, kFlagSlab). When every group, node and chunk box that has
//      members carries the same lo.y and hi.y, bit for bit (host-checked, TraceParams.slab: the
//      generated scenes, whose hierarchy spheres all sit at one height with one radius), the two
//      y-plane terms fma(lo.y, inv.y, c.y), fma(hi.y, inv.y, c.y) have the same operands in every
//      box test of a ray, so they are the same two fp32 numbers: box_ray computes them once,
//      t0 = max(min of the two, 0) and t1 = max of the two, and each box test takes tnear =
//      max3(x near, z near, t0), tfar = min3(x far, z far, t1). max and min of these values (finite
//      or +inf, never NaN) are exact, associative and commutative, so max3(tnx, tnz, max(tny, 0)) =
//      max(max3(tnx, tny, tnz), 0): the gap is the three-axis gap of (3) and (4), the same boxes
//      are ruled out, and the image, the segments and the issued tests do not change. A padding
//      box (the far point 1e20, no member a ray can accept) gets the slab in place of its own y
//      planes, so its gap may differ: it is ruled out by x and z as before, or its empty groups
//      are tested for nothing.
//  (5) the footprint (the LDS-table flat scan's node level, foot_mask; cluster.hpp fp_tab). If
//      the box test of (3), (3a), (4) keeps node k for a ray (gap >= 0), bit k of the ray's mask
//      is set; so (2)-(4) carry over and only the issued tests change. Let t0, t1 be the ray's y
//      interval over [Ylo, Yhi], the y extent of all node boxes with members, computed as (3a)
//      does (on a slab scene they are (3a)'s own numbers, the operands being bit-equal; otherwise
//      Ylo <= lo.y and hi.y <= Yhi and fma(., inv, c) is monotone in its first operand, so t0 <=
//      the box's clamped near y term and t1 >= its far one). With tn, tf the test's near and far
//      end, t0 <= tn and tf <= t1. gap >= 0 means RN(K c2 + RN(RN(tf - tn) + c1)) >= 0, hence tf
//      - tn >= -E, E = 1.001 (c1 + K c2) (three roundings of relative u and flushes below 2^-123,
//      against c1 >= 2^-71: the host requires L >= 2^-20). So for x (and the same for z), with
//      tnx, tfx the computed near and far plane terms: tnx <= tn <= tf + E <= t1 + E and tfx >=
//      tf >= tn - E >= t0 - E. The kernel takes S = RN(RN(2 c1) + (2 Kmax) c2) >= 1.99 (c1 + K
//      c2) for every finite K (K = +inf: the node is in `always`), ta = RN(t0 - S), tb = RN(t1 +
//      S). |t0|, |t1| <= 1.001 (J / 2) (L + |o|_inf) + tau, so rounding ta and tb costs at most
//      0.1 c1 + u tau, within c1's spare as the shift of (4): ta < t0 - E and t1 + E < tb, i.e.
//      tnx < tb and tfx > ta, strictly. If tb < ta then t0 - t1 > E and no box is kept: the mask
//      is `always`. Otherwise let p = RN(t - cx), X(t) = RN(p d'x) for t = ta, tb: with ix =
//      (1 + e) / d'x, |e| <= 2u, X(t) ix + cx = t + (t - cx) th, |th| <= 4.01u, so Xu(t) = X(t) +
//      8u |X(t)| and Xd(t) = X(t) - 8u |X(t)| satisfy fma(Xu(tb), ix, cx) >= tb and fma(Xd(ta),
//      ix, cx) <= ta for ix > 0 (for ix < 0 with ta and tb exchanged); an underflowing product
//      moves X by at most 2^-126, the host's 2^-100. For ix > 0 the near plane is lo.x: fma(lo.x,
//      ix, cx) = tnx < tb <= fma(Xu(tb), ix, cx) gives lo.x < Xu(tb) by monotonicity, and
//      likewise hi.x > Xd(ta); for ix < 0 the planes swap and lo.x < Xu(ta), hi.x > Xd(tb). X(ta)
//      and X(tb) are ordered by the sign of d'x (RN is monotone), so with Xlo, Xhi the smaller and
//      larger of the two: lo.x <= Xhi + 8u |Xhi| and hi.x >= Xlo - 8u |Xlo|. The cell function
//      cell(X) = trunc(med3(fma(X, scale, offset), 0, N - 1)) never falls as X rises, so cell(Xhi)
//      is the larger cell, and the host, which finds each cell's largest float ue and smallest
//      float le with the same function and sets A[i] = {k: lo.x <= ue + 8u |ue| + 2^-100}, B[i] =
//      {k: hi.x >= le - 8u |le| - 2^-100} (X + 8u |X| is monotone; the end cells reach +-inf),
//      has bit k in A[cell(Xhi)] and B[cell(Xlo)]. The mask is the AND of the four lookups, OR
//      `always`. All of ta, tb, p are finite or, when K c2 overflows, ta = -inf and tb = +inf: no
//      inf - inf (t0, t1, cx finite), no 0 x inf (d'x != 0, scale > 0), and med3 clamps +-inf.
//      The node pass then runs the exact line test (3) on each group box, so a node entered for
//      nothing costs eight group-box tests and pushes what the line test lets through.
//  (5g) the group footprint (the LDS-table flat scan with kFlagGroupFoot, group_foot_mask;
//      cluster.hpp gf_tab). (5) word for word with the group boxes in place of the node boxes: if
//      the box test of (3), (3a), (4) keeps group g for a ray (gap >= 0), bit g of the ray's
//      128-bit mask is set. The cells, the cell function (over gf_n cells), ta, tb and the slack
//      rule are (5)'s; S = RN(RN(2 c1) + (2 Kmax) c2) takes Kmax over the group boxes' own finite
//      K (a larger S is only more conservative), groups with K = +inf are in `always`, padding
//      groups never get a bit, and [Ylo, Yhi] is the one y extent that every group box with
//      members has, bit for bit (the host's condition; it is fp_y, and the slab's on a slab
//      scene), so t0, t1 are the box test's own y terms. By (2)-(4) a group whose box the test
//      rules out holds no member that the exact test accepts, so the mask's groups include every
//      group with such a member; a surplus group entry runs the exact four-sphere test for
//      nothing and changes only the issued tests. The scan pushes the mask's groups straight onto
//      the group stack: no node entry, no node pass, no box test (bound_tests counts none).
//      The host sets the flag only for at most 128 hierarchy groups, one height, and a frame
//      whose camera rays have their lists: those rays cross the scene on long grazing stretches,
//      where the xz rectangle of the tables is much looser than the line test.
//  (6) any hit (occlusion queries, occlude_culled_lane). The question "does hit_sphere accept
//      some sphere with min_t and a fixed max_t = T" is an OR over the spheres, each term a
//      function of that sphere and the ray alone (max_t never shrinks), so the visiting order and
//      the point at which a lane stops do not matter. (2)-(4) do not involve max_t: a box that is
//      ruled out holds no member with disc_f >= 0 and (hb_f < 0 or cc_f < 0), hence none that
//      hit_sphere could accept for any T, +inf included. For a member that passes may_hit,
//      hit_sphere takes root1 = RN((-hb - sq) / a) unless root1 <= min_t or T <= root1, then
//      root2 = RN((-hb + sq) / a) under the same test. sq >= 0 and a > 0, and rounding is
//      monotone, so root2 >= root1: a root1 rejected for T <= root1 (and not for root1 <= min_t)
//      leaves T <= root2, rejected too. So the member is accepted exactly when t = candidate_t
//      (root1 if root1 > min_t, else root2) satisfies min_t < t < T.
// Waves holding a ray outside the guarded range scan the original table in reference order.

// t of one candidate as hit_sphere would accept it (finite case, fact (1)).
__device__ __forceinline__ float candidate_t(float hb, float disc, float a) {
    const float sq = __builtin_sqrtf(disc);
    const float r1 = (-hb - sq) / a;
    if (r1 > kMinT) return r1;
    return (-hb + sq) / a;
}

// candidate_t for a ray of the guarded range (a in [2^-20, 2^60], |o|, |c|, r <= 2^30, so
// |hb| < 2^63 and disc < 2^126), with ya = recip_a(a) computed once per ray. It returns the
// same t as candidate_t wherever that t can be accepted, and a t <= min_t wherever candidate_t's
// is (the only other use of a root: candidate_t's choice between them):
//  * division: hipcc's correctly rounded x / a is v_div_scale (x2), a Newton-refined v_rcp,
//    q0 = x y, two residual corrections (the second in v_div_fmas) and v_div_fixup. v_div_scale
//    leaves both operands alone and v_div_fmas does not rescale when x, a are normal, x / a is
//    normal and exp(x) - exp(a) < 96, exp(x) > 23 (the ISA's V_DIV_SCALE_F32); v_div_fixup only
//    changes special values. div_a runs that unscaled sequence: for |x| in [2^-103, 2^64) the
//    same bits. A root that can be accepted (> min_t = 0.001 with a >= 2^-20) has |x| > 2^-30.
//    For |x| < 2^-103 (or x = 0) both quotients are below 2^-83 in magnitude, so both roots
//    are rejected alike (their sign or last bits never matter). (unit_of below uses the same
//    sequence for the scatter's unit vector, with its own range argument: numerators 0 or in
//    [2^-40, 1] against a length in [2^-20, 2].)
//  * sqrt: hipcc's correctly rounded sqrt scales x < 2^-96, takes v_sqrt and picks between its
//    neighbours by two FMA residuals, then special-cases 0 and inf; sqrt_unscaled runs the
//    unscaled middle, the same bits for x in [2^-96, 2^126]. Lanes with disc < 2^-96 take the
//    full sqrt (a zero discriminant, a grazing ray).
__device__ __forceinline__ float recip_a(float a) {
    const float y0 = __builtin_amdgcn_rcpf(a);
    return __builtin_fmaf(__builtin_fmaf(-a, y0, 1.0f), y0, y0);
}

__device__ __forceinline__ float div_a(float x, float a, float ya) {
    const float q0 = x * ya;
    const float q1 = __builtin_fmaf(__builtin_fmaf(-a, q0, x), ya, q0);
    return __builtin_fmaf(__builtin_fmaf(-a, q1, x), ya, q1);
}

__device__ __forceinline__ float sqrt_unscaled(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u);
    const float sp = __uint_as_float(__float_as_uint(s) + 1u);
    float r = __builtin_fmaf(-sm, s, x) <= 0.0f ? sm : s;
    return __builtin_fmaf(-sp, s, x) > 0.0f ? sp : r;
}

// Correctly rounded sqrt for any x: the unscaled sequence, and hipcc's full one in a real branch
// for lanes outside [2^-96, inf] (tiny, zero, negative or NaN x).
__device__ __forceinline__ float sqrt_fast(float x, uint32_t* rrow = nullptr) {
    float r = sqrt_unscaled(x);
    if (__ballot(!(x >= 0x1p-96f))) {  // wave-uniform: no exec-mask save and restore
        asm volatile("");
        region(rrow, reg::kSqrtFallback);
        const float full = __builtin_sqrtf(x);
        r = !(x >= 0x1p-96f) ? full : r;
    }
    return r;
}

// The scatter's unit vector ru / length(ru) (functions.glsl:43's normalize of three rand()
// values) with one reciprocal: len = sqrt(dot(ru, ru)), recip_a(len) once and div_a per
// component, the same bits as the three full divisions by div_a's argument above. Its two range
// conditions, for numerators x in {0} or [2^-40, 1] and len in [2^-20, 2]:
//  * v_div_scale's numerator bound: it leaves x and len alone when both are normal, x / len is
//    normal and exp(x) - exp(len) < 96, exp(x) > 23. Here exp(x) - exp(len) <= 20, the quotient
//    is at least 2^-41, and 2^-40 is far above 2^-103.
//  * a zero numerator: the full division gives +0 (the components are never negative), and
//    div_a gives q0 = 0 * ya = +0, q1 = fma(fma(-len, 0, 0), ya, 0) = +0 and +0 again.
// tests/test_unit_rcp_cpu.py compares the two forms with the reciprocal moved by an ulp either
// way. The guard is on the bits: a component passes when it is zero or at least 2^-40 (its bits
// less one, as unsigned: zero wraps to the top), len when its bits lie in [2^-20, 2]; a NaN or
// infinite component makes len NaN, and an all-zero vector len = 0, which both fail. A wave with
// a lane outside the guard takes the full sqrt and divisions in a real branch (sqrt_fast is the
// correctly rounded sqrt for every x, so that branch is the expression as it was).
// -DVCRT_UNIT_RCP=0 builds that expression alone.
#ifndef VCRT_UNIT_RCP
#define VCRT_UNIT_RCP 1
#endif
// The first rand() argument of a hit: rand(point.xy) for glass (textures.glsl:51), rand(dir.xy)
// otherwise. The operands by two selects and one rand_arg, instead of both products in
// exec-masked blocks: the same multiplications and addition on the same operands.
// -DVCRT_RAND_ARG_SEL=0 builds the two-sided form.
#ifndef VCRT_RAND_ARG_SEL
#define VCRT_RAND_ARG_SEL 1
#endif
__device__ __forceinline__ float rand_arg_first(bool glass, f3 point, f3 d) {
#if VCRT_RAND_ARG_SEL
    return rand_arg(glass ? point.x : d.x, glass ? point.y : d.y);
#else
    return glass ? rand_arg(point.x, point.y) : rand_arg(d.x, d.y);
#endif
}

__device__ __forceinline__ bool unit_guard(f3 ru, float len) {
    const uint32_t bx = __float_as_uint(ru.x) - 1u, by = __float_as_uint(ru.y) - 1u,
                   bz = __float_as_uint(ru.z) - 1u;
    const uint32_t m = min(min(bx, by), bz);
    return m >= 0x2B800000u - 1u &&                          // each 0 or >= 2^-40
           __float_as_uint(len) - 0x35800000u <= 0x0A800000u;  // 2^-20 <= len <= 2
}

__device__ __forceinline__ f3 unit_of(f3 ru, uint32_t* rrow = nullptr) {
#if VCRT_UNIT_RCP
    const float dd = dot(ru, ru);
    const float len = sqrt_unscaled(dd);
    const float yl = recip_a(len);
    f3 u = mk(div_a(ru.x, len, yl), div_a(ru.y, len, yl), div_a(ru.z, len, yl));
    const bool out = !unit_guard(ru, len);
    if (__ballot(out)) {  // wave-uniform: no exec-mask save and restore
        asm volatile("");
        region(rrow, reg::kUnitFallback);
        const f3 full = divs(ru, __builtin_sqrtf(dd));
        u = mk(out ? full.x : u.x, out ? full.y : u.y, out ? full.z : u.z);
    }
    return u;
#else
    return divs(ru, sqrt_fast(dot(ru, ru), rrow));
#endif
}

__device__ __forceinline__ float candidate_t_fast(float hb, float disc, float a, float ya,
                                                  uint32_t* rrow = nullptr) {
    float sq = sqrt_unscaled(disc);
    if (__ballot(disc < 0x1p-96f)) {  // wave-uniform: no exec-mask save and restore
        asm volatile("");  // a real branch: hipcc would otherwise run the full sqrt for every lane
        region(rrow, reg::kSqrtFallback);
        const float full = __builtin_sqrtf(disc);
        sq = disc < 0x1p-96f ? full : sq;
    }
    const float r1 = div_a(-hb - sq, a, ya);
    // the far root only in waves where some lane rejects the near one (a wave-uniform branch:
    // rays from outside the sphere take the near root; -1.5% VALU at C4, r05_valu_attrib.txt)
    float t = r1;
    if (__ballot(!(r1 > kMinT))) {
        asm volatile("");
        const float r2 = div_a(-hb + sq, a, ya);
        t = r1 > kMinT ? r1 : r2;
    }
    return t;
}

// A member whose origin lies outside or on it (cc >= 0) while the ray points away from its
// centre (hb >= 0) can never be accepted: disc_f <= RN(hb^2) and RN(sqrt(RN(hb^2))) = hb
// (binary fp, no underflow), so RN(-hb + sq) <= 0 and both roots are <= 0 < min_t. If hb^2
// underflows (hb < 2^-63), RN(hb^2) is off by at most 2^-149, so -hb + sq < 2^-74 and, with
// a >= 2^-20, root2 < 2^-54 < min_t all the same.
// A -0 hb only adds candidates; cc is never -0. (Padding members never hit: their
// r^2 = -3e38 makes disc negative or -inf.)
__device__ __forceinline__ bool may_hit(float hb, float cc, float disc) {
    return !(disc < 0.0f) && (hb < 0.0f || cc < 0.0f);
}

// Sign bit set when a member may be accepted: disc >= 0 and (hb < 0 or cc < 0), by sign bits
// (a -0 hb only adds a candidate that the exact test then rejects; disc is never -0).
__device__ __forceinline__ float hit_sign(float hb, float cc, float disc) {
    return __uint_as_float((__float_as_uint(hb) | __float_as_uint(cc)) & ~__float_as_uint(disc));
}

// The big list's may-hit tests by sign bits (kBigSign: big_roots below) and its test in one
// basic block with the first group apart from the loop (kBigPeel). With kBigPeel the second pair
// of a big group is tested whether or not it has members: a padding member (centre 0,
// r^2 = -3e38; the camera-relative record is computed from the same words) has cc = |o|^2 + 3e38,
// finite, and hb^2 <= 1.001 a |o|^2 < a cc, so its disc is negative or -inf, never NaN, and
// neither predicate accepts it -- as for the padding of the first pair and of the hierarchy's
// groups, which were always tested. Without the wave-uniform branch on the member indices the
// splat pairs {o.x, o.x} ... {a, a} and their uses share a block, where instruction selection
// folds them into op_sel_hi (no v_mov pairs), and the 80-B record is one scalar load.
// For A/B runs only: -DVCRT_BIG_SIGN=0 builds may_hit's float compares, the branch and the
// callers' plain loops, =2 the sign bits alone, =3 the one-block test and peeled callers alone.
#ifndef VCRT_BIG_SIGN
#define VCRT_BIG_SIGN 1
#endif
constexpr bool kBigSign = VCRT_BIG_SIGN == 1 || VCRT_BIG_SIGN == 2;
constexpr bool kBigPeel = VCRT_BIG_SIGN == 1 || VCRT_BIG_SIGN == 3;

// pair_disc that also returns cc = |oc|^2 - r^2 (for may_hit).
__device__ __forceinline__ void pair_disc_cc(const v2f ox, const v2f oy, const v2f oz,
                                             const v2f dx, const v2f dy, const v2f dz,
                                             const v2f a2, float4 xy, float4 zr, v2f& hb,
                                             v2f& cc, v2f& disc) {
    const v2f cx = {xy.x, xy.y}, cy = {xy.z, xy.w}, cz = {zr.x, zr.y}, r2 = {zr.z, zr.w};
    const v2f ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;
    hb = ocx * dx + ocy * dy + ocz * dz;
    cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
    disc = hb * hb - a2 * cc;
}

// pair_disc_cc for a camera ray (o = the camera centre) from the camera-relative record
// (TraceParams.cam_rec: oc and cc as pair_disc_cc computes them for that o): the remaining
// operations, in the same order, on the same operands -- the same bits, at half the work.
__device__ __forceinline__ void pair_disc_cam(const v2f dx, const v2f dy, const v2f dz,
                                              const v2f a2, float4 oxy, float4 ozc, v2f& hb,
                                              v2f& cc, v2f& disc) {
    const v2f ocx = {oxy.x, oxy.y}, ocy = {oxy.z, oxy.w}, ocz = {ozc.x, ozc.y};
    cc = (v2f){ozc.z, ozc.w};
    hb = ocx * dx + ocy * dy + ocz * dz;
    disc = hb * hb - a2 * cc;
}

__device__ __forceinline__ void consider(float t, int idx, float& max_t, int& best) {
    // (t, idx) < (max_t, best) lexicographically, as one 64-bit compare of (bits(t), index)
    // (t, max_t > min_t > 0 order as their bits); best < 0 (none yet) counts as index 0, so a
    // t equal to the initial max_t is never taken, as in hit_sphere's strict "<"
    const uint64_t kt = ((uint64_t)__float_as_uint(t) << 32) | (uint32_t)idx;
    const uint64_t km = ((uint64_t)__float_as_uint(max_t) << 32) | (uint32_t)max(best, 0);
    const bool take = (t > kMinT) & (kt < km);
    max_t = take ? t : max_t;
    best = take ? idx : best;
}

__device__ __forceinline__ v2f vfma(v2f x, v2f y, v2f z) {
    return __builtin_elementwise_fma(x, y, z);
}

// 1 when the wave-uniform x != 0, in SALU (the compiler lowers `x ? 1 : 0` of a ballot
// result through a VGPR: v_cndmask + v_readfirstlane per test).
__device__ __forceinline__ uint32_t nonzero(uint64_t x) {
    uint32_t r;
    asm volatile("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, 1, 0" : "=s"(r) : "s"(x) : "scc");
    return r;
}

struct CullRay {  // one ray's origin, splatted for packed tests
    v2f ox, oy, oz;
};

// One ray prepared for the box test (3), splatted for packed tests.
struct BoxRay {
    v2f ix, iy, iz;  // 1 / d'
    v2f cx, cy, cz;  // -o / d'
    v2f c1, c2;      // gap slack: c1 + K_b c2
    // Slab rays (3a): iy holds t0 and cy holds t1, the near and far end of the shared y slab, in
    // place of the y axis' two terms -- the same registers, and the passes fetch the same fields.
};

__device__ __forceinline__ float box_axis(float o, float d, float tau, v2f& i, v2f& c) {
    const float dd = copysignf(fmaxf(fabsf(d), 0x1p-40f), d);
    const float iv = __builtin_amdgcn_rcpf(dd);
    const float co = __builtin_fmaf(-o, iv, tau);  // the plane shift of (4) (tau = 0: none)
    i = (v2f){iv, iv};
    c = (v2f){co, co};
    return fabsf(iv);
}

// ya: recip_a(dot(d, d)), for tau of (4). slab (wave-uniform; the flat scans on a scene whose
// boxes share their y extent, TraceParams.slab): the y axis as the ray's interval of (3a).
__device__ __forceinline__ BoxRay box_ray(const TraceParams& p, const f3 o, const f3 d, float ya,
                                          bool slab = false) {
    BoxRay r;
    const float on = __builtin_amdgcn_sqrtf(dot(o, o)) + p.box_margin[0];
    const float Q = on * on + p.box_margin[1];
    const float tau = __builtin_amdgcn_sqrtf(3.2e-7f * Q * ya);  // (4)
    const float ax = box_axis(o.x, d.x, tau, r.ix, r.cx), ay = box_axis(o.y, d.y, tau, r.iy, r.cy),
                az = box_axis(o.z, d.z, tau, r.iz, r.cz);
    const float J = 2.002f * fmaxf(fmaxf(ax, ay), az);  // 1.001 J
    const float oinf = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    const float c1 = J * (3.04e-7f * (p.box_margin[2] + oinf));  // 5.1u
    const float c2 = J * Q;
    r.c1 = (v2f){c1, c1};
    r.c2 = (v2f){c2, c2};
    if (slab) {
        const float tly = __builtin_fmaf(p.slab[0], r.iy.x, r.cy.x);
        const float thy = __builtin_fmaf(p.slab[1], r.iy.x, r.cy.x);
        const float t0 = fmaxf(fminf(tly, thy), 0.0f);  // with the clamp of (4)
        const float t1 = fmaxf(tly, thy);
        r.iy = (v2f){t0, t0};
        r.cy = (v2f){t1, t1};
    }
    return r;
}

// The box test's gap for a pair of boxes (TraceParams.cbound: (lox0,lox1,loy0,loy1)
// (loz0,loz1,hix0,hix1) (hiy0,hiy1,hiz0,hiz1) (K0,K1,-,-)): negative when the ray rules the box
// out. (All values finite or +inf, so the gap is never -0 or NaN.) kSlab: the ray's y interval
// (3a) in place of the pair's own y planes.
template <bool kSlab = false>
__device__ __forceinline__ v2f box_gap(const BoxRay& r, float4 b0, float4 b1, float4 b2,
                                       float4 b3) {
    if constexpr (kSlab) {
        const v2f lox = {b0.x, b0.y}, loz = {b1.x, b1.y};
        const v2f hix = {b1.z, b1.w}, hiz = {b2.z, b2.w}, K = {b3.x, b3.y};
        const v2f tlx = vfma(lox, r.ix, r.cx), thx = vfma(hix, r.ix, r.cx);
        const v2f tlz = vfma(loz, r.iz, r.cz), thz = vfma(hiz, r.iz, r.cz);
        v2f tn, tf;
        tn.x = fmaxf(fmaxf(fminf(tlx.x, thx.x), fminf(tlz.x, thz.x)), r.iy.x);
        tn.y = fmaxf(fmaxf(fminf(tlx.y, thx.y), fminf(tlz.y, thz.y)), r.iy.y);
        tf.x = fminf(fminf(fmaxf(tlx.x, thx.x), fmaxf(tlz.x, thz.x)), r.cy.x);
        tf.y = fminf(fminf(fmaxf(tlx.y, thx.y), fmaxf(tlz.y, thz.y)), r.cy.y);
        return vfma(K, r.c2, (tf - tn) + r.c1);
    }
    const v2f lox = {b0.x, b0.y}, loy = {b0.z, b0.w}, loz = {b1.x, b1.y};
    const v2f hix = {b1.z, b1.w}, hiy = {b2.x, b2.y}, hiz = {b2.z, b2.w}, K = {b3.x, b3.y};
    const v2f tlx = vfma(lox, r.ix, r.cx), thx = vfma(hix, r.ix, r.cx);
    const v2f tly = vfma(loy, r.iy, r.cy), thy = vfma(hiy, r.iy, r.cy);
    const v2f tlz = vfma(loz, r.iz, r.cz), thz = vfma(hiz, r.iz, r.cz);
    v2f tn, tf;
    tn.x = fmaxf(fmaxf(fminf(tlx.x, thx.x), fminf(tly.x, thy.x)), fminf(tlz.x, thz.x));
    tn.y = fmaxf(fmaxf(fminf(tlx.y, thx.y), fminf(tly.y, thy.y)), fminf(tlz.y, thz.y));
    tf.x = fminf(fminf(fmaxf(tlx.x, thx.x), fmaxf(tly.x, thy.x)), fmaxf(tlz.x, thz.x));
    tf.y = fminf(fminf(fmaxf(tlx.y, thx.y), fmaxf(tly.y, thy.y)), fmaxf(tlz.y, thz.y));
    // (4): the stretch of the line behind -tau does not count
    tn.x = fmaxf(tn.x, 0.0f);
    tn.y = fmaxf(tn.y, 0.0f);
    return vfma(K, r.c2, (tf - tn) + r.c1);
}

// Box test of one pair, wave-uniform: bit 0/1 set when some lane may accept a member of box
// 0/1.
struct BoundPair {
    float4 b0, b1, b2, b3;
};

__device__ __forceinline__ BoundPair load_bound_pair(cfloat4* b) {
    return BoundPair{b[0], b[1], b[2], b[3]};
}

template <bool kStats>
__device__ __forceinline__ uint32_t bound_pair_need(const BoxRay& r, const BoundPair& bp,
                                                    uint32_t& lane_needs, uint32_t& lane_cnt) {
    const v2f g = box_gap(r, bp.b0, bp.b1, bp.b2, bp.b3);
    const bool m0 = !(g.x < 0.0f), m1 = !(g.y < 0.0f);
    const uint64_t n0 = __ballot(m0), n1 = __ballot(m1);
    if constexpr (kStats) {
        lane_needs += __popcll(n0) + __popcll(n1);
        lane_cnt += (uint32_t)m0 + (uint32_t)m1;
    }
    return nonzero(n0) | (nonzero(n1) << 1);
}

// The roots of the big list's members (exact_group_uniform, exact_group_uniform_cam with
// kBigSign), entered by hit_sign's sign bits h0..h3 in place of may_hit's float compares (which
// cost two NaN-quieting v_max, a v_min and two v_cmp per member, and as many again for the gate's
// max of the four disc: one v_bitop3 and one integer compare per member here).
// Exactness: hit_sign's sign bit is may_hit except where hb = -0. cc is never -0 (a difference of
// unequal numbers, or +0 under round-to-nearest) and disc neither (hb^2 - a cc: +0 or a nonzero
// value); disc is finite for a ray of the guarded range (|hb| < 2^63, a |cc| < 2^123; a padding
// member's is -inf, sign set), which both callers' rays are, so no NaN's sign bit is read.
// With hb = -0 and cc >= 0 the bit is set where may_hit is false; if also disc >= 0 then
// disc = RN(0 - RN(a cc)) >= 0 forces RN(a cc) = 0 (cc = 0, or a product that underflows) and
// disc = +0, so sq = 0 and candidate_t_fast's roots are div_a(-hb - 0, a, ya) = (+0) ya = 0 and
// div_a(-hb + 0, a, ya) = 0: both <= kMinT (tests/test_big_sign_cpu.py), and
// `consider` (take only if t > kMinT) rejects them: max_t and best are may_hit's. (hb = -0 with
// cc < 0: both forms accept.) The gate, "some member may hit", is tighter than the old "some disc
// >= 0", which it implies: fewer entries of the block, the same entries of each member.
// A missing second pair takes hb = cc = 0, disc = -1: (0 | 0) & ~bits(-1) = 0, sign clear.
__device__ __forceinline__ void big_roots(float h0, float h1, float h2, float h3, v2f hb01,
                                          v2f d01, v2f hb23, v2f d23, float4 idf, float a,
                                          float ya, float& max_t, int& best, uint32_t* rrow,
                                          uint32_t rb) {
    const uint32_t any = (__float_as_uint(h0) | __float_as_uint(h1)) |
                         (__float_as_uint(h2) | __float_as_uint(h3));
    if (__ballot((int)any < 0)) {
        region(rrow, rb);
        if (__float_as_int(h0) < 0) {
            region(rrow, rb + 1);
            consider(candidate_t_fast(hb01.x, d01.x, a, ya, rrow), __float_as_int(idf.x), max_t,
                     best);
        }
        if (__float_as_int(h1) < 0) {
            region(rrow, rb + 2);
            consider(candidate_t_fast(hb01.y, d01.y, a, ya, rrow), __float_as_int(idf.y), max_t,
                     best);
        }
        if (__float_as_int(h2) < 0) {
            region(rrow, rb + 3);
            consider(candidate_t_fast(hb23.x, d23.x, a, ya, rrow), __float_as_int(idf.z), max_t,
                     best);
        }
        if (__float_as_int(h3) < 0) {
            region(rrow, rb + 4);
            consider(candidate_t_fast(hb23.y, d23.y, a, ya, rrow), __float_as_int(idf.w), max_t,
                     best);
        }
    }
}

// The exact test of one group for every lane (wave-uniform scalar loads of the 80-B record):
// the big-sphere list, tested for every ray ahead of the hierarchy.
__device__ __forceinline__ void exact_group_uniform(cfloat4* rec, const CullRay& r, v2f dx, v2f dy,
                                                    v2f dz, v2f a2, float a, float ya,
                                                    float& max_t, int& best,
                                                    uint32_t* rrow = nullptr, uint32_t rb = 0) {
    const float4 q0 = rec[0], q1 = rec[1], idf = rec[4];
    v2f hb01, cc01, d01, hb23 = {0.f, 0.f}, cc23 = {0.f, 0.f}, d23 = {-1.f, -1.f};
    pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, q0, q1, hb01, cc01, d01);
    // members 2 and 3 only when the group has them (wave-uniform); kBigPeel: always (above)
    if (kBigPeel || __float_as_int(idf.z) >= 0 || __float_as_int(idf.w) >= 0)
        pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, rec[2], rec[3], hb23, cc23, d23);
    if constexpr (kBigSign) {
        big_roots(hit_sign(hb01.x, cc01.x, d01.x), hit_sign(hb01.y, cc01.y, d01.y),
                  hit_sign(hb23.x, cc23.x, d23.x), hit_sign(hb23.y, cc23.y, d23.y), hb01, d01,
                  hb23, d23, idf, a, ya, max_t, best, rrow, rb);
        return;
    }
    const float m4 = fmaxf(fmaxf(d01.x, d01.y), fmaxf(d23.x, d23.y));
    if (__ballot(!(m4 < 0.0f))) {
        region(rrow, rb);
        if (may_hit(hb01.x, cc01.x, d01.x)) {
            region(rrow, rb + 1);
            consider(candidate_t_fast(hb01.x, d01.x, a, ya, rrow), __float_as_int(idf.x), max_t,
                     best);
        }
        if (may_hit(hb01.y, cc01.y, d01.y)) {
            region(rrow, rb + 2);
            consider(candidate_t_fast(hb01.y, d01.y, a, ya, rrow), __float_as_int(idf.y), max_t,
                     best);
        }
        if (may_hit(hb23.x, cc23.x, d23.x)) {
            region(rrow, rb + 3);
            consider(candidate_t_fast(hb23.x, d23.x, a, ya, rrow), __float_as_int(idf.z), max_t,
                     best);
        }
        if (may_hit(hb23.y, cc23.y, d23.y)) {
            region(rrow, rb + 4);
            consider(candidate_t_fast(hb23.y, d23.y, a, ya, rrow), __float_as_int(idf.w), max_t,
                     best);
        }
    }
}

// exact_group_uniform for camera rays, from the group's camera-relative record `crec` (the
// member indices still come from the group record `rec`).
__device__ __forceinline__ void exact_group_uniform_cam(cfloat4* crec, cfloat4* rec, v2f dx,
                                                        v2f dy, v2f dz, v2f a2, float a,
                                                        float ya, float& max_t, int& best,
                                                        uint32_t* rrow = nullptr,
                                                        uint32_t rb = 0) {
    const float4 c0 = crec[0], c1 = crec[1], idf = rec[4];
    v2f hb01, cc01, d01, hb23 = {0.f, 0.f}, cc23 = {0.f, 0.f}, d23 = {-1.f, -1.f};
    pair_disc_cam(dx, dy, dz, a2, c0, c1, hb01, cc01, d01);
    if (kBigPeel || __float_as_int(idf.z) >= 0 || __float_as_int(idf.w) >= 0)
        pair_disc_cam(dx, dy, dz, a2, crec[2], crec[3], hb23, cc23, d23);
    if constexpr (kBigSign) {
        big_roots(hit_sign(hb01.x, cc01.x, d01.x), hit_sign(hb01.y, cc01.y, d01.y),
                  hit_sign(hb23.x, cc23.x, d23.x), hit_sign(hb23.y, cc23.y, d23.y), hb01, d01,
                  hb23, d23, idf, a, ya, max_t, best, rrow, rb);
        return;
    }
    const float m4 = fmaxf(fmaxf(d01.x, d01.y), fmaxf(d23.x, d23.y));
    if (__ballot(!(m4 < 0.0f))) {
        region(rrow, rb);
        if (may_hit(hb01.x, cc01.x, d01.x)) {
            region(rrow, rb + 1);
            consider(candidate_t_fast(hb01.x, d01.x, a, ya, rrow), __float_as_int(idf.x), max_t,
                     best);
        }
        if (may_hit(hb01.y, cc01.y, d01.y)) {
            region(rrow, rb + 2);
            consider(candidate_t_fast(hb01.y, d01.y, a, ya, rrow), __float_as_int(idf.y), max_t,
                     best);
        }
        if (may_hit(hb23.x, cc23.x, d23.x)) {
            region(rrow, rb + 3);
            consider(candidate_t_fast(hb23.x, d23.x, a, ya, rrow), __float_as_int(idf.z), max_t,
                     best);
        }
        if (may_hit(hb23.y, cc23.y, d23.y)) {
            region(rrow, rb + 4);
            consider(candidate_t_fast(hb23.y, d23.y, a, ya, rrow), __float_as_int(idf.w), max_t,
                     best);
        }
    }
}

// Stats builds count in `hit_groups` the lanes that need each group (sum over group bounds)
// and in `lane_cnt` the groups this lane needs.
template <bool kStats>
__device__ __forceinline__ void scan_culled(const TraceParams& p, const f3 o, const f3 d,
                                            float& max_t, int& best, uint32_t& groups_tested,
                                            uint32_t& bounds_tested, uint32_t& hit_groups,
                                            uint32_t& lane_cnt) {
    uint32_t node_lanes = 0, node_cnt = 0;
    uint32_t n_groups = 0, n_bounds = 0;
    const float a = dot(d, d);
    CullRay r;
    r.ox = (v2f){o.x, o.x};
    r.oy = (v2f){o.y, o.y};
    r.oz = (v2f){o.z, o.z};
    const BoxRay br = box_ray(p, o, d, recip_a(a));
    const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {a, a};
    cfloat4* bound = (cfloat4*)p.cbound;
    cfloat4* node = (cfloat4*)p.cnode;
    cfloat4* geom = (cfloat4*)p.cgroup;
    for (int gb = 0; gb < p.nbig; ++gb)  // the big spheres, for every ray
        exact_group_uniform(geom + 5 * gb, r, dx, dy, dz, a2, a, recip_a(a), max_t, best);
    n_groups += (uint32_t)p.nbig;
    geom += 5 * p.nbig;           // the hierarchy's groups
    const int ncg = p.ncgroups;  // multiple of 16: whole node pairs
    cfloat4* top = (cfloat4*)p.ctop;
    uint32_t tops = 0;
    for (int base = 0; base < ncg; base += 64) {
        // level 0: the chunk's own bound (tested for two chunks at a time)
        if ((base & 127) == 0) {
            tops = bound_pair_need<false>(br, load_bound_pair(top + 4 * (base >> 7)), node_lanes,
                                          node_cnt);
            n_bounds += 2;
        }
        if (((tops >> ((base >> 6) & 1)) & 1u) == 0) continue;
        // level 1: which of the next (up to) 8 nodes of 8 groups may any lane hit? (the
        // scalar loads run one pair ahead of the tests)
        const int nn = min(8, (ncg - base) >> 3);
        cfloat4* nb = node + 4 * (base >> 4);
        uint32_t nodes = 0;
        BoundPair cur = load_bound_pair(nb);
        for (int j = 0; j < nn; j += 2) {
            const BoundPair nxt = load_bound_pair(nb + 4 * ((j + 2 < nn ? j + 2 : j) >> 1));
            nodes |= bound_pair_need<false>(br, cur, node_lanes, node_cnt) << j;
            cur = nxt;
        }
        n_bounds += (uint32_t)(nn + 8 * __popc(nodes));
        // level 2: which groups of those nodes?
        uint64_t need = 0;
        if (nodes) cur = load_bound_pair(bound + 4 * ((base + 8 * __builtin_ctz(nodes)) >> 1));
        while (nodes) {
            const int j = __builtin_ctz(nodes);
            nodes &= nodes - 1;
            cfloat4* gb = bound + 4 * ((base + 8 * j) >> 1);
            cfloat4* gnext = bound + 4 * ((base + 8 * (nodes ? __builtin_ctz(nodes) : j)) >> 1);
#pragma unroll
            for (int k = 0; k < 8; k += 2) {
                const BoundPair nxt = load_bound_pair(k + 2 < 8 ? gb + 4 * ((k + 2) >> 1) : gnext);
                need |= (uint64_t)bound_pair_need<kStats>(br, cur, hit_groups, lane_cnt)
                        << (8 * j + k);
                cur = nxt;
            }
        }
        // the exact hit_sphere test on the groups that survived (next group prefetched)
        n_groups += (uint32_t)__popcll(need);
        if (!need) continue;
        int gi = base + __builtin_ctzll(need);
        float4 q0 = geom[5 * gi], q1 = geom[5 * gi + 1], q2 = geom[5 * gi + 2],
               q3 = geom[5 * gi + 3];
        while (true) {
            need &= need - 1;
            const int gn = need ? base + __builtin_ctzll(need) : gi;
            const float4 n0 = geom[5 * gn], n1 = geom[5 * gn + 1], n2 = geom[5 * gn + 2],
                         n3 = geom[5 * gn + 3];
            v2f hb01, cc01, d01, hb23, cc23, d23;
            pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, q0, q1, hb01, cc01, d01);
            pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, q2, q3, hb23, cc23, d23);
            const float m4 = fmaxf(fmaxf(d01.x, d01.y), fmaxf(d23.x, d23.y));
            if (__ballot(!(m4 < 0.0f))) {
                const float4 idf = geom[5 * gi + 4];
                const int4 id = make_int4(__float_as_int(idf.x), __float_as_int(idf.y),
                                          __float_as_int(idf.z), __float_as_int(idf.w));
                if (may_hit(hb01.x, cc01.x, d01.x))
                    consider(candidate_t(hb01.x, d01.x, a), id.x, max_t, best);
                if (may_hit(hb01.y, cc01.y, d01.y))
                    consider(candidate_t(hb01.y, d01.y, a), id.y, max_t, best);
                if (may_hit(hb23.x, cc23.x, d23.x))
                    consider(candidate_t(hb23.x, d23.x, a), id.z, max_t, best);
                if (may_hit(hb23.y, cc23.y, d23.y))
                    consider(candidate_t(hb23.y, d23.y, a), id.w, max_t, best);
            }
            if (!need) break;
            gi = gn;
            q0 = n0;
            q1 = n1;
            q2 = n2;
            q3 = n3;
        }
    }
    tally(groups_tested, 2u * n_groups);  // in half-groups
    tally(bounds_tested, n_bounds);
}

// Per-lane culled scan (variant CULL_LANE). Same tables and tests as scan_culled, but only
// the node level runs wave-uniformly (scalar loads, per-lane results); each lane then tests
// the groups of its own nodes and runs the exact test on its own groups, gathering table rows
// with per-lane addresses (from an LDS copy, or from global memory when the tables are too
// large). A wave's work becomes the largest per-lane need instead of the union over lanes.
// Lanes accept candidates with the same `consider` rule, so the result is the same.

// (acc << 1) | sign bit of v: v_alignbit_b32, one VALU per collected bit.
__device__ __forceinline__ uint32_t push_sign(uint32_t acc, float v) {
    return __builtin_amdgcn_alignbit(acc, __float_as_uint(v), 31);
}

// Sign of the box gap for both boxes of a pair: set (negative) when this lane rules the box
// out. Pushed high element first.
template <bool kSlab = false>
__device__ __forceinline__ uint32_t push_bound_pair(uint32_t acc, const BoxRay& r, float4 b0,
                                                    float4 b1, float4 b2, float4 b3) {
    const v2f D = box_gap<kSlab>(r, b0, b1, b2, b3);
    return push_sign(push_sign(acc, D.y), D.x);
}

// Box test of a group pair in the near/far layout (TraceParams.cbound_nf). For inv = 1/d' > 0
// the exact products order lo*inv <= hi*inv and rounding is monotone, so fma(lo, inv, c) <=
// fma(hi, inv, c): box_gap's per-axis min / max are the lo / hi plane when inv > 0 and the hi / lo
// plane when inv < 0 (d' is never 0). Each axis stores (lo, hi, lo), so the near plane sits at
// byte 8 * sign(inv) of the axis and the far plane 8 bytes after it: one per-lane address per
// axis, one ds_read2_b64 per axis and pair. The gap is box_gap's value (at most the sign of a
// zero tf - tn differs, and adding the slack c1 >= +0 gives the same sum for either zero), for
// one v_max3 + one v_min3 per box instead of 3 min + 3 max + max3 + min3.
struct NearFarAddr {
    const char* x;  // near plane of axis x of pair 0 (far: + 8 bytes)
    const char* y;
    const char* z;
    const char* k;  // (K0, K1) of pair 0
};

__device__ __forceinline__ NearFarAddr near_far_addr(const float4* pairs, float ix, float iy,
                                                     float iz) {
    const char* b = reinterpret_cast<const char*>(pairs);
    NearFarAddr a;
    a.x = b + ((__float_as_uint(ix) >> 31) << 3);
    a.y = b + 24 + ((__float_as_uint(iy) >> 31) << 3);
    a.z = b + 48 + ((__float_as_uint(iz) >> 31) << 3);
    a.k = b + 72;
    return a;
}

__device__ __forceinline__ v2f ld2(const char* p) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    return (v2f){v.x, v.y};
}

template <bool kSlab = false>
__device__ __forceinline__ uint32_t push_bound_pair_nf(uint32_t acc, const BoxRay& r,
                                                       const NearFarAddr& a, int off) {
    const v2f tnx = vfma(ld2(a.x + off), r.ix, r.cx), tfx = vfma(ld2(a.x + off + 8), r.ix, r.cx);
    if constexpr (kSlab) {  // (3a): the y axis is the ray's own interval, clamp included
        const v2f tnz = vfma(ld2(a.z + off), r.iz, r.cz), tfz = vfma(ld2(a.z + off + 8), r.iz, r.cz);
        v2f tn, tf;
        tn.x = fmaxf(fmaxf(tnx.x, tnz.x), r.iy.x);
        tn.y = fmaxf(fmaxf(tnx.y, tnz.y), r.iy.y);
        tf.x = fminf(fminf(tfx.x, tfz.x), r.cy.x);
        tf.y = fminf(fminf(tfx.y, tfz.y), r.cy.y);
        const v2f D = vfma(ld2(a.k + off), r.c2, (tf - tn) + r.c1);
        return push_sign(push_sign(acc, D.y), D.x);
    }
    const v2f tny = vfma(ld2(a.y + off), r.iy, r.cy), tfy = vfma(ld2(a.y + off + 8), r.iy, r.cy);
    const v2f tnz = vfma(ld2(a.z + off), r.iz, r.cz), tfz = vfma(ld2(a.z + off + 8), r.iz, r.cz);
    v2f tn, tf;
    tn.x = fmaxf(fmaxf(tnx.x, tny.x), tnz.x);
    tn.y = fmaxf(fmaxf(tnx.y, tny.y), tnz.y);
    tf.x = fminf(fminf(tfx.x, tfy.x), tfz.x);
    tf.y = fminf(fminf(tfx.y, tfy.y), tfz.y);
    tn.x = fmaxf(tn.x, 0.0f);  // (4), as box_gap
    tn.y = fmaxf(tn.y, 0.0f);
    const v2f D = vfma(ld2(a.k + off), r.c2, (tf - tn) + r.c1);
    return push_sign(push_sign(acc, D.y), D.x);
}

// The four pairs of a node's groups or a chunk's nodes. kSlab 0 / 1: the form is known; -1: by
// the wave-uniform `slab`, the four pairs in either form (not a branch per pair).
template <int kSlab>
__device__ __forceinline__ uint32_t push_bound_pairs4_nf(const BoxRay& r, const NearFarAddr& a,
                                                         bool slab) {
    uint32_t out = 0;
    if (kSlab > 0 || (kSlab < 0 && slab)) {
#pragma unroll
        for (int k = 3; k >= 0; k--) out = push_bound_pair_nf<true>(out, r, a, 80 * k);
    } else {
#pragma unroll
        for (int k = 3; k >= 0; k--) out = push_bound_pair_nf<false>(out, r, a, 80 * k);
    }
    return out;
}

// ---- flattened scan (variant CULL_FLAT) ------------------------------------------------------
// The per-lane scan runs each level as many wave passes as its busiest lane needs (twice the
// mean). Here the work items of the per-lane levels and of the root evaluation are kept as
// four per-wave stacks in LDS and dealt to the wave's live lanes a full wave at a time, each
// lane working on another lane's ray (fetched with ds_bpermute):
//   chunk (owner, chunk)               -> tests the chunk's <= 8 node bounds -> node entries
//   node  (owner, node)                -> tests the node's 8 group bounds -> group entries
//   group (owner, group)               -> exact test of the 4 members     -> candidate entries
//   cand  (owner, group, member)       -> the accepted root, into the owner's key
// Entries are pushed at a wave prefix of the lanes' counts (their order never matters; stack
// heights are wave-uniform, in SGPRs) and carried from chunk to chunk; only the segment's last
// passes run partly empty. (A per-lane LDS atomic add on the height instead serialises on its
// one address: 9x the LDS bank conflicts of the per-lane scan, 9% slower overall.) Every owner's
// (t, sphere index) minimum is an LDS 64-bit word updated with ds_min_u64: the lexicographic
// minimum of (t, index) is what `consider` computes, since t > 0 orders like its bit pattern.
// A pass pushes onto the next stack only while that stack holds < nact <= 64 entries (full
// passes run deepest stack first; the final drain's partial passes run top-down), which bounds
// every stack: < 64 left over + at most 8 x 64 (node, group) or 4 x 64 (cand) pushed by one pass;
// chunk entries (one per lane and chunk) are pushed between drains, onto < 64 left over.
// The group-footprint scan (fact (5g)) has its own drain, flat_drain_groups: a group pass there
// takes two entries per lane, one test after the other, wherever the rule would run a second
// group pass right after the first (ng >= nact + th), and counts as two; it pushes at most
// 2 x 4 x 64 candidates onto < 64 left over, 575 in all, which that scan keeps in its unused node
// stack (see kNodeCap).
// (Round 2: the chunk level was wave-uniform -- every lane tested the nodes of every chunk some
// lane needed, with per-lane min/max box tests on scalar-loaded boxes; as passes the nodes are
// tested only for the lanes that need the chunk, by the near/far box test.)
constexpr int kPendSky = -2;  // trace_impl's pend_best for a deferred sky segment
constexpr int kChunkCap = 128;
// 63 + 8 x 64 node entries; or, in the group-footprint scan, whose node stack is never touched and
// has the candidates' 16-bit type, that scan's candidates: 63 + 2 x 4 x 64 after a double group
// pass, 575 too. `cand` (kCandCap: 63 + 4 x 64) holds the candidates of every other scan, and the
// LDS stays as it was.
constexpr int kNodeCap = 576;
constexpr int kGroupCap = 576;
constexpr int kCandCap = 320;
// The group-footprint level's push cap (fact (5g)): a lane with more groups than this is a heavy
// lane, whose groups the wave deals across its lanes. Light counts up to 7 fit the 3-bit wave
// prefix (a build with -DVCRT_PUSH_CAP=8..15, for A/B runs only, takes the 4-bit one).
#ifndef VCRT_PUSH_CAP
#define VCRT_PUSH_CAP 7
#endif
constexpr uint32_t kPushCap = VCRT_PUSH_CAP;
constexpr int kPushBits = kPushCap <= 7u ? 3 : 4;
static_assert(kPushCap >= 1u && kPushCap <= 15u, "light counts go through wave_prefix<kPushBits>");
// The group-footprint scan's drain with double group passes (flat_drain_groups). For A/B runs
// only: -DVCRT_GROUP_PASS2=0 builds flat_drain's single passes with the candidates in `cand`,
// =2 flat_drain_groups with single passes only.
#ifndef VCRT_GROUP_PASS2
#define VCRT_GROUP_PASS2 1
#endif
constexpr bool kGroupPass2 = VCRT_GROUP_PASS2 != 0;
constexpr bool kGroupPassDouble = VCRT_GROUP_PASS2 == 1;
// The group footprint's mask by two v_bitop3 a word and a zero row in the tables' place of the
// select per word (group_foot_mask). For A/B runs only: -DVCRT_FOOT_BITOP=0 builds the and /
// select / or form, which never reads the zero row.
#ifndef VCRT_FOOT_BITOP
#define VCRT_FOOT_BITOP 1
#endif
constexpr bool kFootBitop = VCRT_FOOT_BITOP != 0;

// Stack entries, by format kFmt:
//   0 (narrow8, the LDS-table kernel, <= 256 groups): 16-bit owner << 8 | index, and 16-bit
//     candidate entries (node/group entry) << 2 | member;
//   1 (narrow10, the boxes-in-LDS kernel, <= 1024 groups): 16-bit owner << 10 | index,
//     32-bit candidate entries;
//   2 (wide, the global-table kernel, any size): 32-bit owner << 24 | index and candidates.
template <int kFmt>
struct FlatFmt {
    using entry_t = typename std::conditional<kFmt == 2, uint32_t, uint16_t>::type;
    using cand_t = typename std::conditional<kFmt == 0, uint16_t, uint32_t>::type;
    static constexpr int kShift = kFmt == 2 ? 24 : kFmt == 1 ? 10 : 8;  // owner field
    static constexpr uint32_t kMask = (1u << kShift) - 1u;
};

template <int kFmt, bool kChunks = true>
struct WaveScratch {
    using entry_t = typename FlatFmt<kFmt>::entry_t;
    static constexpr bool kHasChunks = kChunks;
    unsigned long long key[64];  // per owner lane: (bits(t) << 32) | sphere index
    uint32_t work[2];            // issued-work tallies of the flat scan: half-groups, box tests
    typename FlatFmt<kFmt>::cand_t cand[kCandCap];  // group entry << 2 | member
    entry_t group[kGroupCap];    // owner << kShift | group
    entry_t node[kNodeCap];      // owner << kShift | node
    entry_t chunk[kChunks ? kChunkCap : 0];  // owner << kShift | chunk (64 groups)
};
static_assert(sizeof(WaveScratch<0, false>) == kWaveScratchBytes8, "host LDS size");  // 3464
static_assert(sizeof(WaveScratch<1>) == kWaveScratchBytes, "host LDS size");
static_assert(sizeof(WaveScratch<2>) == kWaveScratchBytesWide, "host LDS size");
static_assert(std::is_same<FlatFmt<0>::cand_t, FlatFmt<0>::entry_t>::value &&
                  kNodeCap >= 63 + 2 * 4 * 64 && kCandCap >= 63 + 4 * 64,
              "a double group pass's candidates fit the node stack, a single pass's `cand`");

// The candidate stack: `node` for the group-footprint scan with double passes (see kNodeCap).
template <bool kInNode, class WS>
__device__ __forceinline__ auto* cand_stack(WS* ws) {
    if constexpr (kInNode)
        return ws->node;
    else
        return ws->cand;
}

// The flat scans' hierarchy group records, 80 B each: four pair-SoA float4s + the members'
// world[] indices. Global records (kGRec, TraceParams.cgroup): the indices as int bits. LDS
// records: the indices as uint16 in the first 8 B of the fifth float4 (the 80-B stride starts
// 16 consecutive records on 16 different bank quadruples, so the ds_read_b128 of a 16-lane group
// reading different groups is conflict-free; a 64-B stride gave four).
template <bool kGRec>
struct GroupTab {
    const float4* geom;
    __device__ __forceinline__ const float4* rec(uint32_t gi) const { return geom + 5u * gi; }
    __device__ __forceinline__ int index(uint32_t gi, uint32_t s) const {
        if constexpr (kGRec) {
            const float4 idf = geom[5u * gi + 4u];
            return __float_as_int(s == 0 ? idf.x : s == 1 ? idf.y : s == 2 ? idf.z : idf.w);
        } else {
            return (int)reinterpret_cast<const uint16_t*>(geom + 5u * gi + 4u)[s];
        }
    }
};

__device__ __forceinline__ unsigned long long pack_hit(float t, int idx) {
    return ((unsigned long long)__float_as_uint(t) << 32) | (uint32_t)idx;
}

// Exclusive prefix over the active lanes of a per-lane count c < 2^kBits, and the wave total.
// With every lane active: an inclusive DPP scan (row_shr 1/2/4/8, row_bcast 15/31; 8 VALU).
// Otherwise (the drain at the end of the grid, where finished lanes are masked off and DPP
// would read their stale registers): bit-sliced ballots, ~5 VALU per bit.
template <int kBits>
__device__ __forceinline__ uint32_t wave_prefix(uint32_t c, uint32_t& total,
                                                uint32_t* rrow = nullptr) {
    if (__builtin_amdgcn_read_exec() == ~0ull) {
        int x = (int)c;
        x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);  // row_shr:1
        x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);  // row_shr:2
        x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);  // row_shr:4
        x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);  // row_shr:8
        x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15
        x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31
        total = (uint32_t)__builtin_amdgcn_readlane(x, 63);
        return (uint32_t)x - c;
    }
    region(rrow, reg::kPrefixSlow);
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int b = 0; b < kBits; ++b) {
        const uint64_t m = __ballot((c >> b) & 1u);
        pre += lanes_below(m) << b;
        tot += (uint32_t)__popcll(m) << b;
    }
    total = tot;
    return pre;
}

// Maximum over the active lanes of v < 2^kBits, wave-uniform: one compare per bit (ballots)
// instead of a shuffle reduction.
template <int kBits>
__device__ __forceinline__ uint32_t wave_max_small(uint32_t v) {
    uint32_t m = 0;
#pragma unroll
    for (int b = kBits - 1; b >= 0; --b)
        if (__ballot(v >= (m | (1u << b)))) m |= 1u << b;
    return m;
}

// v of lane src_x4 / 4 (ds_bpermute; the source lane is live)
__device__ __forceinline__ float from_lane(int src_x4, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_x4, __float_as_int(v)));
}

struct FlatRay {  // this lane's ray, as the passes fetch it
    float ox, oy, oz, dx, dy, dz, a, ya;
    BoxRay br;
};

// The exact test of group entry e (owner << kShift | group) for the owner's ray: bit s set when
// member s may be accepted (hit_sign).
template <int kFmt, bool kGRec>
__device__ __forceinline__ uint32_t group_hit_bits(uint32_t e, const GroupTab<kGRec>& tg,
                                                   const FlatRay& my) {
    using F = FlatFmt<kFmt>;
    const int src = (int)(e >> F::kShift) << 2;
    const float ox = from_lane(src, my.ox), oy = from_lane(src, my.oy), oz = from_lane(src, my.oz);
    const float dx = from_lane(src, my.dx), dy = from_lane(src, my.dy), dz = from_lane(src, my.dz);
    const float a = from_lane(src, my.a);
    const float4* g = tg.rec(e & F::kMask);
    const float4 q0 = g[0], q1 = g[1], q2 = g[2], q3 = g[3];
    const v2f vox = {ox, ox}, voy = {oy, oy}, voz = {oz, oz};
    const v2f vdx = {dx, dx}, vdy = {dy, dy}, vdz = {dz, dz}, a2 = {a, a};
    v2f hb01, cc01, d01, hb23, cc23, d23;
    pair_disc_cc(vox, voy, voz, vdx, vdy, vdz, a2, q0, q1, hb01, cc01, d01);
    pair_disc_cc(vox, voy, voz, vdx, vdy, vdz, a2, q2, q3, hb23, cc23, d23);
    uint32_t hits = push_sign(0u, hit_sign(hb23.y, cc23.y, d23.y));
    hits = push_sign(hits, hit_sign(hb23.x, cc23.x, d23.x));
    hits = push_sign(hits, hit_sign(hb01.y, cc01.y, d01.y));
    return push_sign(hits, hit_sign(hb01.x, cc01.x, d01.x));
}

// One pass over the top min(n, nact) entries of a stack (n wave-uniform). kind 0: cand,
// 1: group, 2: node. Lanes ranked past the entries run on their own ray and push nothing.
// kKind 0: cand, 1: group, 2: node. n: this stack's height; pushed: the height of the stack
// this pass pushes onto (group for node passes, cand for group passes).
template <int kKind, int kFmt, bool kGRec, uint32_t kNS, int kSlab, bool kCandInNode = false,
          class WS>
__device__ __forceinline__ void flat_pass(uint32_t& n, uint32_t& pushed, uint32_t nact,
                                          uint32_t rank, uint32_t lane, WS* ws,
                                          const float4* tbound, const float4* tnode, uint32_t ncg,
                                          const GroupTab<kGRec>& tg, const FlatRay& my,
                                          bool slab, uint32_t* rrow = nullptr) {
    using F = FlatFmt<kFmt>;
    using entry_t = typename F::entry_t;
    const uint32_t m = min(n, nact), top = n - m;
    n = top;
    const bool act = rank < m;
    if constexpr (kKind == 2 || kKind == 3) {  // node: the 8 group bounds of (owner, node);
                                               // chunk: the <= 8 node bounds of (owner, chunk)
        uint32_t e = lane << F::kShift;
        if (act) {
            if constexpr (kKind == 2)
                e = ws->node[top + rank];
            else
                e = ws->chunk[top + rank];
        }
        const int src = (int)(e >> F::kShift) << 2;
        BoxRay r;
        const float ix = from_lane(src, my.br.ix.x), iy = from_lane(src, my.br.iy.x),
                    iz = from_lane(src, my.br.iz.x);
        const float cx = from_lane(src, my.br.cx.x), cy = from_lane(src, my.br.cy.x),
                    cz = from_lane(src, my.br.cz.x);
        const float c1 = from_lane(src, my.br.c1.x), c2 = from_lane(src, my.br.c2.x);
        r.ix = (v2f){ix, ix};
        r.iy = (v2f){iy, iy};
        r.iz = (v2f){iz, iz};
        r.cx = (v2f){cx, cx};
        r.cy = (v2f){cy, cy};
        r.cz = (v2f){cz, cz};
        r.c1 = (v2f){c1, c1};
        r.c2 = (v2f){c2, c2};
        // 4 pairs x 80 B: a node's 8 groups, or a chunk's 8 nodes (padded past the last one)
        const float4* gb = (kKind == 2 ? tbound : tnode) + kNS * (e & F::kMask);
        const NearFarAddr na = near_far_addr(gb, ix, iy, iz);
        const uint32_t gout = push_bound_pairs4_nf<kSlab>(r, na, slab);
        uint32_t valid = 0xffu;
        if constexpr (kKind == 3)  // the last chunk may hold fewer than 8 nodes
            valid = (1u << min(8u, (ncg >> 3) - 8u * (e & F::kMask))) - 1u;
        uint32_t need = act ? (~gout & valid) : 0u;
        uint32_t tot;
        uint32_t pos = pushed + wave_prefix<4>((uint32_t)__popc(need), tot, rrow);
        pushed += tot;
        if (need) {
            const uint32_t tag = (e & ~F::kMask) | ((e & F::kMask) << 3);
            do {
                region(rrow, reg::kPushNode);
                const uint32_t k = (uint32_t)__builtin_ctz(need);
                need &= need - 1;
                if constexpr (kKind == 2)
                    ws->group[pos++] = (entry_t)(tag | k);
                else
                    ws->node[pos++] = (entry_t)(tag | k);
            } while (need);
        }
    } else if constexpr (kKind == 1) {  // group: exact test of the 4 members for the owner's ray
        const uint32_t e = act ? (uint32_t)ws->group[top + rank] : (lane << F::kShift);
        uint32_t hits = group_hit_bits<kFmt>(e, tg, my);
        hits = act ? hits : 0u;
        uint32_t tot;
        uint32_t pos = pushed + wave_prefix<3>((uint32_t)__popc(hits), tot, rrow);
        pushed += tot;
        if (hits) {
            const uint32_t tag = e << 2;
            do {
                region(rrow, reg::kPushGroup);
                const uint32_t s = (uint32_t)__builtin_ctz(hits);
                hits &= hits - 1;
                cand_stack<kCandInNode>(ws)[pos++] = (typename F::cand_t)(tag | s);
            } while (hits);
        }
    } else {  // cand: the member's root (its hb, cc, disc recomputed as the packed test did)
        const uint32_t e = act ? cand_stack<kCandInNode>(ws)[top + rank] : (lane << (F::kShift + 2));
        const int src = (int)(e >> (F::kShift + 2)) << 2;
        const float ox = from_lane(src, my.ox), oy = from_lane(src, my.oy), oz = from_lane(src, my.oz);
        const float dx = from_lane(src, my.dx), dy = from_lane(src, my.dy), dz = from_lane(src, my.dz);
        const float a = from_lane(src, my.a), ya = from_lane(src, my.ya);
        const uint32_t s = e & 3u;
        const uint32_t gi = (e >> 2) & F::kMask;
        const float4* g = tg.rec(gi);
        const float4 xy = g[(s >> 1) * 2], zr = g[(s >> 1) * 2 + 1];
        const bool hi = (s & 1u) != 0;
        const float cx = hi ? xy.y : xy.x, cy = hi ? xy.w : xy.z;
        const float cz = hi ? zr.y : zr.x, r2 = hi ? zr.w : zr.z;
        const float ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;
        const float hb = ocx * dx + ocy * dy + ocz * dz;
        const float cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
        const float disc = hb * hb - a * cc;
        const float t = candidate_t_fast(hb, disc, a, ya);
        if (act && t > kMinT && t < kInfinity)
            atomicMin(&ws->key[e >> (F::kShift + 2)], pack_hit(t, tg.index(gi, s)));
    }
}

// A double group pass of the group-footprint scan: the top m = min(n, 2 nact) group entries, for
// nact < n. Lane `rank` tests entry top + rank (m > nact: every live lane has one) and then entry
// top + nact + rank when that lies below m, one after the other on the same registers: only the
// first test's four hit bits and its entry stay live across the second. The eight hit bits take
// one wave prefix and one push loop, a candidate's entry chosen by its bit's half. What one pass
// costs whatever it holds (the guarded read, the prefix, the loop's set-up, flat_drain's
// selection) is paid once for two passes' entries.
template <int kFmt, bool kGRec, class WS>
__device__ __forceinline__ void flat_group_pass2(uint32_t& n, uint32_t& pushed, uint32_t nact,
                                                 uint32_t rank, uint32_t lane, WS* ws,
                                                 const GroupTab<kGRec>& tg, const FlatRay& my,
                                                 uint32_t* rrow = nullptr) {
    using F = FlatFmt<kFmt>;
    const uint32_t m = min(n, 2u * nact), top = n - m;
    n = top;
    const uint32_t e0 = ws->group[top + rank];
    uint32_t hits = group_hit_bits<kFmt>(e0, tg, my);
    // the second entry's index passes through the first test's result (an empty asm), so that
    // nothing of the second test is scheduled into the first and holds registers beside it
    uint32_t i1 = nact + rank;
    asm volatile("" : "+v"(hits), "+v"(i1));
    const bool act = i1 < m;
    const uint32_t e1 = act ? (uint32_t)ws->group[top + i1] : (lane << F::kShift);
    const uint32_t hits1 = group_hit_bits<kFmt>(e1, tg, my);
    hits |= act ? hits1 << 4 : 0u;
    uint32_t tot;
    uint32_t pos = pushed + wave_prefix<4>((uint32_t)__popc(hits), tot, rrow);
    pushed += tot;
    if (hits) {
        const uint32_t tag0 = e0 << 2, tag1 = e1 << 2;
        do {
            region(rrow, reg::kPushGroup);
            const uint32_t s = (uint32_t)__builtin_ctz(hits);
            hits &= hits - 1;
            ws->node[pos++] = (typename F::cand_t)((s < 4u ? tag0 : tag1) | (s & 3u));
        } while (hits);
    }
}

// Runs passes while a stack holds at least `th` entries (th = nact: full passes only; 1: drain).
// Stats builds: wave clock ticks per phase (s_memtime, wave-uniform).
struct PhaseTicks {
    uint64_t scan = 0, levels = 0, node = 0, group = 0, cand = 0, cand_passes = 0, big = 0,
             push = 0, shade = 0, fetch = 0;
    uint64_t pass_entries = 0, pass_lanes = 0, partial_passes = 0, passes = 0;
    uint64_t group_entries = 0, node_entries = 0;  // entries the group / node passes took
    uint64_t cam = 0;  // the camera fast trace with its shading
    // camera fast trace occupancy: entries, camera lanes, live lanes, listed-loop trips and
    // lane sum, root-loop trips and lane sum; main shading hit lanes
    uint64_t cam_entries = 0, cam_lanes = 0, cam_live = 0, list_trips = 0, list_sum = 0,
             root_trips = 0, root_sum = 0, shade_hits = 0;
    // the loop top: wave ticks in the retire, wave-iterations running the fetch loop, block
    // fetches, items started, wave-iterations running the retire, quanta retired (lanes)
    uint64_t retire = 0, fetch_iters = 0, blk_fetches = 0, items_cur = 0, retire_iters = 0,
             quanta = 0;
};

__device__ __forceinline__ uint64_t ticks() { return __builtin_amdgcn_s_memtime(); }

// Stats builds: the per-wave counters (PhaseTicks, trace_impl's st_*) are per lane under SIMT, as
// tally says of the product's -- a lane that is idle when the wave counts keeps its old value,
// and a lane that is done idles through everything after the loop's `if (done) continue` -- so a
// wave-uniform amount x is credited to the wave's first active lane and trace_impl sums each
// counter over the lanes (wave_sum) before lane 0 adds it to TraceParams.debug. (Reading lane
// 0's own count lost every entry made while lane 0 had no item: the camera trace's and the
// scan's counters of a wave's last items.)
__device__ __forceinline__ void credit(uint64_t& c, uint64_t x) {
    const uint32_t first = (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec());
    c += (threadIdx.x & 63u) == first ? x : 0u;
}

__device__ __forceinline__ unsigned long long wave_sum(uint64_t c) {  // every lane active
    unsigned long long v = c;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

struct FlatStacks {  // wave-uniform stack heights
    uint32_t cand, group, node, chunk;
};

// kGroupsOnly: the group-footprint scan (fact (5g)), whose node and chunk stacks stay empty.
template <bool kStats, int kFmt, bool kGRec, uint32_t kNS, int kSlab, bool kGroupsOnly = false,
          class WS>
__device__ __forceinline__ void flat_drain(uint32_t th, uint32_t nact, uint32_t rank, uint32_t lane,
                                           WS* ws, FlatStacks& h,
                                           const float4* tbound, const float4* tnode, uint32_t ncg,
                                           const GroupTab<kGRec>& tg, const FlatRay& my,
                                           uint32_t& n_groups, uint32_t& n_bounds,
                                           PhaseTicks& pt, bool slab, uint32_t* rrow = nullptr) {
    uint32_t nc = h.cand, ng = h.group, nn = h.node, nk = h.chunk;
    for (;;) {
        __builtin_amdgcn_wave_barrier();  // the entries were written by other lanes
        region(rrow, reg::kDrainTrip);
        uint64_t t0 = 0;
        if constexpr (kStats) {
            t0 = ticks();
            const uint32_t n = nc >= nact ? nc : ng >= nact ? ng : nn >= nact ? nn
                             : nk >= nact ? nk
                             : th == 1u ? (nk ? nk : nn ? nn : ng ? ng : nc) : 0u;
            if (n) {
                credit(pt.pass_entries, min(n, nact));
                credit(pt.pass_lanes, nact);
                credit(pt.partial_passes, n < nact);
                credit(pt.passes, 1u);
            }
        }
        // full passes first, deepest stack first; then (final drain only) the partial passes
        // top-down, chunks before nodes before groups before candidates, so that each level's
        // remainder joins the next level's before that one runs: ~3 partial passes per segment
        // instead of a cascade. A pass onto a stack runs only while that stack holds < nact <= 64
        // entries, which keeps the caps (see kNodeCap).
        int kind = -1;
        if (nc >= nact) kind = 0;
        else if (ng >= nact) kind = 1;
        else if (!kGroupsOnly && nn >= nact) kind = 2;
        else if (!kGroupsOnly && nk >= nact) kind = 3;
        else if (th == 1u) kind = !kGroupsOnly && nk ? 3 : !kGroupsOnly && nn ? 2 : ng ? 1 : nc ? 0 : -1;
        if (kind == 0) {
            region(rrow, reg::kPassCand);
            flat_pass<0, kFmt, kGRec, kNS, kSlab>(nc, nc, nact, rank, lane, ws, tbound, tnode, ncg,
                                                  tg, my, slab, rrow);
            if constexpr (kStats) {
                credit(pt.cand, ticks() - t0);
                credit(pt.cand_passes, 1u);
            }
        } else if (kind == 1) {
            region(rrow, reg::kPassGroup);
            ++n_groups;
            if constexpr (kStats && kFmt == 0) credit(pt.group_entries, min(ng, nact));
            flat_pass<1, kFmt, kGRec, kNS, kSlab>(ng, nc, nact, rank, lane, ws, tbound, tnode, ncg,
                                                  tg, my, slab, rrow);
            if constexpr (kStats) credit(pt.group, ticks() - t0);
        } else if (kind == 2) {
            if constexpr (!kGroupsOnly) {
            region(rrow, reg::kPassNode);
            n_bounds += 8;
            if constexpr (kStats && kFmt == 0) credit(pt.node_entries, min(nn, nact));
            flat_pass<2, kFmt, kGRec, kNS, kSlab>(nn, ng, nact, rank, lane, ws, tbound, tnode, ncg,
                                                  tg, my, slab, rrow);
            if constexpr (kStats) credit(pt.node, ticks() - t0);
            }
        } else if (kind == 3) {
            if constexpr (WS::kHasChunks && !kGroupsOnly) {  // (nk stays 0 without the chunk stack)
                region(rrow, reg::kPassChunk);
                n_bounds += 8;
                flat_pass<3, kFmt, kGRec, kNS, kSlab>(nk, nn, nact, rank, lane, ws, tbound,
                                                       tnode, ncg, tg, my, slab, rrow);
                if constexpr (kStats) credit(pt.levels, ticks() - t0);
            }
        } else {
            break;
        }
    }
    h.cand = nc;
    h.group = ng;
    h.node = nn;
    h.chunk = nk;
}

// flat_drain for the group-footprint scan (its kGroupsOnly form: only the group and candidate
// stacks hold anything) with double group passes and the candidates in `node` (see kNodeCap).
// th is 1 or nact, so flat_drain's rule comes down to two scalar compares a trip: a group pass
// while fewer than nact candidates wait and the group stack holds th entries (a drain: any; full
// passes only: nact), else a candidate pass while that stack holds th (nact of them run first
// either way; a drain then takes the remainder), else done. The group pass is a double one where
// the rule would choose a group pass again right after a single one, ng >= nact + th, and counts
// as those two in n_groups and in the stats build's pass counters; between slices (th = nact) it
// takes full halves only, so the remainder joins the next slice as it did.
template <bool kStats, int kFmt, bool kGRec, class WS>
__device__ __forceinline__ void flat_drain_groups(uint32_t th, uint32_t nact, uint32_t rank,
                                                  uint32_t lane, WS* ws, FlatStacks& h,
                                                  const GroupTab<kGRec>& tg, const FlatRay& my,
                                                  uint32_t& n_groups, PhaseTicks& pt,
                                                  uint32_t* rrow = nullptr) {
    static_assert(kFmt == 0, "the candidates' type is the node entries' at kFmt 0");
    uint32_t nc = h.cand, ng = h.group;
    auto count_pass = [&](uint32_t n) {  // the stats build's occupancy of a pass over n entries
        if constexpr (kStats) {
            credit(pt.pass_entries, min(n, nact));
            credit(pt.pass_lanes, nact);
            credit(pt.partial_passes, n < nact);
            credit(pt.passes, 1u);
        }
    };
    for (;;) {
        __builtin_amdgcn_wave_barrier();  // the entries were written by other lanes
        region(rrow, reg::kDrainTrip);
        uint64_t t0 = 0;
        if constexpr (kStats) t0 = ticks();
        if (nc < nact && ng >= th) {
            region(rrow, reg::kPassGroup);
            ++n_groups;
            count_pass(ng);
            if constexpr (kStats) credit(pt.group_entries, min(ng, nact));
            if (kGroupPassDouble && ng >= nact + th) {
                region(rrow, reg::kPassGroup);
                region(rrow, reg::kGroupPass2);
                ++n_groups;
                count_pass(ng - nact);
                if constexpr (kStats) credit(pt.group_entries, min(ng - nact, nact));
                flat_group_pass2<kFmt, kGRec>(ng, nc, nact, rank, lane, ws, tg, my, rrow);
            } else {
                flat_pass<1, kFmt, kGRec, 0u, -1, true>(ng, nc, nact, rank, lane, ws, nullptr,
                                                        nullptr, 0u, tg, my, false, rrow);
            }
            if constexpr (kStats) credit(pt.group, ticks() - t0);
        } else if (nc >= th) {
            region(rrow, reg::kPassCand);
            count_pass(nc);
            flat_pass<0, kFmt, kGRec, 0u, -1, true>(nc, nc, nact, rank, lane, ws, nullptr, nullptr,
                                                    0u, tg, my, false, rrow);
            if constexpr (kStats) {
                credit(pt.cand, ticks() - t0);
                credit(pt.cand_passes, 1u);
            }
        } else {
            break;
        }
    }
    h.cand = nc;
    h.group = ng;
}

// The node mask of one ray from the footprint tables (fact (5); the LDS-table kernel's node
// level): bit k set for every node k whose box test would keep it, and for few others. t0, t1:
// the ray's y interval over all node boxes (the slab's on a slab scene); ddx, ddz: d' of box_axis;
// ft: the four tables in LDS (TraceParams.fp_tab), 32-bit masks when `wide` (wave-uniform).
__device__ __forceinline__ uint32_t foot_cell(float x, const float so[2]) {
    const float f = __builtin_fmaf(x, so[0], so[1]);  // +-inf stays +-inf: scale > 0, offset finite
    return (uint32_t)__builtin_amdgcn_fmed3f(f, 0.0f, (float)(kFootCells - 1u));
}

__device__ __forceinline__ uint32_t foot_mask(const TraceParams& p, const BoxRay& br, float t0,
                                              float t1, float ddx, float ddz, const float4* ft,
                                              bool wide) {
    const float S = __builtin_fmaf(p.fp_k2, br.c2.x, br.c1.x + br.c1.x);
    const float ta = t0 - S, tb = t1 + S;  // t0, t1 finite; S finite or +inf
    // where the line is at ta and at tb (cx, cz finite; d' never 0: no inf - inf, no 0 x inf)
    const float xa = (ta - br.cx.x) * ddx, xb = (tb - br.cx.x) * ddx;
    const float za = (ta - br.cz.x) * ddz, zb = (tb - br.cz.x) * ddz;
    const uint32_t ixa = foot_cell(xa, p.fp_x), ixb = foot_cell(xb, p.fp_x);
    const uint32_t iza = foot_cell(za, p.fp_z), izb = foot_cell(zb, p.fp_z);
    // the cell rises with the coordinate: the footprint's ends are the smaller and larger cell
    const uint32_t x0 = min(ixa, ixb), x1 = max(ixa, ixb), z0 = min(iza, izb), z1 = max(iza, izb);
    uint32_t m;
    if (wide) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(ft);
        m = t[x1] & t[kFootCells + x0] & t[2u * kFootCells + z1] & t[3u * kFootCells + z0];
    } else {
        const uint16_t* t = reinterpret_cast<const uint16_t*>(ft);
        m = (uint32_t)(t[x1] & t[kFootCells + x0] & t[2u * kFootCells + z1] &
                       t[3u * kFootCells + z0]);
    }
    return (tb < ta ? 0u : m) | p.fp_always;
}

// The group mask of one ray from the group-level footprint tables (fact (5g)): foot_mask's cells,
// ta, tb and S over the group boxes, 128-bit masks (bit g = hierarchy group g). gt: the four tables
// of TraceParams.gf_n cells in LDS.
__device__ __forceinline__ uint4 group_foot_mask(const TraceParams& p, const BoxRay& br, float t0,
                                                 float t1, float ddx, float ddz,
                                                 const float4* gt) {
    const float S = __builtin_fmaf(p.gf_k2, br.c2.x, br.c1.x + br.c1.x);
    const float ta = t0 - S, tb = t1 + S;  // t0, t1 finite; S finite or +inf
    const float xa = (ta - br.cx.x) * ddx, xb = (tb - br.cx.x) * ddx;
    const float za = (ta - br.cz.x) * ddz, zb = (tb - br.cz.x) * ddz;
    const uint32_t n = p.gf_n;
    const float last = (float)(n - 1u);
    auto cell = [last](float x, const float so[2]) {
        const float f = __builtin_fmaf(x, so[0], so[1]);
        return (uint32_t)__builtin_amdgcn_fmed3f(f, 0.0f, last);
    };
    const uint32_t ixa = cell(xa, p.gf_x), ixb = cell(xb, p.gf_x);
    const uint32_t iza = cell(za, p.gf_z), izb = cell(zb, p.gf_z);
    const uint32_t x0 = min(ixa, ixb), x1 = max(ixa, ixb), z0 = min(iza, izb), z1 = max(iza, izb);
    const uint4* t = reinterpret_cast<const uint4*>(gt);
    const bool none = tb < ta;  // the ray never reaches the y extent: only `always`
    uint4 m;
    if constexpr (kFootBitop) {
        // such a ray reads the zero row (cell 4 n) for its first row: 0 & b & c & e = 0, so its
        // mask is `always` as the select per word gave it, for one select on an index; and the
        // words as two v_bitop3 each, a & b & c and then (abc & e) | always
        const uint4 a = t[none ? 4u * n : x1], b = t[n + x0], c = t[2u * n + z1],
                    e = t[3u * n + z0];
        auto word = [](uint32_t wa, uint32_t wb, uint32_t wc, uint32_t we, uint32_t always) {
            return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(wa, wb, wc, kBitopAnd3),
                                               we, always, kBitopAndOr);
        };
        m.x = word(a.x, b.x, c.x, e.x, p.gf_always[0]);
        m.y = word(a.y, b.y, c.y, e.y, p.gf_always[1]);
        m.z = word(a.z, b.z, c.z, e.z, p.gf_always[2]);
        m.w = word(a.w, b.w, c.w, e.w, p.gf_always[3]);
        return m;
    }
    const uint4 a = t[x1], b = t[n + x0], c = t[2u * n + z1], e = t[3u * n + z0];
    m.x = (none ? 0u : a.x & b.x & c.x & e.x) | p.gf_always[0];
    m.y = (none ? 0u : a.y & b.y & c.y & e.y) | p.gf_always[1];
    m.z = (none ? 0u : a.z & b.z & c.z & e.z) | p.gf_always[2];
    m.w = (none ? 0u : a.w & b.w & c.w & e.w) | p.gf_always[3];
    return m;
}

// kChunks: the chunk level as per-lane chunk passes over the near/far node boxes `tnode` (many
// chunks: the stress scene), else each lane's node mask from the footprint tables in `tnode`'s
// place (the LDS-table kernel: two chunks at the final scene).
// kSlab: 1 = the boxes share their y extent (kFlagSlab), box tests by the ray's y interval (3a);
// 0 = they do not; -1 = read the flag here and branch at each run of box tests.
// kGroupFoot (the LDS-table kernel with kFlagGroupFoot, fact (5g)): each lane's group mask from
// the group-level tables in `tnode`'s place, pushed straight onto the group stack: no node level,
// no box test (kSlab -1: the flag only says where the ray's y interval comes from).
// The push is capped: a lane with at most kPushCap groups pushes its own (per-word ctz loops);
// the groups of a lane with more (a heavy lane) are dealt across the wave, lane i writing the
// group of bit i of each 64-bit half of the mask. The dead-lane rule: the scan runs with finished
// lanes masked off (exec = live, in 57 % of the final scene's wave-iterations) and a masked-off
// lane writes nothing, so only the bits of `mask & live` go that way; each bit of `mask & ~live`
// is written by the wave's first live lane in a scalar loop. (The other route, dealing those bit
// positions to the live lanes by rank, needs each lane's r-th set bit of a 64-bit mask, about 30
// VALU per half, and a loop of its own once the dead bits outnumber the live lanes -- one live
// lane may stand for 63 dead ones; the scalar loop is bounded by the bits alone.) The entries
// are the same multiset in another order, their total is known before the first write, and the
// choice between the one-step and the sliced push is the one made before the cap.
template <bool kStats, int kFmt, bool kGRec, bool kChunks, uint32_t kNS, int kSlab,
          bool kGroupFoot = false, class WS>
__device__ __forceinline__ void scan_culled_flat(const TraceParams& p, const float4* tbound,
                                                 const float4* tnode,
                                                 const GroupTab<kGRec>& tg, WS* ws,
                                                 const f3 o, const f3 d, bool primary,
                                                 uint32_t item, float& max_t, int& best,
                                                 uint32_t& groups_tested, uint32_t& bounds_tested,
                                                 PhaseTicks& pt, uint32_t* rrow = nullptr) {
    uint64_t t_in = 0;
    if constexpr (kStats) t_in = ticks();
    // the camera-ray list record, loaded ahead of the big list so its latency overlaps it
    uint32_t inf = 15u;
    if (primary && p.prim_info != nullptr)  // the list of the item's 4x4 quarter (slot 8 y + x)
        inf = p.prim_info[2u * ((item >> 6) * 4u + (((item >> 5) & 1u) << 1) + ((item >> 2) & 1u))];
    FlatRay my;
    my.ox = o.x;
    my.oy = o.y;
    my.oz = o.z;
    my.dx = d.x;
    my.dy = d.y;
    my.dz = d.z;
    my.a = dot(d, d);
    my.ya = recip_a(my.a);
    const bool slab = kSlab < 0 ? (p.flags & kFlagSlab) != 0u : kSlab != 0;  // wave-uniform
    my.br = box_ray(p, o, d, my.ya, slab);
    const BoxRay& br = my.br;
    CullRay r;
    r.ox = (v2f){o.x, o.x};
    r.oy = (v2f){o.y, o.y};
    r.oz = (v2f){o.z, o.z};
    {
        const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {my.a, my.a};
        if constexpr (kBigPeel) {
            // The first group apart from the loop (the generated scenes have one): ahead of a
            // loop with a run-time trip count the compiler copies every splat pair, max_t and
            // best into registers of the loop's own (13 v_mov); the peeled test, one basic block
            // (kBigPeel above), reads the ray's scalars through op_sel_hi, as the group passes do.
            // The further groups' loop takes the scalars through an empty asm, so that its pairs
            // are values of its own: one pair shared by both would again be built ahead of both.
            if (p.nbig > 0) {
                exact_group_uniform((cfloat4*)p.cgroup, r, dx, dy, dz, a2, my.a, my.ya, max_t,
                                    best, rrow, reg::kMainBig);
                if (p.nbig > 1) {
                    float lox = o.x, loy = o.y, loz = o.z, ldx = d.x, ldy = d.y, ldz = d.z;
                    float la = my.a;
                    asm("" : "+v"(lox), "+v"(loy), "+v"(loz), "+v"(ldx), "+v"(ldy), "+v"(ldz),
                        "+v"(la));
                    const CullRay lr = {{lox, lox}, {loy, loy}, {loz, loz}};
                    const v2f ex = {ldx, ldx}, ey = {ldy, ldy}, ez = {ldz, ldz}, ea = {la, la};
                    for (int gb = 1; gb < p.nbig; ++gb)
                        exact_group_uniform((cfloat4*)p.cgroup + 5 * gb, lr, ex, ey, ez, ea, la,
                                            my.ya, max_t, best, rrow, reg::kMainBig);
                }
            }
        } else {
        for (int gb = 0; gb < p.nbig; ++gb)  // the big spheres, for every ray (scalar loads)
            exact_group_uniform((cfloat4*)p.cgroup + 5 * gb, r, dx, dy, dz, a2, my.a, my.ya, max_t,
                                best, rrow, reg::kMainBig);
        }
    }
    if constexpr (kStats) credit(pt.big, ticks() - t_in);
    uint32_t n_bounds = 0, n_groups = (uint32_t)p.nbig;
    const uint32_t lane = threadIdx.x & 63u;
    // finished lanes are masked off for the whole scan: entries go to the live lanes by rank
    const uint64_t live = __ballot(1);
    const uint32_t nact = (uint32_t)__popcll(live), rank = lanes_below(live);
    ws->key[lane] = pack_hit(max_t, best);
    FlatStacks h = {0u, 0u, 0u, 0u};
    // A camera ray (primary) whose tile has a group list (primary.cpp) pushes those groups
    // straight onto the group stack and skips the chunk and node levels: the list holds every
    // group such a ray may need (at most 8 per lane: at most 512 entries on the empty stack).
    const bool listed = (inf & 15u) != 15u;
    const uint32_t lcnt = listed ? inf & 15u : 0u, loff = inf >> 4;
    if (__ballot(lcnt != 0u)) {  // the stack height stays wave-uniform: prefix over all lanes
        region(rrow, reg::kListed);
        uint32_t tot;
        uint32_t pos = wave_prefix<4>(lcnt, tot, rrow);
        h.group = tot;
        const uint16_t* ids = p.prim_ids + loff;
        for (uint32_t k = 0; k < lcnt; ++k) {
            region(rrow, reg::kListedTrip);
            ws->group[pos++] =
                (typename FlatFmt<kFmt>::entry_t)((lane << FlatFmt<kFmt>::kShift) | ids[k]);
        }
    }
    cfloat4* node = (cfloat4*)p.cnode;
    cfloat4* top = (cfloat4*)p.ctop;
    const int ncg = p.ncgroups;
    uint32_t tops = 0;
    // (LDS-table kernel) the lane's node mask, once per segment: no box test at the levels
    uint32_t fmask = 0;
    if constexpr (kGroupFoot) {
        using F = FlatFmt<kFmt>;
        using entry_t = typename F::entry_t;
        region(rrow, reg::kLevelGroups);
        uint64_t t0 = 0;
        if constexpr (kStats) t0 = ticks();
        float ty0 = br.iy.x, ty1 = br.cy.x;
        if (!slab) {  // the y interval over the group boxes' one extent, by box_ray's operations
            const float tly = __builtin_fmaf(p.fp_y[0], br.iy.x, br.cy.x);
            const float thy = __builtin_fmaf(p.fp_y[1], br.iy.x, br.cy.x);
            ty0 = fmaxf(fminf(tly, thy), 0.0f);
            ty1 = fmaxf(tly, thy);
        }
        const float ddx = copysignf(fmaxf(fabsf(d.x), 0x1p-40f), d.x);  // d' of box_axis
        const float ddz = copysignf(fmaxf(fabsf(d.z), 0x1p-40f), d.z);
        uint4 gm = group_foot_mask(p, br, ty0, ty1, ddx, ddz, tnode);
        if (listed) gm = make_uint4(0u, 0u, 0u, 0u);  // a listed camera ray has its groups
        const uint32_t cnt = (uint32_t)(__popc(gm.x) + __popc(gm.y) + __popc(gm.z) + __popc(gm.w));
        // Light lanes (at most kPushCap groups) push their own groups, the light entries first;
        // the wave deals each heavy lane's groups across its lanes after them (below). The
        // wave's total, the heavy lanes' counts by scalar adds, is known before anything is
        // written: it chooses between the one-step and the sliced push as it always did.
        const bool heavy = cnt > kPushCap;
        const uint64_t hv = __ballot(heavy);
        uint32_t ltot;
        const uint32_t pre = wave_prefix<kPushBits>(heavy ? 0u : cnt, ltot, rrow);
        uint32_t tot = ltot;
        for (uint64_t m = hv; m; m &= m - 1)
            tot += (uint32_t)__builtin_amdgcn_readlane((int)cnt, __builtin_ctzll(m));
        const uint32_t tag = lane << F::kShift;
        // All lanes' groups in one step when the stack takes them (left over: the lists' entries);
        // else, rarely, a node's worth (8 groups: at most 512 entries) at a time with full passes
        // in between, which keeps the stack bound of the node passes (see kNodeCap): the first
        // slice joins the lists' entries (a lane has a list or a mask: 8 each at most), every
        // later one fewer than nact left over.
        uint32_t slice = 16u;
        if (h.group + tot <= (uint32_t)kGroupCap) {
            entry_t* out = ws->group + (h.group + pre);
            uint32_t base = h.group + ltot;  // the heavy lanes' entries, above the light ones
            h.group += tot;
            // light lanes: one loop per mask word, each with its own region (the stats build
            // counts trips); a wave leaves a loop with its busiest light lane
            if (!heavy) {
                for (uint32_t bits = gm.x; bits; bits &= bits - 1) {
                    region(rrow, reg::kPushGroups0);
                    *out++ = (entry_t)(tag | (uint32_t)__builtin_ctz(bits));
                }
                for (uint32_t bits = gm.y; bits; bits &= bits - 1) {
                    region(rrow, reg::kPushGroups1);
                    *out++ = (entry_t)(tag | 32u | (uint32_t)__builtin_ctz(bits));
                }
                for (uint32_t bits = gm.z; bits; bits &= bits - 1) {
                    region(rrow, reg::kPushGroups2);
                    *out++ = (entry_t)(tag | 64u | (uint32_t)__builtin_ctz(bits));
                }
                for (uint32_t bits = gm.w; bits; bits &= bits - 1) {
                    region(rrow, reg::kPushGroups3);
                    *out++ = (entry_t)(tag | 96u | (uint32_t)__builtin_ctz(bits));
                }
            }
            // heavy lanes, one at a time (wave-uniform): the lane's mask words as scalars, each
            // 64-bit half as a lane mask: lane i writes group 64 half + i, below it the set bits
            // under i (v_mbcnt), a few dozen instructions whatever the lane's count. A masked-off
            // lane cannot write: the bits on dead positions (mask & ~live) go one by one through
            // the wave's first live lane.
            for (uint64_t m = hv; m; m &= m - 1) {
                region(rrow, reg::kPushHeavy);
                const uint32_t hl = (uint32_t)__builtin_ctzll(m);
                const uint32_t w[4] = {(uint32_t)__builtin_amdgcn_readlane((int)gm.x, hl),
                                       (uint32_t)__builtin_amdgcn_readlane((int)gm.y, hl),
                                       (uint32_t)__builtin_amdgcn_readlane((int)gm.z, hl),
                                       (uint32_t)__builtin_amdgcn_readlane((int)gm.w, hl)};
#pragma unroll
                for (uint32_t half = 0; half < 2u; ++half) {
                    const uint64_t hm = ((uint64_t)w[2u * half + 1u] << 32) | w[2u * half];
                    const uint32_t htag = (hl << F::kShift) | (64u * half);
                    const uint64_t on = hm & live;
                    if (__builtin_amdgcn_inverse_ballot_w64(on))
                        ws->group[base + lanes_below(on)] = (entry_t)(htag | lane);
                    base += (uint32_t)__popcll(on);
                    for (uint64_t dead = hm & ~live; dead; dead &= dead - 1) {
                        if (rank == 0u)
                            ws->group[base] = (entry_t)(htag | (uint32_t)__builtin_ctzll(dead));
                        ++base;
                    }
                }
            }
        } else {
            slice = 0u;
        }
        if constexpr (kStats) credit(pt.push, ticks() - t0);
        for (;;) {
            uint32_t th = 1u;  // past the last slice: drain everything
            if (slice < 16u) {
                region(rrow, reg::kSliceGroups);
                th = nact;
                const uint32_t w = slice < 4u ? gm.x : slice < 8u ? gm.y : slice < 12u ? gm.z : gm.w;
                uint32_t bits = (w >> (8u * (slice & 3u))) & 0xffu;
                uint32_t stot;
                uint32_t pos = h.group + wave_prefix<4>((uint32_t)__popc(bits), stot, rrow);
                h.group += stot;
                const uint32_t stag = tag | (8u * slice);
                while (bits) {
                    region(rrow, reg::kPushSlice);
                    const uint32_t k = (uint32_t)__builtin_ctz(bits);
                    bits &= bits - 1;
                    ws->group[pos++] = (entry_t)(stag | k);
                }
                ++slice;
            }
            if constexpr (kGroupPass2)
                flat_drain_groups<kStats, kFmt, kGRec>(th, nact, rank, lane, ws, h, tg, my,
                                                       n_groups, pt, rrow);
            else
                flat_drain<kStats, kFmt, kGRec, kNS, kSlab, true>(th, nact, rank, lane, ws, h,
                                                                  tbound, tnode, (uint32_t)ncg, tg,
                                                                  my, n_groups, n_bounds, pt, slab,
                                                                  rrow);
            if (th == 1u) break;
        }
    } else {
    if constexpr (!kChunks) {
        float ty0 = br.iy.x, ty1 = br.cy.x;
        if (!slab) {  // the y interval over all node boxes, by box_ray's operations (3a)
            const float tly = __builtin_fmaf(p.fp_y[0], br.iy.x, br.cy.x);
            const float thy = __builtin_fmaf(p.fp_y[1], br.iy.x, br.cy.x);
            ty0 = fmaxf(fminf(tly, thy), 0.0f);
            ty1 = fmaxf(tly, thy);
        }
        const float ddx = copysignf(fmaxf(fabsf(d.x), 0x1p-40f), d.x);  // d' of box_axis
        const float ddz = copysignf(fmaxf(fabsf(d.z), 0x1p-40f), d.z);
        fmask = foot_mask(p, br, ty0, ty1, ddx, ddz, tnode, ncg > 128);
        fmask = listed ? 0u : fmask;
    }
    for (int base = 0;; base += 64) {
        uint32_t th = 1u;  // past the last chunk: drain everything
        if (base < ncg) {
            region(rrow, reg::kLevelChunk);
            th = nact;
            uint64_t t0 = 0;
            if constexpr (kStats) t0 = ticks();
            const int nn = min(8, (ncg - base) >> 3);
            uint32_t nodes = 0;
            bool in_chunk;
            if constexpr (kChunks) {
                // level 0, wave-uniform: the chunk's own bound (two chunks per test), per-lane bits
                if ((base & 127) == 0) {
                    region(rrow, reg::kLevelTop);
                    const BoundPair tp = load_bound_pair(top + 4 * (base >> 7));
                    tops = ~(slab ? push_bound_pair<true>(0u, br, tp.b0, tp.b1, tp.b2, tp.b3)
                                  : push_bound_pair<false>(0u, br, tp.b0, tp.b1, tp.b2, tp.b3)) & 3u;
                    n_bounds += 2;
                }
                in_chunk = !listed && ((tops >> ((base >> 6) & 1)) & 1u) != 0;
            } else {
                // the chunk's nodes of the lane's mask (bit = node index = 8 chunk + j)
                nodes = (fmask >> ((uint32_t)base >> 3)) & ((1u << nn) - 1u);
                in_chunk = nodes != 0u;
            }
            const uint64_t want = __ballot(in_chunk);
            if (want == 0) continue;
            region(rrow, reg::kLevelNodes);
            if constexpr (kChunks) {
            // level 1 (many chunks): a chunk entry per lane whose ray may meet the chunk; chunk
            // passes test its nodes for that lane alone
            if (in_chunk)
                ws->chunk[h.chunk + lanes_below(want)] = (typename FlatFmt<kFmt>::entry_t)(
                    (lane << FlatFmt<kFmt>::kShift) | ((uint32_t)base >> 6));
            h.chunk += (uint32_t)__popcll(want);
            if constexpr (kStats) credit(pt.push, ticks() - t0);
            } else {
            // level 1 (LDS tables: two chunks at the final scene): the mask's nodes of this chunk
            // -> node entries (no box test issued: nothing counted)
            if constexpr (kStats) {
                const uint64_t t1 = ticks();
                credit(pt.levels, t1 - t0);
                t0 = t1;
            }
            uint32_t tot;
            uint32_t pos = h.node + wave_prefix<4>((uint32_t)__popc(nodes), tot, rrow);
            h.node += tot;
            if (nodes) {
                const uint32_t tag = (lane << FlatFmt<kFmt>::kShift) | ((uint32_t)base >> 3);
                do {
                    region(rrow, reg::kPushLevel);
                    const uint32_t j = (uint32_t)__builtin_ctz(nodes);
                    nodes &= nodes - 1;
                    ws->node[pos++] = (typename FlatFmt<kFmt>::entry_t)(tag | j);
                } while (nodes);
            }
            if constexpr (kStats) credit(pt.push, ticks() - t0);
            }
        }
        flat_drain<kStats, kFmt, kGRec, kNS, kSlab>(th, nact, rank, lane, ws, h, tbound, tnode,
                                                    (uint32_t)ncg, tg, my, n_groups, n_bounds, pt,
                                                    slab, rrow);
        if (base >= ncg) break;
    }
    }
    __builtin_amdgcn_wave_barrier();
    const unsigned long long k = ws->key[lane];
    max_t = __uint_as_float((uint32_t)(k >> 32));
    best = (int)(uint32_t)k;
    (void)groups_tested;
    (void)bounds_tested;
    tally_lds(&ws->work[1], __builtin_amdgcn_readfirstlane(n_bounds));
    tally_lds(&ws->work[0], 2u * __builtin_amdgcn_readfirstlane(n_groups));  // half-groups
}

template <bool kStats>
__device__ __forceinline__ void scan_culled_lane(const TraceParams& p, const float4* tbound,
                                                 const float4* tgroup, const f3 o, const f3 d,
                                                 float& max_t, int& best,
                                                 uint32_t& groups_tested,
                                                 uint32_t& bounds_tested, uint32_t& lane_cnt,
                                                 uint32_t& rounds) {
    const float a = dot(d, d);
    CullRay r;
    r.ox = (v2f){o.x, o.x};
    r.oy = (v2f){o.y, o.y};
    r.oz = (v2f){o.z, o.z};
    const BoxRay br = box_ray(p, o, d, recip_a(a));
    const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {a, a};
    cfloat4* node = (cfloat4*)p.cnode;
    cfloat4* top = (cfloat4*)p.ctop;
    const int ncg = p.ncgroups;
    for (int gb = 0; gb < p.nbig; ++gb)  // the big spheres, for every ray (scalar loads)
        exact_group_uniform((cfloat4*)p.cgroup + 5 * gb, r, dx, dy, dz, a2, a, recip_a(a), max_t,
                            best);
    // per-segment pass counters, wave-uniform: kept in SGPRs, folded into the 64-bit totals once
    uint32_t n_bounds = 0, n_groups = (uint32_t)p.nbig;
    uint32_t tops = 0;
    for (int base = 0; base < ncg; base += 64) {
        // level 0, wave-uniform: the chunk's own bound (two chunks per test), per-lane bits
        if ((base & 127) == 0) {
            const BoundPair tp = load_bound_pair(top + 4 * (base >> 7));
            tops = ~push_bound_pair(0u, br, tp.b0, tp.b1, tp.b2, tp.b3) & 3u;
            n_bounds += 2;
        }
        const bool in_chunk = ((tops >> ((base >> 6) & 1)) & 1u) != 0;
        if (__ballot(in_chunk) == 0) continue;
        // level 1, wave-uniform: nodes of this chunk, per-lane bits
        const int nn = min(8, (ncg - base) >> 3);
        cfloat4* nb = node + 4 * (base >> 4);
        // sign bits pushed from the last node down, so bit j ends up = node j ruled out
        uint32_t out = 0;
        BoundPair cur = load_bound_pair(nb + 4 * ((nn - 2) >> 1));
        for (int j = nn - 2; j >= 0; j -= 2) {
            const BoundPair nxt = load_bound_pair(nb + 4 * ((j >= 2 ? j - 2 : j) >> 1));
            out = push_bound_pair(out, br, cur.b0, cur.b1, cur.b2, cur.b3);
            cur = nxt;
        }
        uint32_t nodes = in_chunk ? ~out & ((1u << nn) - 1u) : 0u;
        n_bounds += (uint32_t)nn;
        // level 2, per lane: the groups of this lane's nodes
        uint64_t need = 0;
        while (__ballot(nodes != 0)) {
            n_bounds += 8;  // one wave pass = 8 bound tests
            if (nodes) {
                const int j = __builtin_ctz(nodes);
                nodes &= nodes - 1;
                const float4* gb = tbound + 4 * (base >> 1) + __umul24((uint32_t)j, 16u);
                uint32_t gout = 0;
#pragma unroll
                for (int k = 3; k >= 0; k--) {
                    gout = push_bound_pair(gout, br, gb[4 * k], gb[4 * k + 1], gb[4 * k + 2],
                                           gb[4 * k + 3]);
                }
                need |= (uint64_t)(~gout & 0xffu) << (8 * j);
            }
        }
        if constexpr (kStats) lane_cnt += (uint32_t)__popcll(need);
        // the exact test, per lane on its own groups
        while (__ballot(need != 0)) {
            ++n_groups;
            uint32_t cand = 0;  // stats: candidate roots this lane evaluates in this pass
            if (need) {
                const int k = __builtin_ctzll(need);
                need &= need - 1;
                const float4* g = tgroup + 5 * base + __umul24((uint32_t)k, 5u);
                const float4 q0 = g[0], q1 = g[1], q2 = g[2], q3 = g[3], idf = g[4];
                v2f hb01, cc01, d01, hb23, cc23, d23;
                pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, q0, q1, hb01, cc01, d01);
                pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, q2, q3, hb23, cc23, d23);
                const int i0 = __float_as_int(idf.x), i1 = __float_as_int(idf.y),
                          i2 = __float_as_int(idf.z), i3 = __float_as_int(idf.w);
                // bit s = member s may be accepted (sign bits, pushed from member 3 down)
                uint32_t hits = push_sign(0u, hit_sign(hb23.y, cc23.y, d23.y));
                hits = push_sign(hits, hit_sign(hb23.x, cc23.x, d23.x));
                hits = push_sign(hits, hit_sign(hb01.y, cc01.y, d01.y));
                hits = push_sign(hits, hit_sign(hb01.x, cc01.x, d01.x));
                if constexpr (kStats) cand = __popc(hits);
                while (hits) {
                    const int s = __builtin_ctz(hits);
                    hits &= hits - 1;
                    const float hb = s == 0 ? hb01.x : s == 1 ? hb01.y : s == 2 ? hb23.x : hb23.y;
                    const float ds = s == 0 ? d01.x : s == 1 ? d01.y : s == 2 ? d23.x : d23.y;
                    const int idx = s == 0 ? i0 : s == 1 ? i1 : s == 2 ? i2 : i3;
                    consider(candidate_t(hb, ds, a), idx, max_t, best);
                }
            }
            if constexpr (kStats) {  // wave passes of the candidate loop = max over the active
                                     // lanes (<= 4 members; by ballots: idle lanes are inactive)
                rounds += wave_max_small<3>(cand);
            }
        }
    }
    tally(bounds_tested, __builtin_amdgcn_readfirstlane(n_bounds));
    tally(groups_tested, 2u * __builtin_amdgcn_readfirstlane(n_groups));  // half-groups
}

// ---- Accumulation ring ---------------------------------------------------------------------
// Each wave keeps the chunk sums of its current blocks' pixels in LDS: a ring of 32-B entries
// (pixel, three double sums). A block (64 items: all chunks of a few pixels in chunk-minor order)
// takes the next entries of the ring for its pixels, flushing what they held -- partial sums of
// an older block's pixels -- to the pixels' global sums with one f64 atomic per channel; a
// finished item adds its quantized chunk sums to its pixel's entry with LDS atomics (ds_add_f64)
// if the entry still holds that pixel, else straight to the global sums as before. The sums are
// integers below 2^53 (vcrt_math.h "Accumulation"), so every partition of the additions gives
// the same exact total: the image bits do not depend on which additions went through LDS.
// NaN chunk sums add NaN either way. Each wave flushes its ring before it ends.
struct RingEntry {
    uint32_t q;  // local pixel index, ~0: none
    uint32_t pad;
    double s[3];
};
static_assert(sizeof(RingEntry) == 32, "host LDS size");
constexpr uint32_t kQMask = (1u << kRingQBits) - 1u;  // a lane's pixel index without the entry

__device__ __forceinline__ void ring_flush(RingEntry& e, double* accum) {
    if (e.q != ~0u) {
        double* g = accum + 4u * e.q;
        // exact zeros add nothing (+0 + -0 = +0: the sums start at +0); one channel at a time
        // (few registers: this runs in the block fetch, where the whole lane state is live)
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
            const double v = e.s[c];
            if (v != 0.0) atomicAdd(g + c, v);
        }
    }
}

// A ring block's entry for pixel slot `slot` of local tile lt at tile (txy & 0xffff, txy >> 16):
// flushes the entry's old sums, then holds that pixel with zero sums.
__device__ __forceinline__ void ring_claim(RingEntry* ring, uint32_t ei, uint32_t rn,
                                                     double* accum, uint32_t slot, uint32_t lt,
                                                     uint32_t txy, uint32_t width,
                                                     uint32_t height) {
    if (ei >= rn) ei -= rn;
    RingEntry& re = ring[ei];
    ring_flush(re, accum);
    const uint32_t px = 8u * (txy & 0xffffu) + (slot & 7u), py = 8u * (txy >> 16) + (slot >> 3);
    re.q = (slot < 64u && px < width && py < height) ? lt * 64u + slot : ~0u;
    re.s[0] = re.s[1] = re.s[2] = 0.0;
}

// Local element q = 64 * lt + slot of this rank -> pixel (x, y) and its framebuffer index.
struct Pixel {
    uint32_t x, y, out_index;
    bool valid;  // edge tiles of frames that are not multiples of 8 are partial
};

__device__ __forceinline__ Pixel pixel_of(uint32_t q, uint32_t W, uint32_t H, uint32_t tiles_x,
                                          uint32_t world, uint32_t rank) {
    const uint32_t lt = q >> 6, slot = q & 63u;
    uint32_t tx, ty;
    tile_of(lt, rank, world, tiles_x, &tx, &ty);
    Pixel px;
    px.x = 8u * tx + (slot & 7u);
    px.y = 8u * ty + (slot >> 3);
    px.valid = px.x < W && px.y < H;
    px.out_index = world == 1u ? px.y * W + px.x : q;
    return px;
}

// The viewport point's two terms, each one fixed sequence of fp32 operations: shader.comp:43's
// pixel corner pixel00 + x delta_u + y delta_v, and :48-49's jitter in world units
// jx delta_u + jy delta_v (TraceParams.jitter); the sample's point is their sum.
__device__ __forceinline__ f3 viewport_corner(f3 p00, f3 du, f3 dv, uint32_t x, uint32_t y) {
    return add(add(p00, scale((float)x, du)), scale((float)y, dv));
}

__device__ __forceinline__ f3 viewport_jitter(f3 du, f3 dv, float2 jt) {
    return add(scale(jt.x, du), scale(jt.y, dv));
}

// The jitter term of sample i and a hit sphere's shading rows, from the LDS copy the SMEM scan
// stages for small scenes (TraceParams.stage_*), else from global memory.
template <bool kStageable>
__device__ __forceinline__ float4 jitter_at(const TraceParams& p, const float4* lds, int i) {
    if constexpr (kStageable) {
        if (p.stage_spp != 0u) return lds[3u * p.stage_spheres + (uint32_t)i];
    }
    return p.jitter[i];
}

// The lens origin of sample i (TraceParams.lens; the *_lens kernels), staged after the jitter.
template <bool kStageable>
__device__ __forceinline__ float4 lens_at(const TraceParams& p, const float4* lds, int i) {
    if constexpr (kStageable) {
        if (p.stage_spp != 0u) return lds[3u * p.stage_spheres + p.stage_spp + (uint32_t)i];
    }
    return p.lens[i];
}

template <bool kStageable>
__device__ __forceinline__ void shading_rows(const TraceParams& p, const float4* lds, int best,
                                             float4& cr, float4& sh, float4& mat) {
    if constexpr (kStageable) {
        if (p.stage_spp != 0u) {
            const uint32_t ns = p.stage_spheres;
            cr = lds[best];
            sh = lds[ns + best];
            mat = lds[2u * ns + best];
            return;
        }
    }
    cr = p.center_radius[best];
    sh = p.shade[best];
    mat = p.material[best];
}

// kCull: 0 = linear scan (kLds: table in LDS), 1 = culled scan, 2 = per-lane culled scan
// with the group tables copied to LDS, 3 = per-lane culled scan on global tables.
// kLens: the thin lens (vcrt.h lens_radius > 0): a camera ray starts at its sample's lens origin
// (TraceParams.lens) instead of the camera centre; the host then passes no camera-ray lists, so
// the scans treat a camera ray as any other ray.
template <bool kLds, bool kStats, int kCull = 0, bool kCostOrder = false, bool kLens = false>
__device__ __forceinline__ void trace_impl(const TraceParams& p_arg, float4* lds_dyn) {
    // P: the kernel arguments, read through a pointer to the kernarg segment (the kernels' only
    // argument) that the persistent loop makes opaque at the top of every iteration (below), so
    // that the compiler re-reads the arguments it needs (scalar loads from the constant cache)
    // instead of keeping every value derived from them live across the loop. That freed the ~75
    // SGPRs the flat kernel spilled to VGPR lanes (a v_readlane per reload): C4 +2.6%, stress
    // scene +5%, same bits.
    (void)p_arg;
    const TraceParams* pargs = reinterpret_cast<const TraceParams*>(
        (__attribute__((address_space(4))) const TraceParams*)__builtin_amdgcn_kernarg_segment_ptr());
#define P (*pargs)
    const int n = P.nspheres;
    float4* const lds_geom = lds_dyn;
    if constexpr (kLds) {
        const int nq = 4 * (((n + 3) >> 2) + 1);
        for (int i = threadIdx.x; i < nq; i += blockDim.x) lds_geom[i] = P.geom[i];
        __syncthreads();
    }
    // The SMEM scan of a small scene reads the shading rows and the jitter from an LDS copy
    // (TraceParams.stage_*: [stage_spheres] center_radius, shade, material, then the jitter).
    constexpr bool kStageable = kCull == 0 && !kLds;
    if constexpr (kStageable) {
        if (P.stage_spp != 0u) {
            const uint32_t ns = P.stage_spheres;
            for (uint32_t i = threadIdx.x; i < ns; i += blockDim.x) {
                lds_dyn[i] = P.center_radius[i];
                lds_dyn[ns + i] = P.shade[i];
                lds_dyn[2u * ns + i] = P.material[i];
            }
            for (uint32_t i = threadIdx.x; i < P.stage_spp; i += blockDim.x)
                lds_dyn[3u * ns + i] = P.jitter[i];
            if constexpr (kLens) {
                for (uint32_t i = threadIdx.x; i < P.stage_spp; i += blockDim.x)
                    lds_dyn[3u * ns + P.stage_spp + i] = P.lens[i];
            }
            __syncthreads();
        }
    }

    // group-pair boxes: the flat scan reads the near/far layout (80 B per pair), the others
    // the pair-SoA one (64 B)
    constexpr bool kFlat = kCull == 4 || kCull == 5 || kCull == 6;
    const float4* tbound = kFlat ? P.cbound_nf : P.cbound;
    const float4* tnode = P.cnode_nf;              // the flat scans' chunk passes
    const float4* tgroup = P.cgroup + 5 * P.nbig;  // the hierarchy's group records
    // the flat scan's stacks: after the LDS tables (kCull 4: all tables; kCull 6: the boxes,
    // with the group records in global memory), or alone with the tables in global memory and
    // 32-bit entries (kCull 5)
    constexpr int kFmt = kCull == 5 ? 2 : kCull == 6 ? 1 : 0;  // stack entry format
    constexpr bool kGRec = kCull == 5 || kCull == 6;
    constexpr bool kChunks = kCull == 5 || kCull == 6;
    // float4s per node record of the near/far box tables (a node's 8 group boxes, a chunk's 8
    // node boxes: 4 pairs x 80 B): in LDS padded by 16 B, so that the records of nodes n and
    // n + 2 no longer start on the same LDS bank (stride 84 dwords instead of 80: eight start
    // banks for the ds_read2_b64 of a 16-lane group instead of two)
    constexpr uint32_t kNS = (kCull == 4 || kCull == 6) ? 21u : 20u;
    // the flat scans' per-wave stacks (the LDS-table kernel has no chunk level)
    using WS = WaveScratch<kFmt, kChunks>;
    WS* ws = nullptr;
    GroupTab<kGRec> tg{tgroup};  // the flat scans' view of the group records
    if constexpr (kCull == 2) {
        const int nb = (P.ncgroups >> 1) * 4, ng = P.ncgroups * 5;
        for (int i = threadIdx.x; i < nb; i += blockDim.x) lds_geom[i] = tbound[i];
        for (int i = threadIdx.x; i < ng; i += blockDim.x) lds_geom[nb + i] = tgroup[i];
        __syncthreads();
        tbound = lds_geom;
        tgroup = lds_geom + nb;
    }
    if constexpr (kCull == 4) {  // LDS: near/far boxes, 80-B group records with uint16 indices
        const int nb = (P.ncgroups >> 3) * kNS, ng = P.ncgroups * 5;
        // and the node level's footprint tables (fact (5)) after the group records
        const int nf = (int)(foot_lds_bytes(P.ncgroups) >> 4);
        // With kFlagGroupFoot (fact (5g)) the group-level tables, 4 x gf_n float4s, take the place
        // of the boxes and the node tables (the host: 4 gf_n <= nb + nf), ahead of the records.
        const bool gfoot = (P.flags & kFlagGroupFoot) != 0u;
        // (and their zero row, cell 4 gf_n: within nb + nf, or the one float4 nz more)
        const int nz = kFootBitop ? (int)group_foot_zero_pad(P.ncgroups) : 0;
        const int rb = gfoot ? nb + nf + nz : nb;  // where the group records start
        if (gfoot) {
            const float4* gt = reinterpret_cast<const float4*>(P.gf_tab);
            const int nt = min(4 * (int)P.gf_n + (kFootBitop ? 1 : 0), nb + nf + nz);
            for (int i = threadIdx.x; i < nt; i += blockDim.x) lds_geom[i] = gt[i];
        } else {
            uint32_t* ft = reinterpret_cast<uint32_t*>(lds_geom + nb + ng);
            for (int i = threadIdx.x; i < 4 * nf; i += blockDim.x) ft[i] = P.fp_tab[i];
            for (int i = threadIdx.x; i < nb; i += blockDim.x)
                if (i % kNS != 20u) lds_geom[i] = tbound[i - i / kNS];
        }
        for (int i = threadIdx.x; i < ng; i += blockDim.x) {
            float4 v = tgroup[i];
            if (i % 5 == 4) {  // member indices < 2^16 (<= 1024 groups), as uint16 (-1: 0xffff)
                const uint32_t lo = ((uint32_t)__float_as_int(v.x) & 0xffffu) |
                                    ((uint32_t)__float_as_int(v.y) << 16);
                const uint32_t hi = ((uint32_t)__float_as_int(v.z) & 0xffffu) |
                                    ((uint32_t)__float_as_int(v.w) << 16);
                v = make_float4(__uint_as_float(lo), __uint_as_float(hi), 0.0f, 0.0f);
            }
            lds_geom[rb + i] = v;
        }
        __syncthreads();
        tbound = lds_geom;
        tg.geom = lds_geom + rb;
        // (this kernel: the footprint tables, node level or group level)
        tnode = gfoot ? lds_geom : lds_geom + nb + ng;
        ws = reinterpret_cast<WS*>(lds_geom + nb + ng + nf + nz) + (threadIdx.x >> 6);
        static_assert(foot_lds_bytes(128) % 16u == 0u && foot_lds_bytes(256) % 16u == 0u,
                      "whole float4s");
        static_assert(kNS == 21u && sizeof(WS) == kWaveScratchBytes8,
                      "host LDS size (capi.cpp select_kernel)");
    }
    if constexpr (kCull == 5) ws = reinterpret_cast<WS*>(lds_geom) + (threadIdx.x >> 6);
    if constexpr (kCull == 6) {  // LDS: near/far group boxes, near/far node boxes (whole chunks)
        const int nb = (P.ncgroups >> 3) * kNS, nn = ((P.ncgroups + 63) >> 6) * kNS;
        for (int i = threadIdx.x; i < nb; i += blockDim.x)
            if (i % kNS != 20u) lds_geom[i] = tbound[i - i / kNS];
        for (int i = threadIdx.x; i < nn; i += blockDim.x)
            if (i % kNS != 20u) lds_geom[nb + i] = tnode[i - i / kNS];
        __syncthreads();
        tbound = lds_geom;
        tnode = lds_geom + nb;
        ws = reinterpret_cast<WS*>(lds_geom + nb + nn) +
             (threadIdx.x >> 6);
    }
    const uint32_t lane = threadIdx.x & 63u;
    // stats builds: this wave's row of region counters (null in the product: calls fold away)
    uint32_t* rrow = nullptr;
    if constexpr (kStats) {
        if (P.region)
            rrow = P.region + (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * kRegions;
    }
    const f3 p00 = mk(P.cam[0], P.cam[1], P.cam[2]);
    const f3 du = mk(P.cam[3], P.cam[4], P.cam[5]);
    const f3 dv = mk(P.cam[6], P.cam[7], P.cam[8]);
    const f3 cam = mk(P.cam[9], P.cam[10], P.cam[11]);
    const uint32_t nchunks = (uint32_t)P.nchunks;
    const bool reverse = (P.flags & kFlagReverseOrder) != 0;
    const bool chunk_minor = (P.flags & kFlagChunkMinor) != 0;

    bool done = false, need = true;
    bool newray = false;  // the lane's next sample's camera ray is set up at the next fetch
    bool fin = false;  // the lane's quantum is finished and its sum in acc not yet added
    bool fresh = false;  // the lane's ray is a camera ray not yet traced (flat scan)
    // flat scan: a main-scan hit waits for the next iteration's shading (pend_t, pend_best;
    // pend_best < 0: none), which it shares with that iteration's camera rays
    float pend_t = 0.0f;
    int pend_best = -1;  // -1: none; kPendSky: a sky segment
    int sample = 0, sample_end = 0, pass = 0;
    uint32_t q = 0;
    uint32_t pxy = 0;  // the item's pixel: y << 16 | x
    f3 o = mk(0.f, 0.f, 0.f), d = o, atten = o, acc = o;
    // shader.comp:43-52: the camera ray of sample s of the lane's pixel, (corner + jitter) - center,
    // both terms from tables built with the same operations (TraceParams.jitter per sample index,
    // TraceParams.corner per local slot) instead of 25 VALU instructions at every sample start:
    // C4 +1.1%, C3 +1.1% (profiles/r04_ab_log.md). The linear scans (C2: a small, latency-bound
    // frame, -6% with the corner's load) recompute the corner from pxy.
    auto camera_dir = [&](int s) {
        f3 c;
        if constexpr (kCull != 0) {  // the culled scans: the corner from its table
            const float4 c4 = P.corner[q & kQMask];
            c = mk(c4.x, c4.y, c4.z);
        } else {  // the linear scans (small, latency-bound frames): computed, no load
            c = viewport_corner(p00, du, dv, pxy & 0xffffu, pxy >> 16);
        }
        const float4 j = jitter_at<kStageable>(P, lds_dyn, s);
        if constexpr (kLens) {  // (corner + jitter) - origin_s; the ray's origin set here
            const float4 l = lens_at<kStageable>(P, lds_dyn, s);
            o = mk(l.x, l.y, l.z);
            return sub(add(c, mk(j.x, j.y, j.z)), o);
        } else {
            return sub(add(c, mk(j.x, j.y, j.z)), cam);
        }
    };
    uint32_t segs = 0;  // this lane's segments (< 2^32: ~2.4e5 per lane at the C5 workload)
    uint64_t st_iters = 0, st_active = 0, st_hitgroups = 0, st_fetch = 0;
    // issued work (tally): half-groups (sphere-pair tests of the camera lists count one, group
    // tests two) and box tests
    uint32_t w_halves = 0, w_bounds = 0;
    PhaseTicks pt;                         // stats builds: wave clock per phase
    uint64_t t_begin = 0;
    if constexpr (kStats) t_begin = ticks();
#ifdef VCRT_WAVE_END_TIMES
    const unsigned long long t_start_rt = __builtin_amdgcn_s_memrealtime();
    unsigned long long t_drained_rt = ~0ull;
#endif
    // the wave's current block of items (wave-uniform); 64 = exhausted, fetch a new one
    const uint32_t total_blocks = P.total_items >> 6;
    uint32_t blk_next = 64u, blk_lt = 0u, blk_chunk = 0u, blk_tx = 0u, blk_ty = 0u;
    uint32_t q_x = blockIdx.x & (kQueues - 1u), q_drained = 0u;  // the wave's queue; found empty
    uint32_t blk_nch = nchunks;  // chunks per pixel of the block's part (head or tail)
    uint32_t fetch_waited = 0u;  // wave-iterations the fetch was deferred (flat scans)
    bool blk_tail = false;
    // the wave's accumulation ring (see RingEntry): next entry to hand out; the current block's
    // first pixel slot and first entry + 1 (0: the block's items add to global memory)
    RingEntry* const ring =
        P.ring_n ? reinterpret_cast<RingEntry*>(reinterpret_cast<char*>(lds_dyn) + P.ring_off) +
                       __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * P.ring_n
                 : nullptr;
    uint32_t ring_pos = 0u, blk_ps0 = 0u, blk_ring = 0u;
    if (ring) {
        for (uint32_t i = lane; i < P.ring_n; i += 64u) ring[i].q = ~0u;
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (kFlat) {
        if (lane < 2u) ws->work[lane] = 0u;
        __builtin_amdgcn_wave_barrier();
    }

    // Shades a traced segment (textures.glsl, or the sky of functions.glsl:85-89) and advances
    // the lane's path: accumulate and start the next sample's camera ray (returns true), or
    // finish the chunk (need), or continue with the bounced ray.
    // defer_ray: a sample that ends here leaves its next camera ray to the next iteration's fetch
    // (which sets up new items' first rays anyway; used after the main scan, whose lanes trace
    // that ray no earlier than the next camera fast trace)
    auto shade_and_advance = [&](float max_t, int best, bool defer_ray, uint32_t rb) -> bool {
        bool ended = false, fresh_cam = false;
        f3 contrib = mk(0.f, 0.f, 0.f);
        region(rrow, rb + reg::kShEntry);
        if (best >= 0) {
            region(rrow, rb + reg::kShHit);
            float4 cr, sh, mat;
            shading_rows<kStageable>(P, lds_dyn, best, cr, sh, mat);
            const f3 point = add(scale(max_t, d), o);
            // normal = (point - centre) / radius: the unscaled division with one reciprocal
            // (exact: candidate_t_fast's argument) for numerators and radius in [2^-40, 2^30]
            // (the radius by a host flag), else hipcc's full division in a real branch
            const f3 pcv = sub(point, mk(cr.x, cr.y, cr.z));
            const float yr = recip_a(cr.w);
            f3 normal = mk(div_a(pcv.x, cr.w, yr), div_a(pcv.y, cr.w, yr), div_a(pcv.z, cr.w, yr));
            const float nmin = fminf(fminf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
            const float nmax = fmaxf(fmaxf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
            if (!((P.flags & kFlagRadiiSafe) != 0u && nmin >= 0x1p-40f && nmax <= 0x1p30f)) {
                asm volatile("");
                region(rrow, rb + reg::kShNormalDiv);
                normal = divs(pcv, cr.w);
            }
            const int type = (int)mat.x;
            const f3 albedo = mk(sh.x, sh.y, sh.z);
            const float param = sh.w;
            // rand(dir.xy), rand(dir.xz), rand(dir.yz) for lambertian/metal (functions.glsl:43),
            // rand(point.xy) for glass (textures.glsl:51): three sines for every hit lane
            float s1, s2, s3;
            bool sin_fb = false;
            sin3<true>(rand_arg_first(type == 3, point, d),
                       rand_arg(d.x, d.z), rand_arg(d.y, d.z), s1, s2, s3,
                       (cdouble*)&P.sin_c[0], kStats ? &sin_fb : nullptr);
            if constexpr (kStats) {
                if (__ballot(sin_fb)) region(rrow, rb + reg::kShSinFallback);
            }
            const float r1 = rand_of_sin(s1);
            if (type == 1 || type == 2) {
                region(rrow, rb + reg::kShLamMetal);
                const float r2 = rand_of_sin(s2);
                const float r3 = rand_of_sin(s3);
                const f3 ru = mk(r1, r2, r3);  // random_in_unit_sphere(dir): normalize
                const f3 u = unit_of(ru, rrow);
                if (type == 1) {
                    region(rrow, rb + reg::kShLam);
                    d = add(normal, u);
                    atten = scale(param, mul(atten, albedo));
                } else {
                    region(rrow, rb + reg::kShMetal);
                    d = add(reflect(d, normal), scale(param, u));
                    atten = mul(atten, albedo);
                }
                o = point;
            } else if (type == 3) {
                region(rrow, rb + reg::kShGlass);
                const f3 reflected = reflect(d, normal);
                f3 outward;
                float ni, cosine;
                const float dn = dot(d, normal);
                if (dn > 0.0f) {
                    region(rrow, rb + reg::kShGlassIn);
                    outward = neg(normal);
                    ni = param;
                    cosine = sqrt_fast(1.0f - param * param * (1.0f - dn * dn), rrow);
                } else {
                    region(rrow, rb + reg::kShGlassOut);
                    outward = normal;
                    ni = mat.y;  // 1.0f / param
                    cosine = -dn;
                }
                f3 refracted = mk(0.f, 0.f, 0.f);
                float reflect_prob = 1.0f;
                const float dt = dot(d, outward);
                const float disc = 1.0f - ni * ni * (1.0f - dt * dt);
                if (disc > 0.0f) {
                    region(rrow, rb + reg::kShGlassRefract);
                    const float sd = sqrt_fast(disc, rrow);
                    refracted = sub(scale(ni, sub(d, scale(dt, outward))), scale(sd, outward));
                    reflect_prob = schlick_r0(cosine, mat.z);  // schlick(cosine, param)
                }
                o = point;
                d = (r1 < reflect_prob) ? reflected : refracted;
            }
            ++pass;
            if (pass >= P.max_depth) ended = true;  // undefined GLSL return -> vec3(0)
        } else {
            region(rrow, rb + reg::kShSky);
            const float len = sqrt_fast(dot(d, d), rrow);  // length(d)
            contrib = mul(atten, sky_factor(d.y / len));
            ended = true;
        }

        if (ended) {
            region(rrow, rb + reg::kShEnded);
            acc = add(acc, contrib);  // the quantum's fp32 sum in sample order
            ++sample;
            if (sample == sample_end) {
                region(rrow, rb + reg::kShItemEnd);
                // the item is done: its last quantum's sum in acc is retired at the top of the
                // next iteration (few registers are live there: the accumulation code stays out
                // of shading)
                fin = true;
                need = true;
            } else {
                // a quantum of G samples ends inside the item: its sum is retired the same way,
                // and the item goes on with its next sample
                if (((uint32_t)sample & P.quantum_mask) == 0u) fin = true;
                if (defer_ray) {
                    newray = true;
                } else {
                    region(rrow, rb + reg::kShNewRay);
                    d = camera_dir(sample);
                    if constexpr (!kLens) o = cam;
                    atten = mk(1.f, 1.f, 1.f);
                    pass = 0;
                    fresh_cam = true;
                }
            }
        }
        return fresh_cam;
    };

    for (;;) {
        {  // the argument pointer, opaque to the optimiser (an asm result) and wave-uniform
           // (readfirstlane: loads through it stay scalar), in the constant address space
            uint64_t a = reinterpret_cast<uint64_t>(pargs);
            asm volatile("" : "+s"(a));
            const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
            const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
            pargs = reinterpret_cast<const TraceParams*>(
                (__attribute__((address_space(4))) const TraceParams*)(((uint64_t)hi << 32) | lo));
        }
        region(rrow, reg::kIter);
        uint64_t t_top = 0;
        if constexpr (kStats) {
            t_top = ticks();
            const uint64_t fm = __ballot(fin);
            credit(pt.retire_iters, fm != 0u);
            credit(pt.quanta, (uint64_t)__popcll(fm));
        }
        if (fin) {  // ---- retire the finished quantum: its sum to the pixel ----
            region(rrow, reg::kRetire);
            fin = false;
            if constexpr (!kFlat || kCostOrder) {  // the item's segments (the cost order)
                if (P.pixel_cost != nullptr && need) atomicAdd(P.pixel_cost + (q & kQMask), segs);
            }
            if ((P.flags & kFlagDirect) != 0u) {
                // the pixel's one chunk: color /= SPP in fp32 (shader.comp:56)
                const uint32_t out_index =
                    P.world == 1 ? (pxy >> 16) * (uint32_t)P.width + (pxy & 0xffffu) : q & kQMask;
                P.out[out_index] = make_float4(acc.x / P.spp_total, acc.y / P.spp_total,
                                               acc.z / P.spp_total, 1.0f);
            } else {
                // the quantum sum, quantized: RN_even(S * 2^s) (an integer below 2^44), summed
                // exactly over the pixel's quanta in double (vcrt_math.h "Accumulation"). The
                // scale: 2^32 from s + 128 in the flags' top byte (scalar ops, no load), or with
                // kFlagPixelScale the pixel's own from pixel_emax (a wave-uniform branch).
                // (Three compares with |.| modifiers: NaN compares false; the rare cases in a
                // real branch, so the common path converts without selects.)
                float sc = __uint_as_float(
                    ((P.flags >> kFlagScaleShift) + (127u - (uint32_t)kFlagScaleBias)) << 23);
                const uint32_t qi = q & kQMask, ent = q >> kRingQBits;
                if ((P.flags & kFlagPixelScale) != 0u) {
                    asm volatile("");
                    sc = __uint_as_float((uint32_t)(pixel_scale_log2(P.pixel_emax[qi]) + 127) << 23);
                }
                float ax = acc.x * sc, ay = acc.y * sc, az = acc.z * sc;
                if (!(fabsf(ax) < kAccumQLimit && fabsf(ay) < kAccumQLimit &&
                      fabsf(az) < kAccumQLimit)) {
                    asm volatile("");
                    region(rrow, reg::kRetireNan);
                    if (__builtin_isfinite(acc.x) && __builtin_isfinite(acc.y) &&
                        __builtin_isfinite(acc.z)) {
                        // an outlier quantum: its pixel needs a smaller scale; the host renders
                        // the frame again with pixel_emax (this frame's sums are discarded)
                        const uint32_t mb = __float_as_uint(
                            fmaxf(fabsf(acc.x), fmaxf(fabsf(acc.y), fabsf(acc.z))));
                        atomicMax(P.pixel_emax + qi, mb);
                        atomicMax(P.outlier_max, mb);
                    }
                    ax = ay = az = __builtin_nanf("");  // infinite or NaN radiance: a NaN pixel
                }
                const double v0 = (double)__builtin_rintf(ax);
                const double v1 = (double)__builtin_rintf(ay);
                const double v2 = (double)__builtin_rintf(az);
                // the pixel's ring entry while it still holds this pixel (LDS atomics; a claim
                // that takes the entry for another pixel clears the lane's entry field), else
                // global memory (two branches: a pointer that may be either would make flat
                // atomics, whose completion every later LDS wait would wait for)
#ifdef VCRT_KO_RETIRE_ADD  // timing knock-out (wrong image): the quanta computed, not added
                constexpr bool kAdd = false;
                asm volatile("" ::"v"(v0), "v"(v1), "v"(v2), "v"(qi), "v"(ent));
#else
                constexpr bool kAdd = true;
#endif
                if (kAdd && ent != 0u) {
                    region(rrow, reg::kRetireRing);
                    double* s = ring[ent - 1u].s;
                    atomicAdd(s + 0, v0);
                    atomicAdd(s + 1, v1);
                    atomicAdd(s + 2, v2);
                } else if (kAdd) {
                    region(rrow, reg::kRetireGlobal);
                    double* s = P.accum + 4u * qi;
                    atomicAdd(s + 0, v0);
                    atomicAdd(s + 1, v1);
                    atomicAdd(s + 2, v2);
                }
            }
            acc = mk(0.f, 0.f, 0.f);  // the next quantum (of this item or the next) sums from 0
        }
        if (newray) {  // the next sample's camera ray (shader.comp:48-52), deferred by the sky
            region(rrow, reg::kNewRay);
            newray = false;
            d = camera_dir(sample);
            if constexpr (!kLens) o = cam;
            atten = mk(1.f, 1.f, 1.f);
            pass = 0;
            fresh = true;
        }
        // ---- lanes whose item is finished take the next slots of the wave's current block
        //      (one tile x chunk = 64 items); a new block costs one atomic per wave ----
        uint64_t t_fetch = 0;
        if constexpr (kStats) {
            t_fetch = ticks();
            credit(pt.retire, t_fetch - t_top);
        }
        // The loop only hands out slots; the lane state is set up once after it (setting it up
        // inside made the compiler copy ~20 live registers around the loop on every pass).
        bool got = false;
        uint32_t g_lt = 0u, g_chunk = 0u, g_slot = 0u, g_px = 0u, g_py = 0u, g_ent = 0u;
        int g_s0 = -1, g_s1 = 0;  // a stolen sample range (the drain below), else -1
        uint64_t need_mask = __ballot(need && !done);
        if constexpr (kFlat) {
            // deferred fetches (TraceParams.fetch_min / fetch_wait): while fewer than fetch_min
            // lanes need an item and other lanes still have work, the wave skips the fetch for up
            // to fetch_wait iterations (the waiting lanes idle; the fetch runs for more at once)
            if (need_mask != 0u) {
                if ((uint32_t)__popcll(need_mask) < P.fetch_min && fetch_waited < P.fetch_wait &&
                    __ballot(!need && !done) != 0u) {
                    ++fetch_waited;
                    need_mask = 0u;
                } else {
                    fetch_waited = 0u;
                }
            }
        }
        if constexpr (kStats) credit(pt.fetch_iters, need_mask != 0u);
        while (need_mask) {
            region(rrow, reg::kFetchTrip);
            if (blk_next >= 64u) {
                if constexpr (kStats && kCull == 0) credit(st_fetch, 1u);
                // kQueues queues, each on workgroups of one XCD (workgroups are dispatched to
                // the XCDs round robin): queue x hands out blocks kQueues k + x on its own
                // counter; a wave whose queue is drained moves on to the next open one, and is
                // done when it has found every queue drained
                uint32_t b = ~0u;
                while (b == ~0u && q_drained < kQueues) {
                    const int leader = __ffsll((unsigned long long)__ballot(1)) - 1;
                    const uint32_t nq = (total_blocks + kQueues - 1u - q_x) / kQueues;
                    uint32_t k = 0;
                    const uint32_t amt = 1u;
                    if ((int)lane == leader) k = atomicAdd(P.work + kQueueStride * q_x, amt);
                    k = __builtin_amdgcn_readfirstlane(__shfl(k, leader));
                    if (k < nq) {
                        b = kQueues * k + q_x;
                        break;
                    }
#ifdef VCRT_OLD_DRAIN
                    ++q_drained;
                    q_x = (q_x + 1u) & (kQueues - 1u);
#else
                    // this queue is drained: read every queue's counter at once (one load per
                    // lane; a counter only grows, so "drained" read here is final) and move to
                    // the next open queue after q_x, or finish when none is open. (Trying the
                    // queues one atomic at a time made every wave of the grid issue kQueues
                    // serialized atomics on the same kQueues counters at the end of a frame:
                    // ~0.25 ms of tail per launch.)
                    const uint64_t act = __ballot(1);
                    const uint32_t na = (uint32_t)__popcll(act), rk = lanes_below(act);
                    uint32_t best = 0u;  // kQueues - (distance of the nearest open queue)
                    for (uint32_t base = 0; base < kQueues; base += na) {
                        const uint32_t dq = base + rk + 1u;  // distance from q_x: 1 .. kQueues
                        uint32_t v = 0u;
                        if (dq <= kQueues) {
                            const uint32_t qq = (q_x + dq) & (kQueues - 1u);
                            const uint32_t cnt = __hip_atomic_load(P.work + kQueueStride * qq,
                                                                   __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_AGENT);
                            const uint32_t nqq = (total_blocks + kQueues - 1u - qq) / kQueues;
                            if (cnt < nqq) v = kQueues + 1u - dq;
                        }
                        best = max(best, wave_max_small<6>(v));
                    }
                    // (each failed atomic is on a queue that then reads drained: at most
                    // kQueues of them per wave, as before)
                    ++q_drained;
                    if (best == 0u) {
                        q_drained = kQueues;
                    } else {
                        q_x = (q_x + (kQueues + 1u - best)) & (kQueues - 1u);
                    }
#endif
                }
                if (b == ~0u) {  // queues drained: lanes still wanting work are done
#ifdef VCRT_WAVE_END_TIMES
                    if (t_drained_rt == ~0ull) t_drained_rt = __builtin_amdgcn_s_memrealtime();
#endif
                    if (need) done = true;
                    break;
                }
                if constexpr (kStats) credit(pt.blk_fetches, 1u);
                region(rrow, reg::kBlock);
                // block b = (local tile lt, chunk) of the head, then of the tail: wave-uniform
                // tile origin and sample range; reversed within each part
                if constexpr (!kFlat || kCostOrder) {  // cost order (any part; a scalar load)
                    if (P.block_order != nullptr)
                        b = ((__attribute__((address_space(4))) const uint32_t*)P.block_order)[b];
                }
                blk_tail = b >= P.blocks_head;
                if (blk_tail) b -= P.blocks_head;
                if (reverse) b = (blk_tail ? total_blocks - P.blocks_head : P.blocks_head) - 1u - b;
                blk_nch = blk_tail ? (uint32_t)P.tail_nchunks : nchunks;
                blk_lt = b / blk_nch;
                blk_chunk = b - blk_lt * blk_nch;
                tile_of(blk_lt, (uint32_t)P.rank, (uint32_t)P.world, P.tiles_x, &blk_tx, &blk_ty);
                blk_next = 0u;
                // ring entries for the block's pixel slots ps0 .. ps1 (chunk-minor items
                // 64 c .. 64 c + 63 of the tile are (i / nch, i % nch)): flushed and set up by
                // one lane each (the loop top runs with every lane of the wave)
                blk_ring = 0u;
                if (ring && chunk_minor && __builtin_amdgcn_read_exec() == ~0ull) {
                    const uint32_t ps0 = (64u * blk_chunk) / blk_nch;
                    const uint32_t np = (64u * blk_chunk + 63u) / blk_nch - ps0 + 1u;
                    if (np <= P.ring_n) {
                        region(rrow, reg::kBlockRing);
                        if (lane < np)
                            ring_claim(ring, ring_pos + lane, P.ring_n, P.accum, ps0 + lane,
                                       blk_lt, (blk_ty << 16) | blk_tx, (uint32_t)P.width,
                                       (uint32_t)P.height);
                        __builtin_amdgcn_wave_barrier();
                        // a lane whose item's entry is among those just claimed (its own, or
                        // the one of an item handed to it earlier in this fetch) loses it: the
                        // item's later quanta go to global memory
                        const uint32_t rn = P.ring_n, pos = ring_pos;
                        auto keep = [rn, pos, np](uint32_t ent) {
                            uint32_t rel = ent + rn - 1u - pos;
                            if (rel >= rn) rel -= rn;
                            return (ent != 0u && rel < np) ? 0u : ent;
                        };
                        q = (q & kQMask) | (keep(q >> kRingQBits) << kRingQBits);
                        g_ent = keep(g_ent);
                        blk_ps0 = ps0;
                        blk_ring = ring_pos + 1u;
                        ring_pos += np;
                        if (ring_pos >= P.ring_n) ring_pos -= P.ring_n;
                    }
                }
            }
            const uint32_t avail = 64u - blk_next;
            const uint32_t mine = lanes_below(need_mask);
            if (need && !done && mine < avail) {
                uint32_t slot = blk_next + mine, ch = blk_chunk;
                if (chunk_minor) {  // item 64 j + slot of the tile = (pixel, chunk), chunk-minor
                    // i / n by the host's magic multiplier (exact for every i < 64 n, checked
                    // by the host; 0: none): C4 8-way shards -1% against hipcc's division
#ifdef VCRT_NO_MAGIC
                    const uint32_t m = 0u;
#else
                    const uint32_t m = blk_tail ? P.nch_magic[1] : P.nch_magic[0];
#endif
                    const uint32_t i = 64u * blk_chunk + slot;
                    if (m != 0u) {
                        slot = __umulhi(i, m);
                    } else {
                        asm volatile("");
                        slot = i / blk_nch;
                    }
                    ch = i - slot * blk_nch;
                }
                if (blk_tail) ch |= 0x10000u;  // chunk ch of the tail
                const uint32_t px = 8u * blk_tx + (slot & 7u), py = 8u * blk_ty + (slot >> 3);
                if (px < (uint32_t)P.width && py < (uint32_t)P.height) {  // edge tiles: skip
                    got = true;
                    g_lt = blk_lt;
                    g_chunk = ch;
                    g_slot = slot;
                    g_px = px;
                    g_py = py;
                    need = false;
                    g_ent = 0u;
                    if (blk_ring) {  // the pixel's ring entry (+ 1)
                        uint32_t ei = blk_ring + (slot - blk_ps0);
                        if (ei > P.ring_n) ei -= P.ring_n;
                        g_ent = ei;
                    }
                }
            }
            blk_next += min((uint32_t)__popcll(need_mask), avail);
            need_mask = __ballot(need && !done);
        }
#ifndef VCRT_NO_STEAL
        // ---- the drain: once every queue is empty, an idle lane takes the later quanta of
        //      the wave's longest remaining item (the victim keeps the quantum in progress and
        //      half of the rest). Quanta are summed on their own and added exactly, so any lane
        //      may trace any whole quantum of a pixel: the same bits, the same segments. ----
        if (q_drained >= kQueues && (P.flags & kFlagDirect) == 0u) {
            uint64_t idle = __ballot(done);
            if (idle != 0u) {
                const int gm = (int)P.quantum_mask, G = gm + 1;
                uint32_t rem = 0u;  // whole quanta after the one in progress
                if (!done && !need) {
                    const int next = (sample & ~gm) + G;
                    if (sample_end > next) rem = (uint32_t)((sample_end - next + gm) / G);
                }
                while (idle != 0u) {
                    region(rrow, reg::kSteal);
                    const uint32_t top = wave_max_small<10>(rem);  // <= kAccumMaxChunks
                    if (top == 0u) break;
                    const uint32_t victim = (uint32_t)__builtin_ctzll(__ballot(rem == top));
                    const uint32_t thief = (uint32_t)__builtin_ctzll(idle);
                    idle &= idle - 1u;
                    const uint32_t give = (top + 1u) >> 1;
                    const int v_sample = __builtin_amdgcn_readlane(sample, victim);
                    const int v_end = __builtin_amdgcn_readlane(sample_end, victim);
                    const uint32_t v_q = __builtin_amdgcn_readlane(q, victim);
                    const uint32_t v_pxy = __builtin_amdgcn_readlane(pxy, victim);
                    const int cut = (v_sample & ~gm) + G * (int)(1u + top - give);
                    if (lane == victim) {
                        sample_end = cut;
                        rem = top - give;
                    }
                    if (lane == thief) {
                        got = true;
                        done = false;
                        need = false;
                        g_lt = (v_q & kQMask) >> 6;
                        g_slot = v_q & 63u;
                        g_ent = v_q >> kRingQBits;
                        g_px = v_pxy & 0xffffu;
                        g_py = v_pxy >> 16;
                        g_s0 = cut;
                        g_s1 = v_end;
                        // no victim before its range is set up (the got block below): its
                        // sample / sample_end / q still name the item it finished
                        rem = 0u;
                    }
                }
            }
        }
#endif
        if constexpr (kStats) credit(pt.items_cur, (uint64_t)__popcll(__ballot(got)));
        if (got) {
            region(rrow, reg::kItem);
            q = (g_lt * 64u + g_slot) | (g_ent << kRingQBits);
            pxy = (g_py << 16) | g_px;
            if constexpr (!kFlat || kCostOrder) {
                if (P.pixel_cost != nullptr) atomicSub(P.pixel_cost + g_lt * 64u + g_slot, segs);
            }
            // the item's samples: the four partition values are wave-uniform, read by scalar
            // loads and selected per lane (left to itself the compiler selected their kernarg
            // addresses per lane and read them with vector loads, whose latency the jitter
            // load's address then waited for: two dependent memory round trips per fetch)
            const bool tail = g_chunk >= 0x10000u;
#ifdef VCRT_NO_SCALAR_PART
            const int k_head = P.chunk, k_tail = P.tail_chunk, t_start = P.tail_start,
                      n_spp = P.spp;
#else
            const int k_head = __builtin_amdgcn_readfirstlane(P.chunk);
            const int k_tail = __builtin_amdgcn_readfirstlane(P.tail_chunk);
            const int t_start = __builtin_amdgcn_readfirstlane(P.tail_start);
            const int n_spp = __builtin_amdgcn_readfirstlane(P.spp);
#endif
            const int k = tail ? k_tail : k_head;
            sample = (tail ? t_start : 0) + (int)(g_chunk & 0xffffu) * k;
            sample_end = min(sample + k, tail ? n_spp : t_start);
#ifndef VCRT_NO_STEAL
            if (g_s0 >= 0 && g_s0 < g_s1) {  // a stolen range of whole quanta (never empty)
                sample = g_s0;
                sample_end = g_s1;
            }
#endif
            // first camera ray of the chunk, shader.comp:48-52
            d = camera_dir(sample);
            if constexpr (!kLens) o = cam;
            atten = mk(1.f, 1.f, 1.f);
            pass = 0;
            fresh = true;
        }
        if constexpr (kStats) credit(pt.fetch, ticks() - t_fetch);
        const uint64_t live = __ballot(!done);
        if (live == 0) break;
        if constexpr (kStats) {
            credit(st_iters, 1u);
            credit(st_active, (uint64_t)__popcll(live));
        }
        if (done) continue;

        // ---- flat scan: a camera ray not yet traced (started by the last shading or by the
        //      fetch) is traced first, from its pixel quarter's group list (the big list, then
        //      the listed groups, per lane, with hit_sphere's consider rule: the same sphere
        //      and t as the flat scan), and shaded; the lane then takes its first bounce
        //      through this iteration's scan. The per-wave costs of an iteration (uniform
        //      levels, ray setup, block fetch) are so shared by two segments of such lanes. ----
        if constexpr (kFlat) {
            uint64_t t_cam = 0;
            if constexpr (kStats) t_cam = ticks();
            uint32_t inf = 15u;
            // (kLens: the rays do not share an origin, so no lists and no fast trace)
            if constexpr (!kLens) {
                if (fresh && P.prim_info != nullptr)  // the sphere list of the item's 4x4 quarter
                    inf = P.prim_info[2u * (((q & kQMask) >> 6) * 4u + (((q >> 5) & 1u) << 1) +
                                            ((q >> 2) & 1u)) +
                                      1u];
            }
            const float aa = dot(d, d);
#ifdef VCRT_OLD_GUARDS
            const bool cam_now = !kLens && fresh && (inf & 15u) != 15u &&
                                 (P.flags & kFlagSceneBounded) != 0 && aa >= 0x1p-20f &&
                                 aa <= 0x1p60f && fabsf(o.x) <= 0x1p30f &&
                                 fabsf(o.y) <= 0x1p30f && fabsf(o.z) <= 0x1p30f;
#else
            // (a fresh ray of a pinhole frame starts at the camera centre: the origin's range
            // test and the scene's bound are the host's, which hands out the lists, prim_info,
            // only to a frame that passes both: no flag to load, no compare on o here)
            const bool cam_now = !kLens && fresh && (inf & 15u) != 15u && guard_a(aa);
#endif
            float mt = __uint_as_float(vconst<0x47c35000u>());  // kInfinity
            int bst = (int)vconst<0xffffffffu>();                // -1
            if (__ballot(cam_now)) {
                region(rrow, reg::kCam);
                if constexpr (kStats) {
                    credit(pt.cam_entries, 1u);
                    credit(pt.cam_lanes, (uint64_t)__popcll(__ballot(cam_now)));
                    credit(pt.cam_live, (uint64_t)__popcll(__ballot(1)));
                }
                uint32_t iters = 0, roots = 0;
                if (cam_now) {
                    ++segs;
                    #ifdef VCRT_COST_MAP  // diagnostics: segments per pixel in the sums' unused fourth channel
                    atomicAdd(P.accum + 4u * (q & kQMask) + 3u, 1.0);
                    #endif
                    // A camera ray starts at the camera centre: its spheres' oc and cc come from
                    // camera-relative records (pair_disc_cam: same bits, half the arithmetic of
                    // pair_disc_cc); the roots take candidate_t_fast.
                    cfloat4* crec = (cfloat4*)P.cam_rec;
                    const float ya = recip_a(aa);
                    const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {aa, aa};
                    if constexpr (kBigPeel) {  // the first group apart (see scan_culled_flat)
                        if (P.nbig > 0) {
                            exact_group_uniform_cam(crec, (cfloat4*)P.cgroup, dx, dy, dz, a2, aa,
                                                    ya, mt, bst, rrow, reg::kCamBig);
                            for (int gb = 1; gb < P.nbig; ++gb) {  // the further groups
                                exact_group_uniform_cam(crec + 4 * gb, (cfloat4*)P.cgroup + 5 * gb,
                                                        dx, dy, dz, a2, aa, ya, mt, bst, rrow,
                                                        reg::kCamBig);
                            }
                        }
                    } else {
                    for (int gb = 0; gb < P.nbig; ++gb)  // the big spheres (scalar loads)
                        exact_group_uniform_cam(crec + 4 * gb, (cfloat4*)P.cgroup + 5 * gb, dx, dy,
                                                dz, a2, aa, ya, mt, bst, rrow, reg::kCamBig);
                    }
                    // the quarter's listed spheres, two per record (primary.cpp): the exact
                    // test's may-hit bits are collected first (bit 2k + s)...
                    const uint32_t cnt = inf & 15u;
                    const float4* lr = P.cam_rec + 4u * (uint32_t)P.nbig + 3u * (inf >> 4);
                    uint32_t cbits = 0u;
                    for (uint32_t k = 0; 2u * k < cnt; ++k) {
                        region(rrow, reg::kCamListTrip);
                        ++iters;
                        const float4 q0 = lr[3u * k], q1 = lr[3u * k + 1u];
                        v2f hb, cc, dc;
                        pair_disc_cam(dx, dy, dz, a2, q0, q1, hb, cc, dc);
                        const uint32_t hits = push_sign(push_sign(0u, hit_sign(hb.y, cc.y, dc.y)),
                                                        hit_sign(hb.x, cc.x, dc.x));
                        cbits |= hits << (2u * k);
                    }
                    // ...then the candidates' roots, one per lane and loop trip (the wave runs
                    // as many trips as its busiest lane has candidates, mostly one), with the
                    // sphere's hb and disc recomputed by the same operations (measured: both
                    // members' roots packed in the first loop issue more VALU, +1.8%)
                    while (cbits) {
                        region(rrow, reg::kCamRootTrip);
                        const uint32_t b = (uint32_t)__builtin_ctz(cbits);
                        cbits &= cbits - 1u;
                        const float4* c = lr + 3u * (b >> 1);
                        const float4 xy = c[0], zc = c[1], id = c[2];
                        const bool hi = (b & 1u) != 0;
                        const float ocx = hi ? xy.y : xy.x, ocy = hi ? xy.w : xy.z;
                        const float ocz = hi ? zc.y : zc.x, cc = hi ? zc.w : zc.z;
                        const float hb = ocx * d.x + ocy * d.y + ocz * d.z;
                        const float disc = hb * hb - aa * cc;
                        consider(candidate_t_fast(hb, disc, aa, ya, rrow),
                                 __float_as_int(hi ? id.y : id.x), mt, bst);
                        ++roots;
                    }
                }
                if constexpr (kStats) {
                    // done lanes are inactive here, so no xor butterfly (a partial result that
                    // passes through an inactive lane is lost): each lane adds its own trips to
                    // its own counter, which wave_sum totals after the loop, and the maxima
                    // come from ballots (a listed quarter has <= 14 spheres: <= 7 pairs)
                    pt.list_sum += iters;
                    pt.root_sum += roots;
                    credit(pt.list_trips, wave_max_small<3>(iters));
                    credit(pt.root_trips, wave_max_small<4>(roots));
                }
                // issued work: the big list and the loop's passes (a pair test is half a group
                // test), per wave
                tally_lds(&ws->work[0], 2u * (uint32_t)P.nbig + wave_max_small<3>(iters));
            }
            // One shading for the camera rays just traced and the main-scan hits of the last
            // iteration: the hit branches run once per iteration for both (a lane has at most
            // one of them; each lane's own sequence of operations is unchanged).
            const bool pending = pend_best != -1;
            if (pending) {
                mt = pend_t;
                bst = pend_best >= 0 ? pend_best : -1;  // kPendSky: the sky
                pend_best = -1;
            }
            uint64_t t_cs = 0;
            if constexpr (kStats) t_cs = ticks();
            if (cam_now || pending) {
                region(rrow, reg::kShadeCam);
                fresh = shade_and_advance(mt, bst, false, reg::kShadeBase0);
            }
            if constexpr (kStats) {
                const uint64_t t1 = ticks();
                credit(pt.cam, t1 - t_cam);
                credit(st_fetch, t1 - t_cs);  // flat stats: debug[3] = the camera phase's shading
            }
            if (need) continue;  // that segment finished the lane's chunk
        }

        // ---- one segment: scan the whole sphere list (functions.glsl:73-81) ----
        ++segs;
        #ifdef VCRT_COST_MAP  // diagnostics: segments per pixel in the sums' unused fourth channel
        atomicAdd(P.accum + 4u * (q & kQMask) + 3u, 1.0);
        #endif
        float max_t = __uint_as_float(vconst<0x47c35000u>());  // kInfinity
        int best = (int)vconst<0xffffffffu>();                   // -1
        uint32_t hit_groups = 0;
        if constexpr (kCull != 0) {
            // culling needs every ray of the wave in the guarded finite range (see above)
            const float aa = dot(d, d);
#ifdef VCRT_OLD_GUARDS
            const bool guarded = (P.flags & kFlagSceneBounded) != 0 && aa >= 0x1p-20f &&
                                 aa <= 0x1p60f && fabsf(o.x) <= 0x1p30f &&
                                 fabsf(o.y) <= 0x1p30f && fabsf(o.z) <= 0x1p30f;
#else
            const bool guarded = (P.flags & kFlagSceneBounded) != 0 && guard_a(aa) && guard_o(o);
#endif
            if (__ballot(!guarded) == 0) {
                region(rrow, reg::kScan);
                uint32_t lane_cnt = 0;
                uint64_t t0 = 0;
                if constexpr (kStats) t0 = ticks();
                if constexpr (kCull == 1)
                    scan_culled<kStats>(P, o, d, max_t, best, w_halves, w_bounds, hit_groups,
                                        lane_cnt);
                else if constexpr (kFlat) {
                    // Where the slab flag (wave-uniform) branches, chosen per kernel from the
                    // register allocation each form gets (the spill counts of the code object's
                    // notes): the LDS-table kernel holds the whole scan twice, one branch per
                    // segment; the other two branch around each run of four box pairs (the scan
                    // twice costs the global-table kernel 6 more VGPR spills, the branch per run
                    // costs the LDS-table kernel 4).
                    if constexpr (kCull != 4 && !(kCull == 6 && VCRT_SLAB_BOXES_SCAN))
                        scan_culled_flat<kStats, kFmt, kGRec, kChunks, kNS, -1>(
                            P, tbound, tnode, tg, ws, o, d, pass == 0, q & kQMask, max_t, best,
                            w_halves, w_bounds, pt, rrow);
                    else if (kCull == 4 && (P.flags & kFlagGroupFoot) != 0u)
                        scan_culled_flat<kStats, kFmt, kGRec, kChunks, kNS, -1, kCull == 4>(
                            P, tbound, tnode, tg, ws, o, d, pass == 0, q & kQMask, max_t, best,
                            w_halves, w_bounds, pt, rrow);
                    else if ((P.flags & kFlagSlab) != 0u)
                        scan_culled_flat<kStats, kFmt, kGRec, kChunks, kNS, 1>(
                            P, tbound, tnode, tg, ws, o, d, pass == 0, q & kQMask, max_t, best,
                            w_halves, w_bounds, pt, rrow);
                    else
                        scan_culled_flat<kStats, kFmt, kGRec, kChunks, kNS, 0>(
                            P, tbound, tnode, tg, ws, o, d, pass == 0, q & kQMask, max_t, best,
                            w_halves, w_bounds, pt, rrow);
                }
                else
                    scan_culled_lane<kStats>(P, tbound, tgroup, o, d, max_t, best, w_halves,
                                             w_bounds, lane_cnt, hit_groups);
                if constexpr (kStats) credit(pt.scan, ticks() - t0);
                if constexpr (kStats) {  // CULL stats: debug[3] = sum of per-wave max lane need
                    // (the maximum by ballots: done lanes are inactive here, which an xor
                    // butterfly does not survive)
                    if constexpr (!kFlat) credit(st_fetch, wave_max_small<32>(lane_cnt));
                }
            } else {
                region(rrow, reg::kScanLinear);
                scan_spheres<false>(P, lds_geom, n, o, d, max_t, best, hit_groups);
                if constexpr (kFlat)
                    tally_lds(&ws->work[0], 2u * (uint32_t)((n + 3) >> 2));
                else
                    tally(w_halves, 2u * (uint32_t)((n + 3) >> 2));
            }
        } else {
            scan_spheres<kLds>(P, lds_geom, n, o, d, max_t, best, hit_groups);
            tally(w_halves, 2u * (uint32_t)((n + 3) >> 2));
        }
        if constexpr (kStats) credit(st_hitgroups, hit_groups);

        // ---- shade (textures.glsl) or sky (functions.glsl:85-89) ----
        uint64_t t_shade = 0;
        if constexpr (kStats) {
            t_shade = ticks();
            credit(pt.shade_hits, (uint64_t)__popcll(__ballot(best >= 0)));
        }
        if constexpr (kFlat) {
            // a hit is shaded with the next iteration's camera rays; so is the sky of a lane
            // whose quantum ended in this iteration's camera phase (its sum in acc awaits the
            // retire, so no second sample may end before it)
            if (best >= 0 || fin) {
                pend_t = max_t;
                pend_best = best >= 0 ? best : kPendSky;
                fresh = false;  // the ray is traced (it may have been a camera ray)
            } else {
                region(rrow, reg::kShadeSkyMain);
                fresh = shade_and_advance(max_t, best, true, reg::kShadeBase1);  // the sky
            }
        } else {
            fresh = shade_and_advance(max_t, best, false, reg::kShadeBase0);
        }
        if constexpr (kStats) credit(pt.shade, ticks() - t_shade);

    }

#ifdef VCRT_WAVE_END_TIMES  // diagnostics builds (VCRT_DEBUG_STATS=2): when waves start, end,
                            // and see the queue drained (s_memrealtime, 100 MHz)
    if (!kStats && lane == 0 && P.debug) {
        const unsigned long long t = __builtin_amdgcn_s_memrealtime();
        atomicMax(P.debug + 4, t);
        atomicMin(P.debug + 5, t);
        atomicAdd(P.debug + 6, t >> 8);
        atomicAdd(P.debug + 7, 1ull);
        atomicMin(P.debug + 9, t_start_rt);
        atomicMin(P.debug + 10, t_drained_rt);
        atomicAdd(P.debug + 11, t_drained_rt >> 8);
        // wave lifetimes in 0.1 ms buckets (debug 12..27, the last open-ended) and how long
        // the wave ran on after it saw the queue drained (28..31: < 0.1, < 0.3, < 0.6 ms, more)
        const unsigned long long life = (t - t_start_rt) / 10000ull;
        atomicAdd(P.debug + 12 + (life < 15ull ? life : 15ull), 1ull);
        const unsigned long long after = t_drained_rt == ~0ull ? 0ull : (t - t_drained_rt) / 10000ull;
        atomicAdd(P.debug + (after < 1ull ? 28 : after < 3ull ? 29 : after < 6ull ? 30 : 31), 1ull);
    }
#endif
    if (ring) {  // the wave's remaining partial sums (every lane of the wave is here)
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lane; i < P.ring_n; i += 64u) ring_flush(ring[i], P.accum);
    }
    // one segment-counter atomic per wave
    unsigned long long total = segs;  // widened before the wave sum
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
    if (lane == 0 && total) atomicAdd(P.segments, total);
    if (P.work_done) {  // the tallies' wave sums (64-bit: a wave's total may pass 2^32)
        unsigned long long wh = w_halves, wb = w_bounds;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            wh += __shfl_xor(wh, off);
            wb += __shfl_xor(wb, off);
        }
        if constexpr (kFlat) {  // and the flat scan's per-wave LDS tallies
            __builtin_amdgcn_wave_barrier();
            wh += ws->work[0];
            wb += ws->work[1];
        }
        if (lane == 0) {
            atomicAdd(P.work_done + 0, wh / 2u);
            atomicAdd(P.work_done + 1, wb);
        }
    }
    if constexpr (kStats) {
        // the wave's counts: every counter summed over the lanes (credit); every lane is here
        st_iters = wave_sum(st_iters);
        st_active = wave_sum(st_active);
        st_hitgroups = wave_sum(st_hitgroups);
        st_fetch = wave_sum(st_fetch);
        for (uint64_t PhaseTicks::*f :
             {&PhaseTicks::scan, &PhaseTicks::levels, &PhaseTicks::node, &PhaseTicks::group,
              &PhaseTicks::cand, &PhaseTicks::cand_passes, &PhaseTicks::big, &PhaseTicks::push,
              &PhaseTicks::shade, &PhaseTicks::fetch, &PhaseTicks::pass_entries,
              &PhaseTicks::pass_lanes, &PhaseTicks::partial_passes, &PhaseTicks::passes,
              &PhaseTicks::group_entries, &PhaseTicks::node_entries, &PhaseTicks::cam,
              &PhaseTicks::cam_entries, &PhaseTicks::cam_lanes, &PhaseTicks::cam_live,
              &PhaseTicks::list_trips, &PhaseTicks::list_sum, &PhaseTicks::root_trips,
              &PhaseTicks::root_sum, &PhaseTicks::shade_hits, &PhaseTicks::retire,
              &PhaseTicks::fetch_iters, &PhaseTicks::blk_fetches, &PhaseTicks::items_cur,
              &PhaseTicks::retire_iters, &PhaseTicks::quanta})
            pt.*f = wave_sum(pt.*f);
        if (lane == 0 && P.debug) {
            atomicAdd(P.debug + 0, (unsigned long long)st_iters);
            atomicAdd(P.debug + 1, (unsigned long long)st_active);
            atomicAdd(P.debug + 2, (unsigned long long)st_hitgroups);
            atomicAdd(P.debug + 3, (unsigned long long)st_fetch);
            const unsigned long long t = __builtin_amdgcn_s_memrealtime();
            atomicMax(P.debug + 4, t);
            atomicMin(P.debug + 5, t);
            atomicAdd(P.debug + 6, t >> 8);  // mean wave end time (in 256-tick units)
            atomicAdd(P.debug + 7, 1ull);
            atomicAdd(P.debug + 8, (unsigned long long)pt.scan);
            atomicAdd(P.debug + 9, (unsigned long long)pt.levels);
            atomicAdd(P.debug + 10, (unsigned long long)pt.node);
            atomicAdd(P.debug + 11, (unsigned long long)pt.group);
            atomicAdd(P.debug + 12, (unsigned long long)pt.cand);
            atomicAdd(P.debug + 13, (unsigned long long)pt.cand_passes);
            atomicAdd(P.debug + 14, (unsigned long long)(ticks() - t_begin));
            atomicAdd(P.debug + 15, (unsigned long long)pt.big);
            atomicAdd(P.debug + 16, (unsigned long long)pt.push);
            atomicAdd(P.debug + 17, (unsigned long long)pt.shade);
            atomicAdd(P.debug + 18, (unsigned long long)pt.fetch);
            atomicAdd(P.debug + 19, (unsigned long long)pt.pass_entries);
            atomicAdd(P.debug + 20, (unsigned long long)pt.pass_lanes);
            atomicAdd(P.debug + 21, (unsigned long long)pt.partial_passes);
            atomicAdd(P.debug + 22, (unsigned long long)pt.passes);
            atomicAdd(P.debug + 23, (unsigned long long)pt.cam);
            atomicAdd(P.debug + 24, (unsigned long long)pt.cam_entries);
            atomicAdd(P.debug + 25, (unsigned long long)pt.cam_lanes);
            atomicAdd(P.debug + 26, (unsigned long long)pt.cam_live);
            atomicAdd(P.debug + 27, (unsigned long long)pt.list_trips);
            atomicAdd(P.debug + 28, (unsigned long long)pt.list_sum);
            atomicAdd(P.debug + 29, (unsigned long long)pt.root_trips);
            atomicAdd(P.debug + 30, (unsigned long long)pt.root_sum);
            atomicAdd(P.debug + 31, (unsigned long long)pt.shade_hits);
            atomicAdd(P.debug + 32, (unsigned long long)pt.retire);
            atomicAdd(P.debug + 33, (unsigned long long)pt.fetch_iters);
            atomicAdd(P.debug + 34, (unsigned long long)pt.blk_fetches);
            atomicAdd(P.debug + 35, (unsigned long long)pt.items_cur);
            if constexpr (kCull == 4) {  // entries of the LDS-table kernel's group / node passes
                atomicAdd(P.debug + 36, (unsigned long long)pt.group_entries);
                atomicAdd(P.debug + 37, (unsigned long long)pt.node_entries);
            }
            atomicAdd(P.debug + 38, (unsigned long long)pt.retire_iters);
            atomicAdd(P.debug + 39, (unsigned long long)pt.quanta);
        }
    }
}
#undef P

}  // namespace

#ifndef VCRT_FLAT_BLOCK
#define VCRT_FLAT_BLOCK 256  // threads per workgroup the LDS flat scan is compiled for
#endif
#ifndef VCRT_FLAT_WAVES
#define VCRT_FLAT_WAVES 5  // waves per SIMD the flat scans are compiled for (LDS allows 5)
#endif

// VCRT_PART selects the kernels of one code-generation unit (Makefile: the global-table flat
// kernels are compiled apart, with the default scheduler settings); unset: every kernel.
#if !defined(VCRT_PART) || VCRT_PART == 1
extern "C" __global__ __launch_bounds__(256) void vcrt_trace_lds(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_geom[];
    trace_impl<true, false>(p, lds_geom);
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_smem(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_dyn[];
    trace_impl<false, false>(p, lds_dyn);
}

// Culled scan (exact; see scan_culled): spatially grouped sphere table + wave-level group tests.
extern "C" __global__ __launch_bounds__(256) void vcrt_trace_cull(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_dyn[];
    trace_impl<false, false, 1>(p, lds_dyn);
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_cull_stats(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_dyn[];
    trace_impl<false, true, 1>(p, lds_dyn);
}

// Per-lane culled scan (scan_culled_lane): tables in LDS (dynamic size = group-pair bounds +
// group records) or read from global memory.
extern "C" __global__ __launch_bounds__(256) void vcrt_trace_cull_lane_lds(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 2>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_cull_lane_lds_stats(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, true, 2>(p, lds_tab);
}

// Per-lane scan with the exact phase flattened over the wave (exact_flat): LDS tables plus
// 3.5 KB of scratch per wave.
extern "C" __global__ __launch_bounds__(VCRT_FLAT_BLOCK)
__attribute__((amdgpu_waves_per_eu(VCRT_FLAT_WAVES))) void vcrt_trace_cull_flat(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 4>(p, lds_tab);
}

// The flat scans' cost-order builds (vcrt_draw_next_frame "cost order"): the product kernel plus
// the per-pixel segment count of the measuring frame and the block order of later frames.
extern "C" __global__ __launch_bounds__(VCRT_FLAT_BLOCK)
__attribute__((amdgpu_waves_per_eu(VCRT_FLAT_WAVES))) void vcrt_trace_cull_flat_cost(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 4, true>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_cull_flat_stats(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, true, 4>(p, lds_tab);
}

#endif

#if !defined(VCRT_PART) || VCRT_PART == 2
// The flat scan for tables too large for LDS beside its stacks (the stress scene): tables in
// global memory (L2-resident), 32-bit stack entries (any group count), stacks alone in LDS.
extern "C" __global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(VCRT_FLAT_WAVES))) void vcrt_trace_cull_flat_global(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 5>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(VCRT_FLAT_WAVES))) void vcrt_trace_cull_flat_global_cost(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 5, true>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_cull_flat_global_stats(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, true, 5>(p, lds_tab);
}

// The flat scan for up to 1024 hierarchy groups whose records do not fit in LDS beside the
// stacks (the stress scene): the group and node boxes in LDS, one copy per CU for 16 waves
// (1024-thread workgroups), the group records in global memory, 16-bit stack entries.
extern "C" __global__ __launch_bounds__(1024) void vcrt_trace_cull_flat_boxes(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 6>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(1024) void vcrt_trace_cull_flat_boxes_cost(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 6, true>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(1024) void vcrt_trace_cull_flat_boxes_stats(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, true, 6>(p, lds_tab);
}

#endif

#if !defined(VCRT_PART) || VCRT_PART == 1
// The same with 1024-thread workgroups: one table copy serves 16 waves, so tables of up to
// 160 KB (the whole LDS of a CU; 4100 spheres take 108 KB) still live in LDS.
extern "C" __global__ __launch_bounds__(1024) void vcrt_trace_cull_lane_lds_wide(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 2>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(1024) void vcrt_trace_cull_lane_lds_wide_stats(
    TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, true, 2>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_cull_lane(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_dyn[];
    trace_impl<false, false, 3>(p, lds_dyn);
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_cull_lane_stats(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_dyn[];
    trace_impl<false, true, 3>(p, lds_dyn);
}

// Diagnostics builds (VCRT_DEBUG_STATS=1): same kernels plus lane-occupancy/tail counters.
extern "C" __global__ __launch_bounds__(256) void vcrt_trace_lds_stats(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_geom[];
    trace_impl<true, true>(p, lds_geom);
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_smem_stats(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_dyn[];
    trace_impl<false, true>(p, lds_dyn);
}

// Exact sample sums -> pixels (vcrt_math.h "Accumulation"; shader.comp:56 divides by SPP).
extern "C" __global__ __launch_bounds__(256) void vcrt_resolve(ResolveParams p) {
    if (p.counters != nullptr && blockIdx.x == 0u) {  // the tracer's counters: read, then zeroed
        unsigned long long v = 0ull;
        if (threadIdx.x < 4u) v = p.counters[threadIdx.x];
        __syncthreads();
        if (threadIdx.x < 4u) p.counters_out[threadIdx.x] = v;
        uint32_t* w = reinterpret_cast<uint32_t*>(p.counters);
        for (uint32_t i = threadIdx.x; i < p.counter_words; i += blockDim.x) w[i] = 0u;
        __threadfence_system();
    }
    const uint32_t elems = p.local_tiles * 64u;
    const double st = (double)p.spp_total, inv_all = p.inv_scale;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < elems;
         q += gridDim.x * blockDim.x) {
        const Pixel px = pixel_of(q, (uint32_t)p.width, (uint32_t)p.height, p.tiles_x,
                                  (uint32_t)p.world, (uint32_t)p.rank);
        if (!px.valid) continue;
        const double4 s = *reinterpret_cast<const double4*>(p.accum + 4u * q);
        const double inv = p.pixel_emax ? __builtin_ldexp(1.0, -pixel_scale_log2(p.pixel_emax[q]))
                                        : inv_all;
        if (p.zero_accum) *reinterpret_cast<double4*>(p.accum + 4u * q) = double4{0.0, 0.0, 0.0, 0.0};
        p.out[px.out_index] = make_float4(resolve_channel(s.x, inv, st),
                                          resolve_channel(s.y, inv, st),
                                          resolve_channel(s.z, inv, st),
#ifdef VCRT_COST_MAP  // diagnostics: alpha = the pixel's segments (tracer VCRT_COST_MAP)
                                          (float)s.w);
#else
                                          1.0f);
#endif
    }
}

// TraceParams.jitter (SetupJitterParams): the jitter term of every sample index.
extern "C" __global__ __launch_bounds__(256) void vcrt_setup_jitter(SetupJitterParams p) {
    const f3 p00 = mk(p.cam[0], p.cam[1], p.cam[2]);
    const f3 du = mk(p.cam[3], p.cam[4], p.cam[5]);
    const f3 dv = mk(p.cam[6], p.cam[7], p.cam[8]);
    const uint32_t total = p.nsamples + (p.corner ? p.slots : 0u);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gridDim.x * blockDim.x) {
        if (i < p.nsamples) {
            const f3 v = viewport_jitter(du, dv, p.jitter_in[i]);
            p.jitter[i] = make_float4(v.x, v.y, v.z, 0.0f);
        } else {  // the pixel corner of local slot q (edge-tile slots outside the frame too)
            const uint32_t q = i - p.nsamples, slot = q & 63u;
            uint32_t tx, ty;
            tile_of(q >> 6, p.rank, p.world, p.tiles_x, &tx, &ty);
            const f3 c = viewport_corner(p00, du, dv, 8u * tx + (slot & 7u), 8u * ty + (slot >> 3));
            p.corner[q] = make_float4(c.x, c.y, c.z, 0.0f);
        }
    }
}

// Re-interleave the packed tile framebuffers gathered from every rank into one frame.
extern "C" __global__ __launch_bounds__(256) void vcrt_assemble(AssembleParams p) {
    const uint32_t W = (uint32_t)p.width;
    const uint32_t total = W * (uint32_t)p.height;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gridDim.x * blockDim.x) {
        const uint32_t y = i / W, x = i - y * W;
        uint32_t r, lt;
        owner_of(x >> 3, y >> 3, (uint32_t)p.world, p.tiles_x, &r, &lt);
        const uint32_t slot = ((y & 7u) << 3) | (x & 7u);
        p.frame[i] = p.gathered[((size_t)r * p.tiles_per_rank + lt) * 64u + slot];
    }
}

// sRGB8 encode (present-time conversion of the B8G8R8A8_SRGB swapchain, Frontend.cpp:43):
// a channel's byte is the number of the 255 host-computed thresholds it reaches, i.e. the
// round-to-nearest of the exact sRGB encode of the clamped value; alpha is stored linearly.
extern "C" __global__ __launch_bounds__(256) void vcrt_encode_srgb8(EncodeParams p) {
    __shared__ float th[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) th[i] = i < 255 ? p.thresholds[i] : 3e38f;
    __syncthreads();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.count;
         i += gridDim.x * blockDim.x) {
        const float4 v = p.in[i];
        const float c[3] = {v.x, v.y, v.z};
        unsigned char b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int lo = 0;  // count of thresholds <= c[k] (NaN reaches none: 0)
#pragma unroll
            for (int step = 128; step > 0; step >>= 1)
                if (c[k] >= th[lo + step - 1]) lo += step;
            b[k] = (unsigned char)lo;
        }
        const float a = v.w != v.w ? 0.0f : fminf(fmaxf(v.w, 0.0f), 1.0f);
        p.out[i] = make_uchar4(b[0], b[1], b[2], (unsigned char)(a * 255.0f + 0.5f));
    }
}

// Self-test of sin_fast (vcrt_math.h) against sin_canonical on the fp32 inputs with bit
// patterns first .. first + count - 1 (wrapping): counts the inputs where they differ and where
// the fast value was not accepted (the fallback ran), and keeps the smallest differing pattern.
extern "C" __global__ __launch_bounds__(256) void vcrt_check_sin(SinCheckParams p) {
    uint64_t bad = 0, fallback = 0;
    uint32_t first_bad = 0xFFFFFFFFu;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.count; i += stride) {
        const uint32_t bits = p.first + i;
        const float x = __uint_as_float(bits);
        float f;
        const bool ok = sin_fast_try(x, f);
        if (!ok) f = sin_canonical(x);
        fallback += ok ? 0u : 1u;
        const float want = sin_canonical(x);
        // and the two-argument form the scatter uses (sin3: sin_fast_try_n<2>), on the input and
        // its negation: every accepted value must be the canonical one
        const float xs[2] = {x, -x};
        float fs[2], ft[2], fu[1];
        const bool ok2 = sin_fast_try_n<2>(xs, fs);
        // and the table form (constants from the kernel arguments, as the tracer reads them)
        const bool okt = sin_fast_try_n<2, true>(xs, ft, (cdouble*)&p.sin_c[0]);
        const bool oku = sin_fast_try_n<1, true>(xs, fu, (cdouble*)&p.sin_c[0]);
        const float wneg = sin_canonical(-x);
        const bool bad2 = (ok2 && (__float_as_uint(fs[0]) != __float_as_uint(want) ||
                                   __float_as_uint(fs[1]) != __float_as_uint(wneg))) ||
                          (okt && (__float_as_uint(ft[0]) != __float_as_uint(want) ||
                                   __float_as_uint(ft[1]) != __float_as_uint(wneg))) ||
                          (oku && __float_as_uint(fu[0]) != __float_as_uint(want));
        if (__float_as_uint(f) != __float_as_uint(want) || bad2) {
            ++bad;
            first_bad = min(first_bad, bits);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        bad += __shfl_xor(bad, off);
        fallback += __shfl_xor(fallback, off);
        first_bad = min(first_bad, (uint32_t)__shfl_xor((int)first_bad, off));
    }
    if ((threadIdx.x & 63u) == 0) {
        if (bad) atomicAdd(p.result + 0, (unsigned long long)bad);
        if (fallback) atomicAdd(p.result + 1, (unsigned long long)fallback);
        if (first_bad != 0xFFFFFFFFu) atomicMin(p.first_bad, first_bad);
    }
}

extern "C" __global__ __launch_bounds__(256) void vcrt_fill(FillParams p) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.count;
         i += gridDim.x * blockDim.x)
        p.out[i] = p.value;
}
#endif

// ---------------------------------------------------------------------------------------------
// Ray queries: ray_color (functions.glsl:65-92) and the first hit_sphere scan of caller-supplied
// rays, a code-generation unit of its own (Makefile, part 3); shade_segment serves the adaptive
// sampling kernel too (part 15).
#if !defined(VCRT_PART) || VCRT_PART == 3 || VCRT_PART == 15
namespace {

// One traced segment shaded: the arithmetic of trace_impl's shade_and_advance, hit and sky
// branches, on a ray that belongs to no pixel. A hit scatters the ray (o, d, atten), returns its
// normal (functions.glsl:33-35: (point - centre) / radius, not flipped) and false; the sky
// returns true with the path's radiance atten * sky in contrib.
__device__ __forceinline__ bool shade_segment(const TraceParams& S, float max_t, int best, f3& o,
                                              f3& d, f3& atten, f3& normal, f3& contrib) {
    if (best < 0) {
        const float len = sqrt_fast(dot(d, d));  // length(d)
        contrib = mul(atten, sky_factor(d.y / len));
        return true;
    }
    const float4 cr = S.center_radius[best], sh = S.shade[best], mat = S.material[best];
    const f3 point = add(scale(max_t, d), o);
    // the unscaled division with one reciprocal for numerators and radius in [2^-40, 2^30] (the
    // radius by a host flag), else hipcc's full division in a real branch: the same bits
    const f3 pcv = sub(point, mk(cr.x, cr.y, cr.z));
    const float yr = recip_a(cr.w);
    normal = mk(div_a(pcv.x, cr.w, yr), div_a(pcv.y, cr.w, yr), div_a(pcv.z, cr.w, yr));
    const float nmin = fminf(fminf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
    const float nmax = fmaxf(fmaxf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
    if (!((S.flags & kFlagRadiiSafe) != 0u && nmin >= 0x1p-40f && nmax <= 0x1p30f)) {
        asm volatile("");
        normal = divs(pcv, cr.w);
    }
    const int type = (int)mat.x;
    const f3 albedo = mk(sh.x, sh.y, sh.z);
    const float param = sh.w;
    // rand(dir.xy), rand(dir.xz), rand(dir.yz) for lambertian/metal (functions.glsl:43),
    // rand(point.xy) for glass (textures.glsl:51)
    float s1, s2, s3;
    sin3<true>(rand_arg_first(type == 3, point, d), rand_arg(d.x, d.z), rand_arg(d.y, d.z), s1,
               s2, s3, (cdouble*)&S.sin_c[0], nullptr);
    const float r1 = rand_of_sin(s1);
    if (type == 1 || type == 2) {
        const float r2 = rand_of_sin(s2);
        const float r3 = rand_of_sin(s3);
        const f3 ru = mk(r1, r2, r3);  // random_in_unit_sphere(dir): normalize
        const f3 u = unit_of(ru);
        if (type == 1) {
            d = add(normal, u);
            atten = scale(param, mul(atten, albedo));
        } else {
            d = add(reflect(d, normal), scale(param, u));
            atten = mul(atten, albedo);
        }
        o = point;
    } else if (type == 3) {
        const f3 reflected = reflect(d, normal);
        f3 outward;
        float ni, cosine;
        const float dn = dot(d, normal);
        if (dn > 0.0f) {
            outward = neg(normal);
            ni = param;
            cosine = sqrt_fast(1.0f - param * param * (1.0f - dn * dn));
        } else {
            outward = normal;
            ni = mat.y;  // 1.0f / param
            cosine = -dn;
        }
        f3 refracted = mk(0.f, 0.f, 0.f);
        float reflect_prob = 1.0f;
        const float dt = dot(d, outward);
        const float disc = 1.0f - ni * ni * (1.0f - dt * dt);
        if (disc > 0.0f) {
            const float sd = sqrt_fast(disc);
            refracted = sub(scale(ni, sub(d, scale(dt, outward))), scale(sd, outward));
            reflect_prob = schlick_r0(cosine, mat.z);  // schlick(cosine, param)
        }
        o = point;
        d = (r1 < reflect_prob) ? reflected : refracted;
    }
    return false;
}

}  // namespace
#endif

#if !defined(VCRT_PART) || VCRT_PART == 3
// A persistent grid of lanes, one ray per lane: a lane whose path has ended takes the next ray
// index, and a wave claims the indices of all its needing lanes with one atomic (adjacent lanes
// of a claim get adjacent rays). Every segment runs the per-lane culled scan on the global tables
// when the scene has them and every ray the wave holds is in the guarded range, else the linear
// scan: the same sphere and t either way (facts (1)-(4) above), so a ray's result does not
// depend on the rays it shares a wave with. Lanes with no ray left sit out (as trace_impl's done
// lanes do: the scans' ballots see the active lanes only) and hold a guarded ray.
extern "C" __global__ __launch_bounds__(256) void vcrt_trace_rays(RayQueryParams p_arg) {
    // the arguments through a pointer to the kernarg segment, as trace_impl reads them (scalar
    // loads from the constant cache; the sine's constant table is addressed there)
    (void)p_arg;
    const RayQueryParams& p = *reinterpret_cast<const RayQueryParams*>(
        (__attribute__((address_space(4))) const RayQueryParams*)
            __builtin_amdgcn_kernarg_segment_ptr());
    const TraceParams& S = p.scene;
    const uint32_t lane = threadIdx.x & 63u;
    if (S.max_depth <= 0) {  // ray_color's undefined return (canonical 0) without a scan
        const uint4 h0 = make_uint4(__float_as_uint(kInfinity), 0xffffffffu, 0u, 0u);
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.count;
             i += gridDim.x * blockDim.x) {
            if (p.radiance) p.radiance[i] = make_float4(0.f, 0.f, 0.f, 1.f);
            if (p.hits) {
                p.hits[2u * (size_t)i] = h0;
                p.hits[2u * (size_t)i + 1u] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        return;
    }
    const int n = S.nspheres;
    const float4* tgroup = S.cgroup + 5 * S.nbig;  // the hierarchy's group records
    bool need = true, done = false;
    uint32_t idx = 0u;
    f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 1.f, 0.f), atten = mk(1.f, 1.f, 1.f);
    int pass = 0;
    // the first segment's record (vcrt_ray_hit)
    float hit_t = kInfinity;
    int hit_sphere = -1;
    f3 hit_normal = mk(0.f, 0.f, 0.f);
    uint32_t segs = 0u;  // this lane's segments, all its rays
    uint32_t w_halves = 0u, w_bounds = 0u;
    for (;;) {
        // ---- lanes whose path has ended take the next rays: one atomic per wave ----
        const uint64_t need_mask = __ballot(need && !done);
        if (need_mask != 0u) {
            const int leader = __builtin_ctzll(need_mask);
            uint32_t base = 0u;
            if ((int)lane == leader) base = atomicAdd(p.work, (uint32_t)__popcll(need_mask));
            base = __builtin_amdgcn_readfirstlane(__shfl(base, leader));
            if (need && !done) {
                idx = base + lanes_below(need_mask);
                if (idx < p.count) {
                    const float* po = p.origins + 3u * (size_t)idx;
                    const float* pd = p.dirs + 3u * (size_t)idx;
                    o = mk(po[0], po[1], po[2]);
                    d = mk(pd[0], pd[1], pd[2]);
                    atten = mk(1.f, 1.f, 1.f);
                    pass = 0;
                    need = false;
                } else {  // no ray left: nothing more is stored, and the ray held is guarded
                    done = true;
                    o = mk(0.f, 0.f, 0.f);
                    d = mk(0.f, 1.f, 0.f);
                }
            }
        }
        if (__ballot(!done) == 0u) break;
        if (done) continue;

        // ---- one segment: scan the whole sphere list (functions.glsl:73-81) ----
        ++segs;
        float max_t = kInfinity;
        int best = -1;
        uint32_t hit_groups = 0u, lane_cnt = 0u;
        const float aa = dot(d, d);
        const bool guarded = (S.flags & kFlagSceneBounded) != 0 && aa >= 0x1p-20f &&
                             aa <= 0x1p60f && fabsf(o.x) <= 0x1p30f && fabsf(o.y) <= 0x1p30f &&
                             fabsf(o.z) <= 0x1p30f;
        if (S.ncgroups > 0 && __ballot(!guarded) == 0u) {
            scan_culled_lane<false>(S, S.cbound, tgroup, o, d, max_t, best, w_halves, w_bounds,
                                    lane_cnt, hit_groups);
        } else {
            scan_spheres<false>(S, nullptr, n, o, d, max_t, best, hit_groups);
            tally(w_halves, 2u * (uint32_t)((n + 3) >> 2));
        }

        // ---- shade (textures.glsl) or sky (functions.glsl:85-89) ----
        f3 normal = mk(0.f, 0.f, 0.f), contrib = mk(0.f, 0.f, 0.f);
        const bool first = pass == 0;
        bool ended = shade_segment(S, max_t, best, o, d, atten, normal, contrib);
        if (first) {
            hit_t = best >= 0 ? max_t : kInfinity;
            hit_sphere = best;
            hit_normal = normal;
        }
        if (!ended) {
            ++pass;
            ended = pass >= S.max_depth;  // undefined GLSL return -> vec3(0)
        }
        if (ended) {
            if (p.radiance) p.radiance[idx] = make_float4(contrib.x, contrib.y, contrib.z, 1.0f);
            if (p.hits) {
                // the path's scans: one per hit, and the sky's
                const uint32_t nseg = (uint32_t)pass + (best < 0 ? 1u : 0u);
                p.hits[2u * (size_t)idx] = make_uint4(__float_as_uint(hit_t), (uint32_t)hit_sphere,
                                                      nseg, 0u);
                p.hits[2u * (size_t)idx + 1u] =
                    make_uint4(__float_as_uint(hit_normal.x), __float_as_uint(hit_normal.y),
                               __float_as_uint(hit_normal.z), 0u);
            }
            need = true;
        }
    }
    // one atomic per wave and tally
    unsigned long long total = segs, wh = w_halves, wb = w_bounds;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        total += __shfl_xor(total, off);
        wh += __shfl_xor(wh, off);
        wb += __shfl_xor(wb, off);
    }
    if (lane == 0) {
        if (total) atomicAdd(p.tallies + 0, total);
        atomicAdd(p.tallies + 1, wh / 2u);
        atomicAdd(p.tallies + 2, wb);
    }
}
#endif

// ---------------------------------------------------------------------------------------------
// Occlusion queries: is any sphere accepted by hit_sphere between min_t and the ray's own reach
// (fact (6))? A code-generation unit of its own (Makefile, part 4); the scans serve the ambient
// visibility buffer's secondary rays too (part 10).
#if !defined(VCRT_PART) || VCRT_PART == 4 || VCRT_PART == 10
namespace {

// min_t < t < T: hit_sphere's strict comparisons on the candidate's t (fact (6))
__device__ __forceinline__ bool reaches(float t, float T) { return (t > kMinT) & (t < T); }

// exact_group_uniform for an any-hit query: true when the lane's ray accepts a member of the
// group (the big-sphere list; candidate_t_fast returns candidate_t's t wherever that t is above
// min_t, whatever the far limit).
__device__ __forceinline__ bool occlude_group_uniform(cfloat4* rec, const CullRay& r, v2f dx,
                                                      v2f dy, v2f dz, v2f a2, float a, float ya,
                                                      float T) {
    const float4 q0 = rec[0], q1 = rec[1], idf = rec[4];
    v2f hb01, cc01, d01, hb23 = {0.f, 0.f}, cc23 = {0.f, 0.f}, d23 = {-1.f, -1.f};
    pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, q0, q1, hb01, cc01, d01);
    // members 2 and 3 only when the group has them (wave-uniform)
    if (__float_as_int(idf.z) >= 0 || __float_as_int(idf.w) >= 0)
        pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, rec[2], rec[3], hb23, cc23, d23);
    const float m4 = fmaxf(fmaxf(d01.x, d01.y), fmaxf(d23.x, d23.y));
    bool occ = false;
    if (__ballot(!(m4 < 0.0f))) {
        if (may_hit(hb01.x, cc01.x, d01.x))
            occ |= reaches(candidate_t_fast(hb01.x, d01.x, a, ya), T);
        if (may_hit(hb01.y, cc01.y, d01.y))
            occ |= reaches(candidate_t_fast(hb01.y, d01.y, a, ya), T);
        if (may_hit(hb23.x, cc23.x, d23.x))
            occ |= reaches(candidate_t_fast(hb23.x, d23.x, a, ya), T);
        if (may_hit(hb23.y, cc23.y, d23.y))
            occ |= reaches(candidate_t_fast(hb23.y, d23.y, a, ya), T);
    }
    return occ;
}

// scan_culled_lane for an any-hit query with the far limit T (fact (6)): the same big-group
// list and the same chunk, node and group box tests on the global tables, but a lane that has
// found an accepted member (occ) asks for nothing more -- it drops out of the chunk, node and
// group ballots -- and the wave leaves the chunk loop once every lane is occluded. Lanes that
// enter occluded (the lanes past the batch's end) never ask for anything.
__device__ __forceinline__ bool occlude_culled_lane(const TraceParams& p, const float4* tbound,
                                                    const float4* tgroup, const f3 o, const f3 d,
                                                    const float T, bool occ,
                                                    uint32_t& groups_tested,
                                                    uint32_t& bounds_tested) {
    const float a = dot(d, d);
    const float ya = recip_a(a);
    CullRay r;
    r.ox = (v2f){o.x, o.x};
    r.oy = (v2f){o.y, o.y};
    r.oz = (v2f){o.z, o.z};
    const BoxRay br = box_ray(p, o, d, ya);
    const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {a, a};
    cfloat4* node = (cfloat4*)p.cnode;
    cfloat4* top = (cfloat4*)p.ctop;
    const int ncg = p.ncgroups;
    // per-query pass counters, wave-uniform
    uint32_t n_bounds = 0, n_groups = 0;
    for (int gb = 0; gb < p.nbig; ++gb) {  // the big spheres (scalar loads)
        if (__ballot(!occ) == 0) break;
        ++n_groups;
        occ |= occlude_group_uniform((cfloat4*)p.cgroup + 5 * gb, r, dx, dy, dz, a2, a, ya, T);
    }
    uint32_t tops = 0;
    for (int base = 0; base < ncg; base += 64) {
        if (__ballot(!occ) == 0) break;
        // level 0, wave-uniform: the chunk's own bound (two chunks per test), per-lane bits
        if ((base & 127) == 0) {
            const BoundPair tp = load_bound_pair(top + 4 * (base >> 7));
            tops = ~push_bound_pair(0u, br, tp.b0, tp.b1, tp.b2, tp.b3) & 3u;
            n_bounds += 2;
        }
        const bool in_chunk = !occ && ((tops >> ((base >> 6) & 1)) & 1u) != 0;
        if (__ballot(in_chunk) == 0) continue;
        // level 1, wave-uniform: nodes of this chunk, per-lane bits
        const int nn = min(8, (ncg - base) >> 3);
        cfloat4* nb = node + 4 * (base >> 4);
        // sign bits pushed from the last node down, so bit j ends up = node j ruled out
        uint32_t out = 0;
        BoundPair cur = load_bound_pair(nb + 4 * ((nn - 2) >> 1));
        for (int j = nn - 2; j >= 0; j -= 2) {
            const BoundPair nxt = load_bound_pair(nb + 4 * ((j >= 2 ? j - 2 : j) >> 1));
            out = push_bound_pair(out, br, cur.b0, cur.b1, cur.b2, cur.b3);
            cur = nxt;
        }
        uint32_t nodes = in_chunk ? ~out & ((1u << nn) - 1u) : 0u;
        n_bounds += (uint32_t)nn;
        // level 2, per lane: the groups of this lane's nodes
        uint64_t need = 0;
        while (__ballot(nodes != 0)) {
            n_bounds += 8;  // one wave pass = 8 bound tests
            if (nodes) {
                const int j = __builtin_ctz(nodes);
                nodes &= nodes - 1;
                const float4* gb = tbound + 4 * (base >> 1) + __umul24((uint32_t)j, 16u);
                uint32_t gout = 0;
#pragma unroll
                for (int k = 3; k >= 0; k--) {
                    gout = push_bound_pair(gout, br, gb[4 * k], gb[4 * k + 1], gb[4 * k + 2],
                                           gb[4 * k + 3]);
                }
                need |= (uint64_t)(~gout & 0xffu) << (8 * j);
            }
        }
        // the exact test, per lane on its own groups, until the lane is occluded
        while (__ballot(need != 0)) {
            ++n_groups;
            if (need) {
                const int k = __builtin_ctzll(need);
                need &= need - 1;
                const float4* g = tgroup + 5 * base + __umul24((uint32_t)k, 5u);
                const float4 q0 = g[0], q1 = g[1], q2 = g[2], q3 = g[3];
                v2f hb01, cc01, d01, hb23, cc23, d23;
                pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, q0, q1, hb01, cc01, d01);
                pair_disc_cc(r.ox, r.oy, r.oz, dx, dy, dz, a2, q2, q3, hb23, cc23, d23);
                // bit s = member s may be accepted (sign bits, pushed from member 3 down)
                uint32_t hits = push_sign(0u, hit_sign(hb23.y, cc23.y, d23.y));
                hits = push_sign(hits, hit_sign(hb23.x, cc23.x, d23.x));
                hits = push_sign(hits, hit_sign(hb01.y, cc01.y, d01.y));
                hits = push_sign(hits, hit_sign(hb01.x, cc01.x, d01.x));
                while (hits) {
                    const int s = __builtin_ctz(hits);
                    hits &= hits - 1;
                    const float hb = s == 0 ? hb01.x : s == 1 ? hb01.y : s == 2 ? hb23.x : hb23.y;
                    const float ds = s == 0 ? d01.x : s == 1 ? d01.y : s == 2 ? d23.x : d23.y;
                    if (reaches(candidate_t(hb, ds, a), T)) {
                        occ = true;
                        hits = 0u;
                        need = 0u;
                    }
                }
            }
        }
    }
    tally(bounds_tested, __builtin_amdgcn_readfirstlane(n_bounds));
    tally(groups_tested, 2u * __builtin_amdgcn_readfirstlane(n_groups));  // half-groups
    return occ;
}

// hit_sphere's acceptance (functions.glsl:14-40) after the discriminant test passed, against a
// far limit that does not shrink: accept_root's logic, literally.
__device__ __forceinline__ bool accepts_root(float hb, float disc, float a, float T) {
    const float min_t = kMinT;
    const float sq = __builtin_sqrtf(disc);
    float root = (-hb - sq) / a;
    bool ok = true;
    if (root <= min_t || T <= root) {
        root = (-hb + sq) / a;
        ok = !(root <= min_t || T <= root);
    }
    return ok;
}

// The linear scan for an any-hit query, any ray: four spheres per step from the original table
// (scalar loads, the next group prefetched), every sphere whose discriminant is not negative put
// through accepts_root, until the whole wave is occluded. Padding spheres (index >= n) never
// accept.
__device__ __forceinline__ bool occlude_linear(const TraceParams& p, int n, const f3 o,
                                               const f3 d, const float T, bool occ,
                                               uint32_t& groups_tested) {
    const float a = dot(d, d);
    const v2f ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
    const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {a, a};
    const int ngroups = (n + 3) >> 2;
    uint32_t n_groups = 0;
    Group g = load_group<false>(nullptr, p, 0);
    for (int gi = 0; gi < ngroups; ++gi) {
        if (__ballot(!occ) == 0) break;
        ++n_groups;
        const Group nx = load_group<false>(nullptr, p, gi + 1);  // table padded by one group
        v2f hb01, d01, hb23, d23;
        pair_disc(ox, oy, oz, dx, dy, dz, a2, g.q[0], g.q[1], hb01, d01);
        pair_disc(ox, oy, oz, dx, dy, dz, a2, g.q[2], g.q[3], hb23, d23);
        const int j = 4 * gi;
        const bool e0 = !occ && !(d01.x < 0.0f), e1 = !occ && !(d01.y < 0.0f) && j + 1 < n,
                   e2 = !occ && !(d23.x < 0.0f) && j + 2 < n,
                   e3 = !occ && !(d23.y < 0.0f) && j + 3 < n;
        if (__ballot(e0 || e1 || e2 || e3)) {
            if (e0) occ |= accepts_root(hb01.x, d01.x, a, T);
            if (e1) occ |= accepts_root(hb01.y, d01.y, a, T);
            if (e2) occ |= accepts_root(hb23.x, d23.x, a, T);
            if (e3) occ |= accepts_root(hb23.y, d23.y, a, T);
        }
        g = nx;
    }
    tally(groups_tested, 2u * __builtin_amdgcn_readfirstlane(n_groups));  // half-groups
    return occ;
}

}  // namespace
#endif

#if !defined(VCRT_PART) || VCRT_PART == 4
// One scan per ray and no work counter: wave w of the grid takes rays 64 w + lane, then strides
// by the grid's waves (coalesced loads of 3 + 3 + 1 dwords per ray, one byte stored per lane).
// A wave takes the culled scan when the scene has tables and all its rays are in the guarded
// range, else the linear scan: the same answer either way (fact (6)), so a ray's result does not
// depend on the rays it shares a wave with. Lanes past the end of the batch hold a guarded ray,
// start as occluded -- they never keep the wave in a loop -- and store nothing. No LDS.
extern "C" __global__ __launch_bounds__(256) void vcrt_occlude_rays(OcclusionParams p_arg) {
    // the arguments through a pointer to the kernarg segment, as trace_impl reads them
    (void)p_arg;
    const OcclusionParams& p = *reinterpret_cast<const OcclusionParams*>(
        (__attribute__((address_space(4))) const OcclusionParams*)
            __builtin_amdgcn_kernarg_segment_ptr());
    const TraceParams& S = p.scene;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = p.count;
    const uint32_t stride = gridDim.x * blockDim.x;  // a multiple of 64
    const float4* tgroup = S.cgroup + 5 * S.nbig;    // the hierarchy's group records
    uint32_t w_halves = 0u, w_bounds = 0u;
    // count <= 2^30 and the stride is far below 2^30: the index does not wrap
    for (uint32_t base = __builtin_amdgcn_readfirstlane(
             (blockIdx.x * blockDim.x + threadIdx.x) & ~63u);
         base < count; base += stride) {
        const uint32_t idx = base + lane;
        const bool live = idx < count;
        f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 1.f, 0.f);
        float T = kInfinity;
        if (live) {
            const float* po = p.origins + 3u * (size_t)idx;
            const float* pd = p.dirs + 3u * (size_t)idx;
            o = mk(po[0], po[1], po[2]);
            d = mk(pd[0], pd[1], pd[2]);
            if (p.tmax) T = p.tmax[idx];
        }
        const float aa = dot(d, d);
        const bool guarded = (S.flags & kFlagSceneBounded) != 0 && aa >= 0x1p-20f &&
                             aa <= 0x1p60f && fabsf(o.x) <= 0x1p30f && fabsf(o.y) <= 0x1p30f &&
                             fabsf(o.z) <= 0x1p30f;
        bool occ = !live;
        if (S.ncgroups > 0 && __ballot(!guarded) == 0u)
            occ = occlude_culled_lane(S, S.cbound, tgroup, o, d, T, occ, w_halves, w_bounds);
        else
            occ = occlude_linear(S, S.nspheres, o, d, T, occ, w_halves);
        if (live) p.occluded[idx] = occ ? (uint8_t)1 : (uint8_t)0;
    }
    // one atomic per wave and tally
    unsigned long long wh = w_halves, wb = w_bounds;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        wh += __shfl_xor(wh, off);
        wb += __shfl_xor(wb, off);
    }
    if (lane == 0) {
        atomicAdd(p.tallies + 0, wh / 2u);
        atomicAdd(p.tallies + 1, wb);
    }
}
#endif

// ---- thin-lens frames (vcrt.h lens_radius > 0) ----------------------------------------------
// Part 5, a unit of its own with the default scheduler: the frame kernels a lens renderer
// launches, trace_impl with kLens. The linear SMEM scan has its cost-order hooks built in; the
// flat scans come as the product build and the cost-order build, with the launch bounds and
// wave targets of their pinhole kernels. There are no lens stats builds.
#if !defined(VCRT_PART) || VCRT_PART == 5
extern "C" __global__ __launch_bounds__(256) void vcrt_trace_smem_lens(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_dyn[];
    trace_impl<false, false, 0, false, true>(p, lds_dyn);
}

extern "C" __global__ __launch_bounds__(VCRT_FLAT_BLOCK)
__attribute__((amdgpu_waves_per_eu(VCRT_FLAT_WAVES))) void vcrt_trace_cull_flat_lens(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 4, false, true>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(VCRT_FLAT_BLOCK)
__attribute__((amdgpu_waves_per_eu(VCRT_FLAT_WAVES))) void vcrt_trace_cull_flat_lens_cost(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 4, true, true>(p, lds_tab);
}

// The global-table scan at five waves per SIMD spills two VGPRs to scratch (as its pinhole build
// does); the lens builds are compiled for four and keep everything in registers.
extern "C" __global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(VCRT_FLAT_WAVES - 1))) void vcrt_trace_cull_flat_global_lens(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 5, false, true>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(VCRT_FLAT_WAVES - 1))) void vcrt_trace_cull_flat_global_lens_cost(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 5, true, true>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(1024) void vcrt_trace_cull_flat_boxes_lens(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 6, false, true>(p, lds_tab);
}

extern "C" __global__ __launch_bounds__(1024) void vcrt_trace_cull_flat_boxes_lens_cost(TraceParams p) {
    extern __shared__ __attribute__((aligned(16))) float4 lds_tab[];
    trace_impl<false, false, 6, true, true>(p, lds_tab);
}
#endif

// ---------------------------------------------------------------------------------------------
// Feature buffers (vcrt_draw_features): first-hit albedo, normal, depth, coverage and sphere id
// of the frame's own camera rays, a code-generation unit of its own (Makefile, part 8).
// One wave per local 8x8 tile, one lane per slot; a lane runs its pixel's n samples in index
// order and keeps the eight sums in registers, so the bits depend on the sample order alone.
// Lanes of slots outside the frame sit out (the scans' ballots see the active lanes only).
// A sample's ray is trace_impl's camera ray: (corner + jitter_i) - origin, the origin the camera
// centre or, with a lens, the table's centre + offset_i. Its first hit comes from one of three
// routes, which give the same sphere and t (facts (1)-(4) above):
//  * the camera-ray lists (a pinhole frame that has them, the lane's quarter listed, guard_a):
//    the big groups' camera-relative records, then the quarter's listed pairs -- the helper
//    calls of trace_impl's camera fast trace;
//  * else what vcrt_trace_rays runs: the per-lane culled scan on the global tables when the
//    scene has them and every ray the wave's remaining lanes hold is in the guarded range,
//  * else the linear scan.
#if !defined(VCRT_PART) || VCRT_PART == 10 || VCRT_PART == 12 || VCRT_PART == 15
namespace {

// The first hit of one sample's camera ray (o, d), aa = dot(d, d), by the three routes above, as
// a function for the ambient visibility kernel (part 10): inf is the list word of the lane's
// quarter (15 in its low bits: no list), max_t and best enter as (kInfinity, -1). The statements
// are vcrt_frame_features' own, which keeps its copy: called from there the function moves that
// kernel's register allocation, and part 8's object file is to stay what it was.
__device__ __forceinline__ void frame_first_hit(const TraceParams& S, const uint32_t inf,
                                                const float4* tgroup, const int n, const f3 o,
                                                const f3 d, const float aa, float& max_t,
                                                int& best, uint32_t& listed, uint32_t& w_halves,
                                                uint32_t& w_bounds) {
    // (a pinhole ray starts at the camera centre: the host hands out prim_info only to
    // a bounded scene and a centre within 2^30, the other half of the range guard)
    const bool cam_now = (inf & 15u) != 15u && guard_a(aa);
    if (cam_now) {
        ++listed;
        cfloat4* crec = (cfloat4*)S.cam_rec;
        const float ya = recip_a(aa);
        const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {aa, aa};
        for (int gb = 0; gb < S.nbig; ++gb)  // the big spheres (scalar loads)
            exact_group_uniform_cam(crec + 4 * gb, (cfloat4*)S.cgroup + 5 * gb, dx, dy,
                                    dz, a2, aa, ya, max_t, best);
        // the quarter's listed spheres, two per record (primary.cpp)
        const uint32_t cnt = inf & 15u;
        const float4* lr = S.cam_rec + 4u * (uint32_t)S.nbig + 3u * (inf >> 4);
        uint32_t iters = 0u;
        for (uint32_t m = 0; 2u * m < cnt; ++m) {
            ++iters;
            const float4 q0 = lr[3u * m], q1 = lr[3u * m + 1u], id = lr[3u * m + 2u];
            v2f hb, cc, dc;
            pair_disc_cam(dx, dy, dz, a2, q0, q1, hb, cc, dc);
            if (__float_as_int(hit_sign(hb.x, cc.x, dc.x)) < 0)
                consider(candidate_t_fast(hb.x, dc.x, aa, ya), __float_as_int(id.x),
                         max_t, best);
            if (__float_as_int(hit_sign(hb.y, cc.y, dc.y)) < 0)
                consider(candidate_t_fast(hb.y, dc.y, aa, ya), __float_as_int(id.y),
                         max_t, best);
        }
        // issued work as the frame counts it: a pair test is half a group test
        tally(w_halves, 2u * (uint32_t)S.nbig + wave_max_small<3>(iters));
    } else {
        uint32_t hit_groups = 0u, lane_cnt = 0u;
        const bool guarded = (S.flags & kFlagSceneBounded) != 0 && aa >= 0x1p-20f &&
                             aa <= 0x1p60f && fabsf(o.x) <= 0x1p30f &&
                             fabsf(o.y) <= 0x1p30f && fabsf(o.z) <= 0x1p30f;
        if (S.ncgroups > 0 && __ballot(!guarded) == 0u) {
            scan_culled_lane<false>(S, S.cbound, tgroup, o, d, max_t, best, w_halves,
                                    w_bounds, lane_cnt, hit_groups);
        } else {
            scan_spheres<false>(S, nullptr, n, o, d, max_t, best, hit_groups);
            tally(w_halves, 2u * (uint32_t)((n + 3) >> 2));
        }
    }
}

}  // namespace
#endif

#if !defined(VCRT_PART) || VCRT_PART == 8
extern "C" __global__ __launch_bounds__(256) void vcrt_frame_features(FeatureParams p_arg) {
    // the arguments through a pointer to the kernarg segment, as trace_impl reads them
    (void)p_arg;
    const FeatureParams& p = *reinterpret_cast<const FeatureParams*>(
        (__attribute__((address_space(4))) const FeatureParams*)
            __builtin_amdgcn_kernarg_segment_ptr());
    const TraceParams& S = p.scene;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (lt >= S.local_tiles) return;  // (the whole wave)
    const uint32_t q = lt * 64u + lane;
    const Pixel px = pixel_of(q, (uint32_t)S.width, (uint32_t)S.height, S.tiles_x,
                              (uint32_t)S.world, (uint32_t)S.rank);
    const uint32_t nsamples = p.n;
    const bool lens = S.lens != nullptr;
    uint32_t w_halves = 0u, w_bounds = 0u, listed = 0u;
    if (px.valid) {
        const f3 p00 = mk(S.cam[0], S.cam[1], S.cam[2]);
        const f3 du = mk(S.cam[3], S.cam[4], S.cam[5]);
        const f3 dv = mk(S.cam[6], S.cam[7], S.cam[8]);
        const f3 cam = mk(S.cam[9], S.cam[10], S.cam[11]);
        // shader.comp:43's pixel corner, vcrt_setup_jitter's operations (TraceParams.corner)
        const f3 corner = viewport_corner(p00, du, dv, px.x, px.y);
        // the sphere list of the lane's 4x4 quarter (slot 8 y + x), as trace_impl reads it
        uint32_t inf = 15u;
        if (p.use_lists != 0u && !lens && S.prim_info != nullptr)
            inf = S.prim_info[2u * (lt * 4u + (((lane >> 5) & 1u) << 1) + ((lane >> 2) & 1u)) + 1u];
        const int n = S.nspheres;
        const float4* tgroup = S.cgroup + 5 * S.nbig;  // the hierarchy's group records
        cfloat4* jitter = (cfloat4*)S.jitter;           // wave-uniform indices: scalar loads
        cfloat4* lens_tab = (cfloat4*)S.lens;
        f3 sum_a = mk(0.f, 0.f, 0.f), sum_n = mk(0.f, 0.f, 0.f);
        float sum_c = 0.f, sum_z = 0.f;
        int s_first = -1;
        for (uint32_t k = 0; k < nsamples; ++k) {
            const float4 j = jitter[k];
            f3 o = cam;
            if (lens) {
                const float4 l = lens_tab[k];
                o = mk(l.x, l.y, l.z);
            }
            const f3 d = sub(add(corner, mk(j.x, j.y, j.z)), o);
            const float aa = dot(d, d);
            float max_t = kInfinity;
            int best = -1;
            // (a pinhole ray starts at the camera centre: the host hands out prim_info only to
            // a bounded scene and a centre within 2^30, the other half of the range guard)
            const bool cam_now = (inf & 15u) != 15u && guard_a(aa);
            if (cam_now) {
                ++listed;
                cfloat4* crec = (cfloat4*)S.cam_rec;
                const float ya = recip_a(aa);
                const v2f dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z}, a2 = {aa, aa};
                for (int gb = 0; gb < S.nbig; ++gb)  // the big spheres (scalar loads)
                    exact_group_uniform_cam(crec + 4 * gb, (cfloat4*)S.cgroup + 5 * gb, dx, dy,
                                            dz, a2, aa, ya, max_t, best);
                // the quarter's listed spheres, two per record (primary.cpp)
                const uint32_t cnt = inf & 15u;
                const float4* lr = S.cam_rec + 4u * (uint32_t)S.nbig + 3u * (inf >> 4);
                uint32_t iters = 0u;
                for (uint32_t m = 0; 2u * m < cnt; ++m) {
                    ++iters;
                    const float4 q0 = lr[3u * m], q1 = lr[3u * m + 1u], id = lr[3u * m + 2u];
                    v2f hb, cc, dc;
                    pair_disc_cam(dx, dy, dz, a2, q0, q1, hb, cc, dc);
                    if (__float_as_int(hit_sign(hb.x, cc.x, dc.x)) < 0)
                        consider(candidate_t_fast(hb.x, dc.x, aa, ya), __float_as_int(id.x),
                                 max_t, best);
                    if (__float_as_int(hit_sign(hb.y, cc.y, dc.y)) < 0)
                        consider(candidate_t_fast(hb.y, dc.y, aa, ya), __float_as_int(id.y),
                                 max_t, best);
                }
                // issued work as the frame counts it: a pair test is half a group test
                tally(w_halves, 2u * (uint32_t)S.nbig + wave_max_small<3>(iters));
            } else {
                uint32_t hit_groups = 0u, lane_cnt = 0u;
                const bool guarded = (S.flags & kFlagSceneBounded) != 0 && aa >= 0x1p-20f &&
                                     aa <= 0x1p60f && fabsf(o.x) <= 0x1p30f &&
                                     fabsf(o.y) <= 0x1p30f && fabsf(o.z) <= 0x1p30f;
                if (S.ncgroups > 0 && __ballot(!guarded) == 0u) {
                    scan_culled_lane<false>(S, S.cbound, tgroup, o, d, max_t, best, w_halves,
                                            w_bounds, lane_cnt, hit_groups);
                } else {
                    scan_spheres<false>(S, nullptr, n, o, d, max_t, best, hit_groups);
                    tally(w_halves, 2u * (uint32_t)((n + 3) >> 2));
                }
            }
            // ---- the sample's rows: sky (functions.glsl:85-89) or the hit's ----
            if (best < 0) {
                const float len = sqrt_fast(aa);  // length(d)
                sum_a = add(sum_a, sky_factor(d.y / len));
                // (normal, depth and coverage add +0)
            } else {
                const float4 cr = S.center_radius[best], sh = S.shade[best];
                const float4 mat = S.material[best];
                const f3 point = add(scale(max_t, d), o);
                // shade_segment's normal: the unscaled division, else the full one (same bits)
                const f3 pcv = sub(point, mk(cr.x, cr.y, cr.z));
                const float yr = recip_a(cr.w);
                f3 normal = mk(div_a(pcv.x, cr.w, yr), div_a(pcv.y, cr.w, yr),
                               div_a(pcv.z, cr.w, yr));
                const float nmin = fminf(fminf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
                const float nmax = fmaxf(fmaxf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
                if (!((S.flags & kFlagRadiiSafe) != 0u && nmin >= 0x1p-40f && nmax <= 0x1p30f)) {
                    asm volatile("");
                    normal = divs(pcv, cr.w);
                }
                const bool glass = (int)mat.x == 3;
                sum_a = add(sum_a, glass ? mk(1.f, 1.f, 1.f) : mk(sh.x, sh.y, sh.z));
                sum_n = add(sum_n, normal);
                sum_z = sum_z + max_t;
                sum_c = sum_c + 1.0f;
            }
            if (k == 0u) s_first = best;
        }
        const float fn = (float)nsamples;
        if (p.albedo)
            p.albedo[px.out_index] =
                make_float4(sum_a.x / fn, sum_a.y / fn, sum_a.z / fn, sum_c / fn);
        if (p.normal_depth)
            p.normal_depth[px.out_index] =
                make_float4(sum_n.x / fn, sum_n.y / fn, sum_n.z / fn, sum_z / fn);
        if (p.sphere) p.sphere[px.out_index] = s_first;
    }
    // one atomic per wave and tally, into the block's slot (FeatureParams.tallies)
    unsigned long long nl = listed, wh = w_halves, wb = w_bounds;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nl += __shfl_xor(nl, off);
        wh += __shfl_xor(wh, off);
        wb += __shfl_xor(wb, off);
    }
    if (lane == 0) {
        unsigned long long* slot = p.tallies + 8u * (blockIdx.x & (kFeatureTallySlots - 1u));
        if (nl) atomicAdd(slot + 0, nl);
        if (wh) atomicAdd(slot + 1, wh / 2u);
        if (wb) atomicAdd(slot + 2, wb);
    }
}
#endif

// ---------------------------------------------------------------------------------------------
// The ambient visibility buffer (vcrt_draw_occlusion), a code-generation unit of its own (Makefile,
// part 10): the feature kernel's shape -- one wave per local 8x8 tile, one lane per slot, the
// pixel's n samples in index order, the first hit through frame_first_hit -- and after each
// sample its m any-hit rays from P = o + t d along d' = N + u_j, N the hit's normal turned
// against the ray, u_j the host's table (vcrt_ambient_dirs) read at wave-uniform indices, through
// the occlusion queries' scans with the far limit `reach`. A lane whose sample missed enters them
// occluded with a guarded dummy ray, as vcrt_occlude_rays' dead lanes do: it asks for nothing and
// counts nothing. The wave takes the culled scan when the scene has tables and every lane's
// (P, d') is in the guarded range, else the linear scan: the same answer (fact (6)). A lane keeps
// two integers, its samples that hit and its secondary rays that were occluded, so the plane's
// bits depend on the rays alone; two conversions, two divisions and one store at the end. No LDS.
#if !defined(VCRT_PART) || VCRT_PART == 10
extern "C" __global__ __launch_bounds__(256) void vcrt_frame_occlusion(
    OcclusionBufferParams p_arg) {
    // the arguments through a pointer to the kernarg segment, as trace_impl reads them
    (void)p_arg;
    const OcclusionBufferParams& p = *reinterpret_cast<const OcclusionBufferParams*>(
        (__attribute__((address_space(4))) const OcclusionBufferParams*)
            __builtin_amdgcn_kernarg_segment_ptr());
    const TraceParams& S = p.scene;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (lt >= S.local_tiles) return;  // (the whole wave)
    const uint32_t q = lt * 64u + lane;
    const Pixel px = pixel_of(q, (uint32_t)S.width, (uint32_t)S.height, S.tiles_x,
                              (uint32_t)S.world, (uint32_t)S.rank);
    const uint32_t nsamples = p.n, nsecondary = p.m;
    const bool lens = S.lens != nullptr;
    uint32_t w_halves = 0u, w_bounds = 0u, listed = 0u, hits = 0u, blocked = 0u;
    if (px.valid) {
        const f3 p00 = mk(S.cam[0], S.cam[1], S.cam[2]);
        const f3 du = mk(S.cam[3], S.cam[4], S.cam[5]);
        const f3 dv = mk(S.cam[6], S.cam[7], S.cam[8]);
        const f3 cam = mk(S.cam[9], S.cam[10], S.cam[11]);
        const f3 corner = viewport_corner(p00, du, dv, px.x, px.y);
        // the sphere list of the lane's 4x4 quarter (slot 8 y + x), as trace_impl reads it
        uint32_t inf = 15u;
        if (p.use_lists != 0u && !lens && S.prim_info != nullptr)
            inf = S.prim_info[2u * (lt * 4u + (((lane >> 5) & 1u) << 1) + ((lane >> 2) & 1u)) + 1u];
        const int n = S.nspheres;
        const float4* tgroup = S.cgroup + 5 * S.nbig;  // the hierarchy's group records
        cfloat4* jitter = (cfloat4*)S.jitter;           // wave-uniform indices: scalar loads
        cfloat4* lens_tab = (cfloat4*)S.lens;
        cfloat4* udir = (cfloat4*)p.dirs;
        const float T = p.reach;
        const bool any_reach = T > kMinT;  // else no root lies in (min_t, T): every ray is open
        for (uint32_t k = 0; k < nsamples; ++k) {
            const float4 j = jitter[k];
            f3 o = cam;
            if (lens) {
                const float4 l = lens_tab[k];
                o = mk(l.x, l.y, l.z);
            }
            const f3 d = sub(add(corner, mk(j.x, j.y, j.z)), o);
            const float aa = dot(d, d);
            float max_t = kInfinity;
            int best = -1;
            frame_first_hit(S, inf, tgroup, n, o, d, aa, max_t, best, listed, w_halves, w_bounds);
            const bool hit = best >= 0;
            if (hit) ++hits;
            if (__ballot(hit && any_reach) == 0u) continue;
            // ---- the hit's point and its normal turned against the ray ----
            f3 P = mk(0.f, 0.f, 0.f), N = mk(0.f, 0.f, 0.f);
            if (hit) {
                const float4 cr = S.center_radius[best];
                P = add(scale(max_t, d), o);
                // shade_segment's normal: the unscaled division, else the full one (same bits)
                const f3 pcv = sub(P, mk(cr.x, cr.y, cr.z));
                const float yr = recip_a(cr.w);
                N = mk(div_a(pcv.x, cr.w, yr), div_a(pcv.y, cr.w, yr), div_a(pcv.z, cr.w, yr));
                const float nmin = fminf(fminf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
                const float nmax = fmaxf(fmaxf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
                if (!((S.flags & kFlagRadiiSafe) != 0u && nmin >= 0x1p-40f && nmax <= 0x1p30f)) {
                    asm volatile("");
                    N = divs(pcv, cr.w);
                }
                if (dot(d, N) > 0.0f) N = mk(-N.x, -N.y, -N.z);
            }
            const bool p_guarded = (S.flags & kFlagSceneBounded) != 0 && fabsf(P.x) <= 0x1p30f &&
                                   fabsf(P.y) <= 0x1p30f && fabsf(P.z) <= 0x1p30f;
            // ---- the sample's secondary rays ----
            const uint32_t row = k * nsecondary;
            for (uint32_t s = 0; s < nsecondary; ++s) {
                const float4 u = udir[row + s];
                // a lane without a hit: occluded from the start, a guarded ray
                const f3 d2 = hit ? add(N, mk(u.x, u.y, u.z)) : mk(0.f, 1.f, 0.f);
                const float a2 = dot(d2, d2);
                const bool guarded = !hit || (p_guarded && a2 >= 0x1p-20f && a2 <= 0x1p60f);
                bool occ = !hit;
                if (S.ncgroups > 0 && __ballot(!guarded) == 0u)
                    occ = occlude_culled_lane(S, S.cbound, tgroup, P, d2, T, occ, w_halves,
                                              w_bounds);
                else
                    occ = occlude_linear(S, n, P, d2, T, occ, w_halves);
                if (hit && occ) ++blocked;
            }
        }
        // open = (hit samples' open rays) + m per sky sample = n m - blocked: integers, exact
        const uint32_t all = nsamples * nsecondary;
        const float v = (float)(all - blocked) / (float)all;
        p.visibility[px.out_index] = make_float4(v, v, v, (float)hits / (float)nsamples);
    }
    // one atomic per wave and tally, into the block's slot (OcclusionBufferParams.tallies)
    unsigned long long nl = listed, wh = w_halves, wb = w_bounds, nh = hits, nb = blocked;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nl += __shfl_xor(nl, off);
        wh += __shfl_xor(wh, off);
        wb += __shfl_xor(wb, off);
        nh += __shfl_xor(nh, off);
        nb += __shfl_xor(nb, off);
    }
    if (lane == 0) {
        unsigned long long* slot = p.tallies + 8u * (blockIdx.x & (kFeatureTallySlots - 1u));
        if (nl) atomicAdd(slot + 0, nl);
        if (wh) atomicAdd(slot + 1, wh / 2u);
        if (wb) atomicAdd(slot + 2, wb);
        if (nh) atomicAdd(slot + 3, nh);
        if (nb) atomicAdd(slot + 4, nb);
    }
}
#endif

// ---------------------------------------------------------------------------------------------
// The reprojection map (vcrt_draw_motion), a code-generation unit of its own (Makefile, part 12):
// the feature kernel's shape -- one wave per local 8x8 tile, one lane per slot -- for one ray per
// pixel, the centre ray (corner - camera centre: no jitter, no lens offset, so a lens renderer's
// map is the pinhole's; it takes no list, its lists do not exist). The first hit goes through
// frame_first_hit; the centre ray lies inside its quarter's footprint, so a pinhole frame's lists
// serve it. The hit's normal is the feature kernel's; the point the sphere's previous centre and
// radius put it at, or for the sky the ray's own direction from the previous centre, goes through
// motion_project (vcrt_math.h). Identity -- the same camera and a sphere whose previous centre and
// radius have the current bits, or the sky -- is written as such, not computed: (x, y, t or 1).
#if !defined(VCRT_PART) || VCRT_PART == 12
extern "C" __global__ __launch_bounds__(256) void vcrt_frame_motion(MotionParams p_arg) {
    // the arguments through a pointer to the kernarg segment, as trace_impl reads them
    (void)p_arg;
    const MotionParams& p = *reinterpret_cast<const MotionParams*>(
        (__attribute__((address_space(4))) const MotionParams*)
            __builtin_amdgcn_kernarg_segment_ptr());
    const TraceParams& S = p.scene;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (lt >= S.local_tiles) return;  // (the whole wave)
    const uint32_t q = lt * 64u + lane;
    const Pixel px = pixel_of(q, (uint32_t)S.width, (uint32_t)S.height, S.tiles_x,
                              (uint32_t)S.world, (uint32_t)S.rank);
    const bool lens = S.lens != nullptr;
    uint32_t w_halves = 0u, w_bounds = 0u, listed = 0u, hits = 0u, projected = 0u, same = 0u;
    if (px.valid) {
        const f3 p00 = mk(S.cam[0], S.cam[1], S.cam[2]);
        const f3 du = mk(S.cam[3], S.cam[4], S.cam[5]);
        const f3 dv = mk(S.cam[6], S.cam[7], S.cam[8]);
        const f3 cam = mk(S.cam[9], S.cam[10], S.cam[11]);
        const f3 corner = viewport_corner(p00, du, dv, px.x, px.y);
        // the sphere list of the lane's 4x4 quarter (slot 8 y + x), as trace_impl reads it
        uint32_t inf = 15u;
        if (p.use_lists != 0u && !lens && S.prim_info != nullptr)
            inf = S.prim_info[2u * (lt * 4u + (((lane >> 5) & 1u) << 1) + ((lane >> 2) & 1u)) + 1u];
        const int n = S.nspheres;
        const float4* tgroup = S.cgroup + 5 * S.nbig;  // the hierarchy's group records
        const f3 o = cam;
        const f3 d = sub(corner, o);
        const float aa = dot(d, d);
        float max_t = kInfinity;
        int best = -1;
        frame_first_hit(S, inf, tgroup, n, o, d, aa, max_t, best, listed, w_halves, w_bounds);
        const bool hit = best >= 0;
        if (hit) ++hits;
        MotionCamera mc;
        mc.center = mk(p.prev_cam[0], p.prev_cam[1], p.prev_cam[2]);
        mc.e = mk(p.prev_cam[3], p.prev_cam[4], p.prev_cam[5]);
        mc.nw = mk(p.prev_cam[6], p.prev_cam[7], p.prev_cam[8]);
        mc.nu = mk(p.prev_cam[9], p.prev_cam[10], p.prev_cam[11]);
        mc.nv = mk(p.prev_cam[12], p.prev_cam[13], p.prev_cam[14]);
        mc.num = p.prev_cam[15];
        const float key = (float)(best + 2);
        bool identity = p.same_camera != 0u;
        f3 Q = add(mc.center, d);  // the sky is a direction: no parallax
        if (hit) {
            const float4 cr = S.center_radius[best];
            const float* pr = p.prev + (size_t)p.prev_stride * (uint32_t)best;
            const float pcx = pr[0], pcy = pr[1], pcz = pr[2], prr = pr[3];
            identity = identity && __float_as_uint(pcx) == __float_as_uint(cr.x) &&
                       __float_as_uint(pcy) == __float_as_uint(cr.y) &&
                       __float_as_uint(pcz) == __float_as_uint(cr.z) &&
                       __float_as_uint(prr) == __float_as_uint(cr.w);
            const f3 point = add(scale(max_t, d), o);
            // shade_segment's normal: the unscaled division, else the full one (same bits)
            const f3 pcv = sub(point, mk(cr.x, cr.y, cr.z));
            const float yr = recip_a(cr.w);
            f3 normal = mk(div_a(pcv.x, cr.w, yr), div_a(pcv.y, cr.w, yr), div_a(pcv.z, cr.w, yr));
            const float nmin = fminf(fminf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
            const float nmax = fmaxf(fmaxf(fabsf(pcv.x), fabsf(pcv.y)), fabsf(pcv.z));
            if (!((S.flags & kFlagRadiiSafe) != 0u && nmin >= 0x1p-40f && nmax <= 0x1p30f)) {
                asm volatile("");
                normal = divs(pcv, cr.w);
            }
            Q = add(mk(pcx, pcy, pcz), scale(prr, normal));
        }
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
        if (identity) {
            m = make_float4((float)px.x, (float)px.y, hit ? max_t : 1.0f, key);
            ++same;
            ++projected;
        } else {
            f3 r;
            if (motion_project(mc, sub(Q, mc.center), &r)) {
                m = make_float4(r.x, r.y, r.z, key);
                ++projected;
            }
        }
        if (p.motion) p.motion[px.out_index] = m;
        if (p.surface) p.surface[px.out_index] = make_float4(key, hit ? max_t : 0.0f, 0.f, 0.f);
    }
    // one atomic per wave and tally, into the block's slot (MotionParams.tallies)
    unsigned long long nl = listed, wh = w_halves, wb = w_bounds, nh = hits, np = projected,
                       ni = same;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nl += __shfl_xor(nl, off);
        wh += __shfl_xor(wh, off);
        wb += __shfl_xor(wb, off);
        nh += __shfl_xor(nh, off);
        np += __shfl_xor(np, off);
        ni += __shfl_xor(ni, off);
    }
    if (lane == 0) {
        unsigned long long* slot = p.tallies + 8u * (blockIdx.x & (kFeatureTallySlots - 1u));
        if (nl) atomicAdd(slot + 0, nl);
        if (wh) atomicAdd(slot + 1, wh / 2u);
        if (wb) atomicAdd(slot + 2, wb);
        if (nh) atomicAdd(slot + 3, nh);
        if (np) atomicAdd(slot + 4, np);
        if (ni) atomicAdd(slot + 5, ni);
    }
}
#endif

// ---------------------------------------------------------------------------------------------
// Adaptive sampling (vcrt_draw_samples), a code-generation unit of its own (Makefile, part 15):
// for every local pixel n_p = min(counts[p], max_count) further samples of the frame's own rays,
// summed in quanta of kSampleQuantum (vcrt.h states the order). Three kernels:
//   vcrt_sample_scan     the exclusive prefix of ceil(n_p / 4) over the local slots, the item
//                        table (slot, quantum) and the totals;
//   vcrt_trace_samples   vcrt_trace_rays' persistent grid over the items: a lane runs its item's
//                        up to four paths one after another, keeps the quantum's sum in registers
//                        and stores one float4 per item. The rays are vcrt_frame_features'
//                        ((corner + jitter_i) - origin), the first segment goes through
//                        frame_first_hit, every segment through shade_segment;
//   vcrt_sample_resolve  one lane per local slot adds its quanta in ascending k and applies the
//                        accumulate rule.
// A pixel's quanta are items of their own, so a pixel with many samples spreads over lanes and
// waves; the bits depend on the item's sample indices only, not on who traced it.
// Bounds: a slot q < total_pixels indexes offsets; counts, sums and mean are read and written at
// pixel_of's out_index of valid slots only (< elements); an item index is below count before the
// item, the scratch or the tables are touched; a table index 4 k + j is below n_p <= max_count.
#if !defined(VCRT_PART) || VCRT_PART == 15
namespace {

// Exclusive prefix of v over the 256 threads of the block (every thread calls), and the total.
__device__ __forceinline__ uint32_t block_prefix(uint32_t v, uint32_t& total, uint32_t* wave_tot) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= (uint32_t)off) x += y;
    }
    __syncthreads();  // the previous call's reads are done
    if (lane == 63u) wave_tot[wave] = x;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kSampleScanBlock / 64u; ++w) {
        const uint32_t t = wave_tot[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    total = all;
    return before + x - v;
}

// n_p of local slot q: 0 outside the frame
__device__ __forceinline__ uint32_t sample_count_of(const uint16_t* counts, uint32_t max_count,
                                                    const Pixel& px) {
    if (!px.valid) return 0u;
    const uint32_t c = counts[px.out_index];
    return c < max_count ? c : max_count;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void vcrt_sample_scan(SampleScanParams p) {
    __shared__ uint32_t wave_tot[kSampleScanBlock / 64u];
    __shared__ unsigned long long red[2][kSampleScanBlock / 64u];
    const uint32_t t = threadIdx.x;
    if (p.phase == 1u) {  // one block: block_sums' quanta -> their exclusive prefix; the totals
        unsigned long long carry = 0ull, my_s = 0ull, my_p = 0ull;
        for (uint32_t base = 0; base < p.blocks; base += kSampleScanBlock) {
            const uint32_t b = base + t;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (b < p.blocks) v = p.block_sums[b];
            uint32_t total;
            const uint32_t ex = block_prefix(v.x, total, wave_tot);
            if (b < p.blocks) p.block_sums[b].x = (uint32_t)(carry + ex);
            carry += total;
            my_s += v.y;
            my_p += v.z;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            my_s += __shfl_xor(my_s, off);
            my_p += __shfl_xor(my_p, off);
        }
        if ((t & 63u) == 0u) {
            red[0][t >> 6] = my_s;
            red[1][t >> 6] = my_p;
        }
        __syncthreads();
        if (t == 0u) {
            unsigned long long s = 0ull, n = 0ull;
            for (uint32_t w = 0; w < kSampleScanBlock / 64u; ++w) {
                s += red[0][w];
                n += red[1][w];
            }
            p.totals[0] = s;
            p.totals[1] = n;
            p.totals[2] = carry;
            p.totals[3] = 0ull;
        }
        return;
    }
    // phases 0 and 2: four consecutive slots per thread
    const uint32_t q0 = blockIdx.x * kSampleScanSlots + 4u * t;
    uint32_t n[4], quanta = 0u, samples = 0u, pixels = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        n[i] = 0u;
        const uint32_t q = q0 + i;
        if (q < p.total_pixels) {
            const Pixel px = pixel_of(q, (uint32_t)p.width, (uint32_t)p.height, p.tiles_x,
                                      (uint32_t)p.world, (uint32_t)p.rank);
            n[i] = sample_count_of(p.counts, p.max_count, px);
        }
        quanta += (n[i] + kSampleQuantum - 1u) / kSampleQuantum;
        samples += n[i];
        pixels += n[i] != 0u ? 1u : 0u;
    }
    uint32_t total;
    const uint32_t ex = block_prefix(quanta, total, wave_tot);
    if (p.phase == 0u) {
        uint32_t s = samples, c = pixels;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s += __shfl_xor(s, off);
            c += __shfl_xor(c, off);
        }
        if ((t & 63u) == 0u) {
            red[0][t >> 6] = s;
            red[1][t >> 6] = c;
        }
        __syncthreads();
        if (t == 0u) {
            unsigned long long ss = 0ull, cc = 0ull;
            for (uint32_t w = 0; w < kSampleScanBlock / 64u; ++w) {
                ss += red[0][w];
                cc += red[1][w];
            }
            p.block_sums[blockIdx.x] = make_uint4(total, (uint32_t)ss, (uint32_t)cc, 0u);
        }
        return;
    }
    uint32_t off = p.block_sums[blockIdx.x].x + ex;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t q = q0 + i;
        if (q >= p.total_pixels) break;
        p.offsets[q] = off;
        const uint32_t nq = (n[i] + kSampleQuantum - 1u) / kSampleQuantum;
        for (uint32_t k = 0; k < nq; ++k) {
            const uint32_t left = n[i] - kSampleQuantum * k;
            const uint32_t m = left < kSampleQuantum ? left : kSampleQuantum;
            p.items[off + k] = make_uint2(q, k | (m << 16));
        }
        off += nq;
    }
}

extern "C" __global__ __launch_bounds__(256) void vcrt_trace_samples(SampleTraceParams p_arg) {
    // the arguments through a pointer to the kernarg segment, as trace_impl reads them
    (void)p_arg;
    const SampleTraceParams& p = *reinterpret_cast<const SampleTraceParams*>(
        (__attribute__((address_space(4))) const SampleTraceParams*)
            __builtin_amdgcn_kernarg_segment_ptr());
    const TraceParams& S = p.scene;
    const uint32_t lane = threadIdx.x & 63u;
    if (S.max_depth <= 0) {  // ray_color's undefined return (canonical 0): every quantum sums 0
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.count;
             i += gridDim.x * blockDim.x)
            p.scratch[i] = make_float4(0.f, 0.f, 0.f, (float)(p.items[i].y >> 16));
        return;
    }
    const int n = S.nspheres;
    const float4* tgroup = S.cgroup + 5 * S.nbig;  // the hierarchy's group records
    const bool lens = S.lens != nullptr;
    const bool lists = p.use_lists != 0u && !lens && S.prim_info != nullptr;
    const f3 p00 = mk(S.cam[0], S.cam[1], S.cam[2]);
    const f3 du = mk(S.cam[3], S.cam[4], S.cam[5]);
    const f3 dv = mk(S.cam[6], S.cam[7], S.cam[8]);
    const f3 cam = mk(S.cam[9], S.cam[10], S.cam[11]);
    bool need = true, done = false, fresh = false;
    uint32_t idx = 0u;
    // the lane's item: its pixel's corner and list word, the table index of its next sample, the
    // samples it has left and the quantum's sum so far
    f3 corner = mk(0.f, 0.f, 0.f), qsum = mk(0.f, 0.f, 0.f);
    uint32_t inf = 15u, tab = 0u, left = 0u, item_m = 0u;
    f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 1.f, 0.f), atten = mk(1.f, 1.f, 1.f);
    int pass = 0;
    uint32_t segs = 0u, listed = 0u;  // this lane's, all its items
    uint32_t w_halves = 0u, w_bounds = 0u;
    for (;;) {
        // ---- lanes whose item has ended take the next items: one atomic per wave ----
        const uint64_t need_mask = __ballot(need && !done);
        if (need_mask != 0u) {
            const int leader = __builtin_ctzll(need_mask);
            uint32_t base = 0u;
            if ((int)lane == leader) base = atomicAdd(p.work, (uint32_t)__popcll(need_mask));
            base = __builtin_amdgcn_readfirstlane(__shfl(base, leader));
            if (need && !done) {
                idx = base + lanes_below(need_mask);
                if (idx < p.count) {
                    const uint2 it = p.items[idx];
                    const uint32_t q = it.x;
                    const Pixel px = pixel_of(q, (uint32_t)S.width, (uint32_t)S.height, S.tiles_x,
                                              (uint32_t)S.world, (uint32_t)S.rank);
                    // shader.comp:43's pixel corner, vcrt_setup_jitter's operations
                    corner = viewport_corner(p00, du, dv, px.x, px.y);
                    // the sphere list of the slot's 4x4 quarter, as vcrt_frame_features reads it
                    inf = 15u;
                    if (lists) {
                        const uint32_t lt = q >> 6, slot = q & 63u;
                        inf = S.prim_info[2u * (lt * 4u + (((slot >> 5) & 1u) << 1) +
                                                ((slot >> 2) & 1u)) + 1u];
                    }
                    tab = kSampleQuantum * (it.y & 0xffffu);
                    item_m = it.y >> 16;
                    left = item_m;
                    qsum = mk(0.f, 0.f, 0.f);
                    fresh = true;
                    need = false;
                } else {  // no item left: nothing more is stored, and the ray held is guarded
                    done = true;
                    o = mk(0.f, 0.f, 0.f);
                    d = mk(0.f, 1.f, 0.f);
                }
            }
        }
        if (__ballot(!done) == 0u) break;
        if (done) continue;

        // ---- first segments that have a camera-ray list, ahead of the scan: a lane starting a
        // sample takes its first hit from its quarter's list and shades it here, so that the
        // scan below serves its second segment together with the other lanes' later ones (a
        // wave's lanes start their samples at different times: taken inside the scan's step
        // the list route would cost every iteration both routes' time). A sample that ends on
        // its first segment makes the lane start its next one: at most four trips per item.
        for (;;) {
            if (fresh) {  // the item's next sample: vcrt_frame_features' camera ray
                const float4 j = S.jitter[tab];
                o = cam;
                if (lens) {
                    const float4 l = S.lens[tab];
                    o = mk(l.x, l.y, l.z);
                }
                d = sub(add(corner, mk(j.x, j.y, j.z)), o);
                atten = mk(1.f, 1.f, 1.f);
                pass = 0;
            }
            const float aa = dot(d, d);
            const bool cam_seg = fresh && !need && (inf & 15u) != 15u && guard_a(aa);
            if (__ballot(cam_seg) == 0u) break;
            if (cam_seg) {
                ++segs;
                float max_t = kInfinity;
                int best = -1;
                frame_first_hit(S, inf, tgroup, n, o, d, aa, max_t, best, listed, w_halves,
                                w_bounds);
                fresh = false;
                f3 normal = mk(0.f, 0.f, 0.f), contrib = mk(0.f, 0.f, 0.f);
                bool ended = shade_segment(S, max_t, best, o, d, atten, normal, contrib);
                if (!ended) {
                    ++pass;
                    ended = pass >= S.max_depth;  // undefined GLSL return -> vec3(0)
                }
                if (ended) {
                    qsum = add(qsum, contrib);  // S_k, in index order
                    ++tab;
                    --left;
                    if (left != 0u) {
                        fresh = true;
                    } else {
                        p.scratch[idx] = make_float4(qsum.x, qsum.y, qsum.z, (float)item_m);
                        need = true;
                    }
                }
            }
        }
        if (need) continue;  // the item ended on a first segment: the next claim

        // ---- one segment by the scans of vcrt_trace_rays (frame_first_hit with no list word):
        // a first segment without a list, and every later one ----
        ++segs;
        float max_t = kInfinity;
        int best = -1;
        frame_first_hit(S, 15u, tgroup, n, o, d, dot(d, d), max_t, best, listed, w_halves,
                        w_bounds);
        fresh = false;

        // ---- shade (textures.glsl) or sky (functions.glsl:85-89) ----
        f3 normal = mk(0.f, 0.f, 0.f), contrib = mk(0.f, 0.f, 0.f);
        bool ended = shade_segment(S, max_t, best, o, d, atten, normal, contrib);
        if (!ended) {
            ++pass;
            ended = pass >= S.max_depth;  // undefined GLSL return -> vec3(0)
        }
        if (ended) {
            qsum = add(qsum, contrib);  // S_k, in index order
            ++tab;
            --left;
            if (left != 0u) {
                fresh = true;
            } else {
                p.scratch[idx] = make_float4(qsum.x, qsum.y, qsum.z, (float)item_m);
                need = true;
            }
        }
    }
    // one atomic per wave and tally, into the block's slot (SampleTraceParams.tallies)
    unsigned long long nl = listed, wh = w_halves, wb = w_bounds, total = segs;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nl += __shfl_xor(nl, off);
        wh += __shfl_xor(wh, off);
        wb += __shfl_xor(wb, off);
        total += __shfl_xor(total, off);
    }
    if (lane == 0) {
        unsigned long long* slot = p.tallies + 8u * (blockIdx.x & (kFeatureTallySlots - 1u));
        if (nl) atomicAdd(slot + 0, nl);
        if (wh) atomicAdd(slot + 1, wh / 2u);
        if (wb) atomicAdd(slot + 2, wb);
        if (total) atomicAdd(slot + 3, total);
    }
}

extern "C" __global__ __launch_bounds__(256) void vcrt_sample_resolve(SampleResolveParams p) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= p.total_pixels) return;
    const Pixel px = pixel_of(q, (uint32_t)p.width, (uint32_t)p.height, p.tiles_x,
                              (uint32_t)p.world, (uint32_t)p.rank);
    if (!px.valid) return;  // slots outside the frame are neither read nor written
    const uint32_t np = sample_count_of(p.counts, p.max_count, px);
    const uint32_t nq = (np + kSampleQuantum - 1u) / kSampleQuantum;
    const float4* sk = p.scratch + p.offsets[q];
    f3 s = mk(0.f, 0.f, 0.f);
    for (uint32_t k = 0; k < nq; ++k) {  // S_p: from +0, ascending k
        const float4 v = sk[k];
        s = add(s, mk(v.x, v.y, v.z));
    }
    float4 out = make_float4(s.x, s.y, s.z, (float)np);
    if (p.accumulate != 0u) {
        const float4 old = p.sums[px.out_index];
        out = np != 0u ? make_float4(old.x + s.x, old.y + s.y, old.z + s.z, old.w + (float)np)
                       : old;
    }
    if (p.accumulate == 0u || np != 0u) p.sums[px.out_index] = out;
    if (p.mean)
        p.mean[px.out_index] = out.w == 0.0f
                                   ? make_float4(0.f, 0.f, 0.f, 1.f)
                                   : make_float4(out.x / out.w, out.y / out.w, out.z / out.w, 1.f);
}
#endif

// ---------------------------------------------------------------------------------------------
// Self-test of unit_of (the scatter's unit vector) on caller-supplied triples, a code-generation
// unit of its own (Makefile, part 9): out[i] = unit_of(in[i]), to be compared on the host with
// the correctly rounded sqrt and divisions.
#if !defined(VCRT_PART) || VCRT_PART == 9
extern "C" __global__ __launch_bounds__(256) void vcrt_check_unit(UnitCheckParams p) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.count; i += stride) {
        const f3 u = unit_of(mk(p.in[3u * i], p.in[3u * i + 1u], p.in[3u * i + 2u]));
        p.out[3u * i] = u.x;
        p.out[3u * i + 1u] = u.y;
        p.out[3u * i + 2u] = u.z;
    }
}
#endif
