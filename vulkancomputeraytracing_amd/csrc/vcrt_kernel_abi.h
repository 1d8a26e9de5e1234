// vcrt_kernel_abi.h -- argument blocks passed by value to the gfx950 kernels of
// vcrt_tracer.hsaco (host: capi.cpp via hipModuleLaunchKernel; device: tracer.hip).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#endif

namespace vcrt {

// The frame is cut into 8x8 pixel tiles (tx, ty). Rank r of world owns the tiles with
// (tx + ty) % world == r, numbered row-major as local tiles lt (vcrt_math.h tile_of /
// owner_of). Work items are (local tile, sample
// chunk, slot): 64 consecutive items are one tile at one chunk of samples, one lane per pixel.
// Rank-local framebuffer: world == 1 -> the frame itself, row-major [H][W]; world > 1 -> packed
// tiles [local_tiles][64] (slot = 8 * (y % 8) + x % 8), re-interleaved by vcrt_assemble.
struct TraceParams {
    const float4* geom;           // pair-SoA sphere groups (+1 padding group), scan input
    const float4* center_radius;  // [n] (center.xyz, radius)           -- read once per hit
    const float4* shade;          // [n] (colour.rgb, texture.y = param)
    const float4* material;       // [n] (texture.x = material id, 1 / texture.y, Schlick r0^2
                                  //   of texture.y, 0): the glass quotients precomputed (fp32)
    // shader.comp:43-49's viewport point pixel00 + x delta_u + y delta_v + jx delta_u + jy delta_v
    // is the sum of two fp32 terms: the pixel's corner (the `corner` table below for the culled
    // scans, computed at each sample start by the linear ones) and the sample's jitter term, a
    // table (vcrt_setup_jitter, the kernel's own operations)
    const float4* jitter;  // [spp] jx delta_u + jy delta_v, (jx, jy) = (-0.5+rand(i,i),
                           //   -0.5+rand(i+1,i+1)) of sample index i (shader.comp:48)
    float4* out;           // rank-local framebuffer, rgba32f (layout above)
    double* accum;         // [local_tiles * 64][4] exact sums of the quantized quantum sums (r,
                           //   g, b, unused), vcrt_math.h "Accumulation"; unused with kFlagDirect
    uint32_t* work;        // eight work-queue counters kQueueStride apart, zeroed every launch
    unsigned long long* segments;  // ray segments traced, zeroed before every launch
    unsigned long long* debug;     // diagnostics counters (stats kernels only), may be null
    unsigned long long* work_done;  // [2]: sphere groups tested, group bounds tested
    // spatially clustered copy of the scene for the culled scan (kernel variant CULL)
    const float4* cgroup;   // [(nbig + ncgroups) * 5] per group: four pair-SoA float4s
                            //   (cx0,cx1,cy0,cy1) (cz0,cz1,r0^2,r1^2) (cx2..) (cz2..) + the
                            //   members' world[] indices as int bits (-1 = padding); the nbig
                            //   big-sphere groups first, then the hierarchy in spatial order
    const float4* cbound;   // [ncgroups / 2 * 4] boxes of group pairs, pair-SoA:
                            //   (lox0,lox1,loy0,loy1) (loz0,loz1,hix0,hix1) (hiy0,hiy1,hiz0,hiz1)
                            //   (K0,K1,0,0), K = 8.1u / r_min of the box's members
    const float4* cbound_nf;  // [ncgroups / 2 * 5] the same group-pair boxes for the flat
                              //   scan's near/far reads: per axis (lo0,lo1,hi0,hi1,lo0,lo1),
                              //   x then y then z, then (K0,K1) -- 80 B per pair
    const float4* cnode;    // [ncgroups / 16 * 4] boxes of node pairs (8 groups per node)
    const float4* ctop;     // boxes of pairs of 64-group chunks, same form
    const float4* cnode_nf;  // [ceil(ncgroups / 64) * 4 * 5] the node-pair boxes in the near/far
                             //   layout of cbound_nf, padded to whole chunks (the flat scan's
                             //   chunk passes)
    const uint32_t* prim_info;  // [4 local_tiles][2] camera-ray lists of each 4x4 quarter
                                //   (4 lt + 2 qy + qx) of each local tile, or null: [0] the
                                //   hierarchy groups (main scan) as offset << 4 | count (<= 8),
                                //   [1] the spheres (camera fast trace) as first pair << 4 |
                                //   count (<= 14); 15 = no list. Null also when the scene is
                                //   not bounded or a |component| of the camera centre exceeds
                                //   2^30: with the lists the host vouches for that half of the
                                //   camera rays' range guard (capi.cpp trace_frame)
    const uint16_t* prim_ids;   // hierarchy group indices of the group lists
    const float4* cam_rec;      // with the lists: [nbig * 4] the big groups' camera-relative
                                //   records, pair-SoA (ocx0,ocx1,ocy0,ocy1) (ocz0,ocz1,cc0,cc1)
                                //   (..2,3..) with oc = camera centre - centre, cc = |oc|^2 - r^2,
                                //   fp32 as pair_disc_cc computes them; then the sphere lists'
                                //   pair records [pairs * 3]: (ocx0,ocx1,ocy0,ocy1)
                                //   (ocz0,ocz1,cc0,cc1) (index0, index1 as int bits, 0, 0)
                                //   (cluster.hpp build_camera_records / build_primary_sphere_lists)
    float box_margin[4];    // max |centre|, r_max^2, max |box coordinate|, 0 (rounded up)
    int32_t ncgroups;       // hierarchy groups, multiple of 16
    int32_t nbig;           // big-sphere groups tested for every ray
    int32_t nspheres;
    int32_t width, height, spp, max_depth;
    int32_t rank, world;
    uint32_t tiles_x;      // ceil(width / 8)
    uint32_t local_tiles;  // tiles owned by this rank
    uint32_t total_items;  // local_tiles * 64 * (nchunks + tail_nchunks)
    int32_t chunk;         // samples per work item (<= kAccumMaxChunk) of the head
    int32_t nchunks;       // ceil(tail_start / chunk)
    // The tail: samples tail_start .. spp-1 of every pixel in chunks of tail_chunk (tail_nchunks
    // of them), handed out after all head blocks (the first blocks_head = local_tiles *
    // nchunks). No tail: tail_start = spp, tail_nchunks = 0.
    int32_t tail_start, tail_chunk, tail_nchunks;
    uint32_t blocks_head;
    // the accumulation quantum G - 1 (G a power of two): a lane's fp32 sum is quantized and added
    // to the pixel's sums at every sample index that is a multiple of G (vcrt_math.h
    // "Accumulation"); items hold whole quanta
    uint32_t quantum_mask;
    uint32_t flags;        // kFlag*; bits 24..31: s + 128, the quantization scale 2^s every
                           //   pixel's quantum sums start at (vcrt_math.h "Accumulation":
                           //   2^32; kFlagPixelScale: each pixel's own from pixel_emax), kept in
                           //   the flags word the retire reads anyway (no load of its own)
    float spp_total;       // kFlagDirect: the divisor (samples per pixel)
    float cam[12];         // pixel00.xyz, delta_u.xyz, delta_v.xyz, center.xyz
    // Per-wave accumulation ring in LDS (tracer.hip "Accumulation ring"): ring_n entries of 32 B
    // per wave (0: none; <= kRingMaxEntries) at byte ring_off of the dynamic LDS, wave w of the
    // workgroup at ring_off + 32 ring_n w. Needs local pixels < 2^kRingQBits.
    uint32_t ring_off, ring_n;
    // The linear SMEM scan's staging (small scenes, C2): when stage_spp != 0 the kernel copies
    // the shading tables of the stage_spheres spheres (center_radius, shade, material: 48 B each)
    // and the jitter table (stage_spp float4) to the start of the dynamic LDS and reads them
    // there: the per-hit and per-sample reads leave global memory (L2 latency on every bounce).
    uint32_t stage_spheres, stage_spp;
    double sin_c[13];  // vcrt_math.h kSinC: the fast sine's constants, read by scalar loads
    const float4* corner;  // [local_tiles * 64] pixel00 + x delta_u + y delta_v per local slot
                           //   (shader.comp:43; vcrt_setup_jitter, the kernel's own operations)
    // chunk-minor slots: (i * nch_magic[part]) >> 32 = i / nchunks of the head (0) / the tail (1)
    // for every item index i < 64 nchunks (host-checked; 0: the kernel divides)
    uint32_t nch_magic[2];
    // deferred fetches (the flat scans): a wave whose lanes still have work fetches items only
    // once fetch_min lanes need one or it has deferred fetch_wait iterations (1, 0: every time)
    uint32_t fetch_min, fetch_wait;
    // stats builds only (VCRT_DEBUG_STATS=1): [waves][88] region entry counts (tracer.hip
    // reg::*), zeroed before the launch; null otherwise
    uint32_t* region;
    // the cost-ordered schedule (drain-bound frames, capi.cpp "cost order"): pixel_cost, when
    // set, receives each local pixel's segments (u32, modular: an item subtracts the lane's
    // segment count at its start and adds it at its end); block_order, when set, maps the k-th
    // block a part hands out to the block of that part to run (the reverse flag is then off)
    uint32_t* pixel_cost;
    const uint32_t* block_order;
    // Outlier quanta (vcrt_math.h "Accumulation"): a quantum sum with |S * 2^s| >= 2^44 (finite)
    // atomicMax-es the float bits of its largest |channel| into pixel_emax[local pixel] and into
    // *outlier_max; with kFlagPixelScale every pixel quantizes at pixel_scale_log2(pixel_emax[.])
    // instead of the flags' scale
    uint32_t* pixel_emax;
    uint32_t* outlier_max;
    // The shared y slab of the flat scans (cluster.hpp CullTables::slab): with kFlagSlab every
    // non-padding group, node and chunk box has lo.y = slab[0] and hi.y = slab[1], and the flat
    // scans compute the two y-plane terms once per ray (tracer.hip box_ray, fact (3a)). Last in
    // the block, so a code object built before them reads the same layout.
    float slab[2];
    // The footprint tables of the LDS-table flat scan (cluster.hpp CullTables::fp_*; tracer.hip
    // fact (5)): fp_tab holds four tables of kFootCells node masks (x: lo <= cell, hi >= cell; z
    // the same), 16-bit when the scene has at most 16 nodes (ncgroups <= 128), else 32-bit;
    // fp_x / fp_z the cells' (scale, offset); fp_y the y extent of all node boxes with members;
    // fp_k2 twice their largest finite K; fp_always the nodes every ray keeps. After the slab,
    // for the same reason.
    const uint32_t* fp_tab;
    float fp_x[2], fp_z[2], fp_y[2];
    float fp_k2;
    uint32_t fp_always;
    // The group-level footprint tables (kFlagGroupFoot; cluster.hpp CullTables::gf_*; tracer.hip
    // fact (5g)): four tables of gf_n 128-bit group masks (bit = hierarchy group index; x: lo <=
    // cell, hi >= cell; z the same), which take the place of the group boxes and the node tables
    // in the LDS-table kernel's image (group_foot_cells); gf_x / gf_z the cells' (scale, offset);
    // gf_k2 twice the group boxes' largest finite K; gf_always the groups every ray keeps. The y
    // extent is fp_y (one height: every group box has it). Last in the block, as the fields above.
    const uint4* gf_tab;
    float gf_x[2], gf_z[2];
    float gf_k2;
    uint32_t gf_n;
    uint32_t gf_always[4];
    // The thin lens (vcrt.h lens_radius > 0; the *_lens kernels only): [spp] the ray origin of
    // each sample index of the frame, camera centre + lens offset (vcrt_math.h lens_offset, built
    // on the host with the same fp32 operations), w = 0; indexed as jitter is. Null for the
    // pinhole, whose kernels do not read it. Last in the block, as the fields above.
    const float4* lens;
};

constexpr uint32_t kQueueStride = 32;  // u32s between the work-queue counters (128 B)
#ifndef VCRT_QUEUES
#define VCRT_QUEUES 32
#endif
// work queues (a power of two): queue x serves workgroups x, x + kQueues, ..., which all sit
// on XCD x % 8; 32 (four per XCD) measured at or above 8 and 16 (profiles/r03_ab_log.md)
constexpr uint32_t kQueues = VCRT_QUEUES;
constexpr uint32_t kMaxQueues = 32;        // counters the host allocates and zeroes
constexpr uint32_t kRingMaxEntries = 63;  // entry + 1 in the top 6 bits of a lane's pixel index
constexpr uint32_t kRingQBits = 26;
// the kernel masks a queue index with kQueues - 1 and the host zeroes kMaxQueues counters
static_assert((kQueues & (kQueues - 1u)) == 0u && kQueues >= 1u && kQueues <= kMaxQueues,
              "VCRT_QUEUES: a power of two <= kMaxQueues");
static_assert(kRingMaxEntries + 1u <= (1u << (32u - kRingQBits)), "ring entry field");

constexpr int32_t kFlatMaxGroups = 1024;   // CULL_FLAT 16-bit entries: 10-bit group / node fields
constexpr int32_t kFlatMaxGroups8 = 256;   // the LDS-table kernel: 8-bit fields, 16-bit candidates
constexpr uint32_t kFootCells = 84;  // cells per footprint table: 4 x 84 16-bit masks take the
                                     // 672 B of the final scene's two chunk records they replace
// bytes of the footprint tables in the LDS-table kernel's image
constexpr uint32_t foot_lds_bytes(int32_t ncgroups) {
    return 4u * kFootCells * (ncgroups > 128 ? 4u : 2u);
}
// cells per group-level footprint table (four tables of 16-B masks): what fits in the bytes of
// the group boxes (336 B per node) and the node tables they replace, so that the LDS image keeps
// its size; 94 at the final scene's 128 groups
constexpr uint32_t kGroupFootMaxGroups = 128;
constexpr uint32_t group_foot_cells(int32_t ncgroups) {
    return (static_cast<uint32_t>(ncgroups) / 8u * 336u + foot_lds_bytes(ncgroups)) / 64u;
}
// The group tables' zero row (tracer.hip group_foot_mask): one all-zero 16-B mask behind the four
// tables, at cell 4 gf_n of the LDS image, which a ray that never reaches the y extent reads in
// place of its first row. The 64-B division above leaves it room except where the tables fill the
// bytes exactly (groups / 8 = 2, 6, 10, 14): there the image grows by this one float4, ahead of
// the group records. 0 at the final scene's 128 groups (32 B to spare).
constexpr uint32_t group_foot_zero_pad(int32_t ncgroups) {
    if (ncgroups <= 0 || static_cast<uint32_t>(ncgroups) > kGroupFootMaxGroups) return 0u;
    const uint32_t bytes = static_cast<uint32_t>(ncgroups) / 8u * 336u + foot_lds_bytes(ncgroups);
    return bytes - 64u * group_foot_cells(ncgroups) >= 16u ? 0u : 1u;
}
// v_bitop3_b32's truth-table bytes (bit 4 x + 2 y + z of the byte is the result for operand bits
// x, y, z) of the two forms the footprint masks are combined with
constexpr uint32_t kBitopAnd3 = 0x80;   // x & y & z
constexpr uint32_t kBitopAndOr = 0xea;  // (x & y) | z
constexpr uint32_t kWaveScratchBytes = 4360;  // CULL_FLAT per-wave LDS stacks, 16-bit entries
constexpr uint32_t kWaveScratchBytes8 = 3464;  // 16-bit candidates, no chunk stack (LDS tables)
constexpr uint32_t kWaveScratchBytesWide = 6920;  // the same with 32-bit entries (global tables)
constexpr uint32_t kFlagReverseOrder = 1u;  // hand out work items last-to-first
constexpr uint32_t kFlagSceneBounded = 2u;  // every |center|, radius <= 2^30 (host-checked)
constexpr uint32_t kFlagChunkMinor = 8u;  // a block's 64 items run chunk-minor: all chunks of
                                          // 64 / nchunks pixels (else one chunk of 64 pixels)
constexpr uint32_t kFlagRadiiSafe = 16u;  // every |radius| in [2^-40, 2^30] (host-checked):
                                         // shading's (p - c) / r may take the unscaled division
constexpr uint32_t kFlagScaleShift = 24u;  // TraceParams.flags: s + kFlagScaleBias
constexpr int32_t kFlagScaleBias = 128;
constexpr uint32_t kFlagPixelScale = 32u;  // per-pixel scales from TraceParams.pixel_emax
constexpr uint32_t kFlagSlab = 64u;  // the boxes share their y extent, TraceParams.slab (a bit
                                     // of the flags word the scans hold anyway: no load, no
                                     // register of its own)
constexpr uint32_t kFlagGroupFoot = 128u;  // the LDS-table flat scan takes each ray's groups from
                                           // TraceParams.gf_* (no node level, no box test); the
                                           // frame's camera rays have their lists
constexpr uint32_t kFlagDirect = 4u;  // one work item per pixel and frame, not progressive: the
                                      // lane writes the pixel itself (no sums, no resolve pass)

// Ray queries (vcrt_trace_rays): ray_color and the first hit of caller-supplied rays. The scene
// block is a TraceParams filled as a frame's is (the scan tables, the shading rows, the flags'
// scene bits, box_margin, slab, sin_c, nspheres, ncgroups, nbig) with max_depth the query's
// depth; the frame fields (out, accum, work, jitter, corner, the camera lists, ...) are null.
// The scan helpers of tracer.hip take it as they take a frame's.
struct RayQueryParams {
    TraceParams scene;
    const float* origins;  // [count][3]
    const float* dirs;     // [count][3]
    float4* radiance;      // [count] (ray_color.rgb, 1), or null
    uint4* hits;           // [count][2] vcrt_ray_hit: (t, sphere, segments, 0) (normal.xyz, 0),
                           //   or null
    uint32_t count;        // <= 2^30
    uint32_t* work;        // the next ray index to hand out, zeroed before the launch (it ends
                           //   below count + 64 * the grid's waves)
    unsigned long long* tallies;  // [3] segments, groups of four put through the exact test (per
                                  //   wave), boxes tested (per wave); zeroed before the launch
};

// Occlusion queries (vcrt_occlude_rays): does hit_sphere accept any sphere for a caller-supplied
// ray with min_t = kMinT and the ray's own max_t? The scene block is filled as RayQueryParams'
// is (the shading rows and max_depth are not read). No work counter: ray i belongs to wave
// (i / 64) mod the grid's waves.
struct OcclusionParams {
    TraceParams scene;
    const float* origins;  // [count][3]
    const float* dirs;     // [count][3]
    const float* tmax;     // [count] each ray's max_t, or null: kInfinity for every ray
    uint8_t* occluded;     // [count] 0 or 1
    uint32_t count;        // <= 2^30
    unsigned long long* tallies;  // [2] groups of four put through the exact test (per wave),
                                  //   boxes tested (per wave); zeroed before the launch
};

// Feature buffers (vcrt_draw_features): first-hit albedo, normal, depth, coverage and sphere id
// of the frame's own camera rays, averaged per pixel. The scene block is a TraceParams filled as
// a frame's is (scene_params, the camera lists prim_info / cam_rec, corner, cam, width, height,
// rank, world, tiles_x, local_tiles); its jitter and lens tables are the call's own, built for
// the sample indices first .. first + n - 1 and indexed from 0. One wave per local tile, one
// lane per slot; the outputs are indexed as the rank-local framebuffer is.
struct FeatureParams {
    TraceParams scene;
    float4* albedo;        // [elements] (sum a_i / n, sum c_i / n), or null
    float4* normal_depth;  // [elements] (sum n_i / n, sum t_i / n), or null
    int32_t* sphere;       // [elements] the sphere of the first sample index (-1: sky), or null
    uint32_t n;            // samples per pixel of the call, >= 1
    uint32_t use_lists;    // 0: every ray takes the query kernel's scans (VCRT_FEATURE_LISTS=0)
    unsigned long long* tallies;  // [kFeatureTallySlots][8]: per slot (64 B), [0] rays answered
                                  //   from the camera-ray lists, [1] groups of four put through
                                  //   the exact test (per wave), [2] boxes tested (per wave);
                                  //   zeroed before the launch, summed over the slots by the host
};
// A frame has one short wave per tile (130 000 at 4K), and atomics on one address serialise
// (measured 8 ns each: three shared counters cost 0.79 ms at 1080p, whatever the samples): block
// b adds to slot b % kFeatureTallySlots, each slot a cache line of its own.
constexpr uint32_t kFeatureTallySlots = 256;

// The ambient visibility buffer (vcrt_draw_occlusion): per sample of the frame's camera rays the
// first hit as the feature kernel finds it, then m any-hit rays from the hit point along normal +
// u_j, counted in integers. The scene block is filled as FeatureParams' is (the call's own jitter
// and lens tables, indexed from 0). One wave per local tile, one lane per slot.
struct OcclusionBufferParams {
    TraceParams scene;
    float4* visibility;    // [elements] (open share x 3, hit share)
    const float4* dirs;    // [n * m] u_j of j = first * m .. (first + n) * m - 1 (vcrt_ambient_dirs),
                           //   sample-major; read at wave-uniform indices
    uint32_t n;            // samples per pixel of the call, >= 1
    uint32_t m;            // secondary rays per hit sample, 1 .. 256; n * m <= 4096
    float reach;           // the secondary rays' max_t, not NaN
    uint32_t use_lists;    // as FeatureParams.use_lists
    unsigned long long* tallies;  // [kFeatureTallySlots][8]: per slot (64 B), [0] .. [2] as
                                  //   FeatureParams.tallies (the primary and the secondary scans
                                  //   together), [3] samples that hit, [4] secondary rays
                                  //   occluded; zeroed before the launch, summed by the host
};

// The reprojection map (vcrt_draw_motion): the first hit of each pixel's centre ray as the feature
// kernel finds it, carried to where the sphere was (prev) and projected through the previous
// camera (vcrt_math.h MotionCamera, computed once on the host). The scene block is filled as
// FeatureParams' is; the jitter and lens tables are not read (the centre ray has neither). One
// wave per local tile, one lane per slot.
struct MotionParams {
    TraceParams scene;
    float4* motion;        // [elements] (px, py, z', key), zeros when the point does not project;
                           //   or null
    float4* surface;       // [elements] (key, t or 0, 0, 0), or null
    const float* prev;     // the previous (centre.xyz, radius) of sphere s at prev + prev_stride s:
                           //   scene.center_radius (stride 4), the host call's packed table
                           //   (stride 4) or the caller's vcrt_sphere records (stride 10)
    uint32_t prev_stride;  // in floats
    uint32_t same_camera;  // 1: the previous camera is the current one (the identity rule applies)
    uint32_t use_lists;    // as FeatureParams.use_lists
    float prev_cam[16];    // C' (0..2), e (3..5), nw (6..8), nu (9..11), nv (12..14), num (15)
    unsigned long long* tallies;  // [kFeatureTallySlots][8]: per slot (64 B), [0] .. [2] as
                                  //   FeatureParams.tallies, [3] rays that hit, [4] pixels that
                                  //   projected (ok), [5] pixels served by the identity rule;
                                  //   zeroed before the launch, summed by the host
};

// Adaptive sampling (vcrt_draw_samples): per local pixel n_p = min(counts, max_count) further
// samples of the frame's own rays, in quanta of kSampleQuantum. Three kernels share the tables:
//   offsets [total_pixels]  the index of each local slot's first item (exclusive prefix of its
//                           quanta, 0 for slots outside the frame)
//   items   [items]         (local slot q, quantum k | samples of the quantum << 16)
//   scratch [items]         (S_k.rgb, samples of the quantum), written by the tracer
constexpr uint32_t kSampleQuantum = 4;       // vcrt_work_quantum's base
constexpr uint32_t kSampleMaxCount = 256;    // counts are clamped to max_count <= this
constexpr uint32_t kSampleScanBlock = 256;   // threads of vcrt_sample_scan
constexpr uint32_t kSampleScanSlots = 1024;  // local slots per block: four per thread
constexpr uint64_t kSampleMaxItems = uint64_t{1} << 28;

// vcrt_sample_scan, launched three times: phase 0, one block per kSampleScanSlots local slots,
// writes block_sums; phase 1, one block, turns block_sums' quanta into their exclusive prefix
// (modulo 2^32: the host refuses more than kSampleMaxItems before anything reads it) and writes
// the totals; phase 2, phase 0's grid, writes offsets and items.
struct SampleScanParams {
    const uint16_t* counts;  // [elements] the caller's plane, rank-local framebuffer layout
    uint4* block_sums;       // [blocks] (quanta, samples, pixels with n_p > 0, 0)
    unsigned long long* totals;  // [4] samples, pixels, items, 0
    uint32_t* offsets;       // [total_pixels]
    uint2* items;            // [items]; phase 2 only
    uint32_t phase, blocks;
    uint32_t max_count;
    uint32_t total_pixels;   // local_tiles * 64
    int32_t width, height, rank, world;
    uint32_t tiles_x;
};

// vcrt_trace_samples: a persistent grid over the items; a lane runs its item's paths one after
// another. The scene block is filled as FeatureParams' is, with the frame's max_depth and the
// call's jitter and lens tables of [first, first + max_count), indexed from 0.
struct SampleTraceParams {
    TraceParams scene;
    const uint2* items;
    float4* scratch;
    uint32_t count;        // items, <= kSampleMaxItems
    uint32_t use_lists;    // as FeatureParams.use_lists
    uint32_t* work;        // the next item to hand out, zeroed before the launch (it ends below
                           //   count + 64 * the grid's waves)
    unsigned long long* tallies;  // [kFeatureTallySlots][8]: per slot (64 B), [0] .. [2] as
                                  //   FeatureParams.tallies, [3] segments; zeroed before the launch
};

// vcrt_sample_resolve: one lane per local slot adds its S_k in ascending k and applies the
// accumulate rule (vcrt.h vcrt_draw_samples).
struct SampleResolveParams {
    const uint16_t* counts;
    const uint32_t* offsets;
    const float4* scratch;
    float4* sums;          // [elements]
    float4* mean;          // [elements], or null
    uint32_t max_count;
    uint32_t accumulate;
    uint32_t total_pixels;
    int32_t width, height, rank, world;
    uint32_t tiles_x;
};

// TraceParams.jitter from the host's jitter (vcrt_math.h rand2) and the camera: run at
// vcrt_begin and for each progressive frame.
struct SetupJitterParams {
    const float2* jitter_in;  // [nsamples] (jx, jy)
    float4* jitter;           // [nsamples] jx delta_u + jy delta_v
    uint32_t nsamples;
    float cam[12];  // as TraceParams.cam
    float4* corner;  // [slots] the local slots' pixel corners, or null
    uint32_t slots, tiles_x, rank, world;
};

// Exact sums -> pixels (vcrt_math.h resolve_channel), rgba32f with alpha 1.
struct ResolveParams {
    double* accum;                    // [local_tiles * 64][4]
    float4* out;                      // rank-local framebuffer
    double inv_scale;                 // 2^-s (the scale of TraceParams.flags bits 24..31)
    float spp_total;                  // samples per pixel accumulated so far (<= 2^19)
    int32_t width, height, rank, world;
    uint32_t tiles_x, local_tiles;
    uint32_t zero_accum;  // 1: write zeros back (the next frame sums from zero: no memset)
    const uint32_t* pixel_emax;  // non-null: each pixel's own scale (vcrt_math.h pixel_scale_log2)
    // the tracer's counters (TraceParams outlier_max, segments, work_done, work queues), or
    // null: block 0 copies their first four u64 to counters_out (host-pinned) and then zeroes
    // counter_words u32 of them, so the next frame needs neither a memset nor a read-back copy
    unsigned long long* counters;
    unsigned long long* counters_out;
    uint32_t counter_words;
};

struct AssembleParams {
    const float4* gathered;  // [world][tiles_per_rank][64] packed rank framebuffers
    float4* frame;           // [height][width]
    int32_t width, height, world;
    uint32_t tiles_x, tiles_per_rank;
};

// Linear rgba32f -> sRGB8 as the reference's B8G8R8A8_SRGB swapchain stores it (Frontend.cpp:43).
struct EncodeParams {
    const float4* in;
    uchar4* out;
    const float* thresholds;  // [255] ascending: byte = #{k : c >= thresholds[k]}
    uint32_t count;
};

struct SinCheckParams {
    unsigned long long* result;  // [2]: inputs where sin_fast != sin_canonical, fallbacks
    uint32_t* first_bad;         // smallest differing bit pattern (init 0xFFFFFFFF)
    uint32_t first, count;       // input bit patterns first .. first + count - 1
    double sin_c[13];            // vcrt_math.h kSinC, for the table form the tracer uses
};

struct UnitCheckParams {
    const float* in;  // [count][3]: the scatter's three rand() values
    float* out;       // [count][3]: tracer.hip unit_of of each triple
    uint32_t count;
};

struct FillParams {
    float4* out;
    uint32_t count;
    float4 value;
};

}  // namespace vcrt
