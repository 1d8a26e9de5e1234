// renderer_state.hpp -- the host library's one RendererState and the launch helpers on its
// stream, shared by the translation units behind the C ABI: capi.cpp (the renderer, the scene and
// the frame), ray_passes.cpp (the queries and the passes that trace the frame's own rays) and
// image_passes.cpp (the passes over caller-supplied planes). The state's device buffers, pinned
// buffers and events are owners (device_resources.hpp) that free themselves, so teardown is an
// assignment of a fresh state (vcrt_end) and there is no list of frees to maintain.
#pragma once

#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include "Shader.hpp"
#include "cluster.hpp"
#include "device_resources.hpp"
#include "hip_status.hpp"
#include "pass_staging.hpp"
#include "scene_update_abi.h"
#include "vcrt.h"
#include "vcrt_kernel_abi.h"
#include "vcrt_math.h"

namespace vcrt {

struct RendererState {
    bool begun = false;
    vcrt_render_desc desc{};
    int device = 0;
    int num_cus = 0;
    size_t max_lds = 0;
    hipStream_t stream = nullptr;
    Event ev_start, ev_stop, ev_resolve;
    VkPipelineShaderStageCreateInfo stage{};
    hipFunction_t k_trace_lds = nullptr, k_trace_smem = nullptr, k_assemble = nullptr,
                  k_fill = nullptr, k_trace_lds_stats = nullptr, k_trace_smem_stats = nullptr,
                  k_resolve = nullptr, k_encode = nullptr, k_trace_cull = nullptr,
                  k_trace_cull_stats = nullptr, k_trace_cull_lane_lds = nullptr,
                  k_trace_cull_lane_lds_stats = nullptr, k_trace_cull_lane = nullptr,
                  k_trace_cull_lane_stats = nullptr, k_trace_cull_lane_lds_wide = nullptr,
                  k_trace_cull_lane_lds_wide_stats = nullptr, k_trace_cull_flat = nullptr,
                  k_trace_cull_flat_stats = nullptr, k_trace_cull_flat_global = nullptr,
                  k_trace_cull_flat_global_stats = nullptr, k_trace_cull_flat_boxes = nullptr,
                  k_trace_cull_flat_boxes_stats = nullptr, k_setup_jitter = nullptr;
    // the flat scans' cost-order builds (null: the code object predates them; no cost order)
    hipFunction_t k_trace_cull_flat_cost = nullptr, k_trace_cull_flat_global_cost = nullptr,
                  k_trace_cull_flat_boxes_cost = nullptr;
    // ray queries (vcrt_trace_rays; null: the code object predates them). The counters (the work
    // index at 0, three u64 tallies from 8) are the query's own, so a frame's are left alone.
    hipFunction_t k_trace_rays = nullptr;
    // the thin-lens frame kernels (desc.lens_radius > 0; null: the code object predates them):
    // the SMEM scan, then the three flat scans and their cost-order builds
    hipFunction_t k_smem_lens = nullptr, k_flat_lens = nullptr, k_flat_lens_cost = nullptr,
                  k_flat_global_lens = nullptr, k_flat_global_lens_cost = nullptr,
                  k_flat_boxes_lens = nullptr, k_flat_boxes_lens_cost = nullptr;
    DeviceBuffer<unsigned long long> d_rq_counters;
    // occlusion queries (vcrt_occlude_rays; null: the code object predates them): tallies in
    // d_rq_counters
    hipFunction_t k_occlude_rays = nullptr;
    // feature buffers (vcrt_draw_features; null: the code object predates them): the jitter
    // terms and lens origins of the call's own sample indices (the frame's tables are left
    // alone) and the tallies' slots; kept and grown only
    hipFunction_t k_frame_features = nullptr;
    bool feature_lists = true;  // VCRT_FEATURE_LISTS=0: no ray takes the camera-ray lists
    DeviceBuffer<float2> d_ft_jitter_in;
    DeviceBuffer<float4> d_ft_jitter, d_ft_lens;
    std::vector<float2> h_ft_jitter;
    std::vector<float4> h_ft_lens;
    DeviceBuffer<unsigned long long> d_ft_counters;
    // the ambient visibility buffer (vcrt_draw_occlusion; null: the code object predates it): the
    // u_j table of the call, kept and grown only; the jitter and lens tables and the tallies'
    // slots are the feature buffers'
    hipFunction_t k_frame_occlusion = nullptr;
    DeviceBuffer<float4> d_ao_dirs;
    std::vector<float4> h_ao_dirs;
    // the reprojection map (vcrt_draw_motion; null: the code object predates it): the host call's
    // packed table of the previous centres and radii, kept and grown only; the tallies' slots are
    // the feature buffers'
    hipFunction_t k_frame_motion = nullptr;
    DeviceBuffer<float4> d_mo_prev;
    std::vector<float4> h_mo_prev;
    // The one staging storage of the host forms (pass_staging.hpp; ray_passes.cpp and
    // image_passes.cpp), kept and grown only: a call takes its planes of 16-byte multiples from
    // staging.wide and its narrower ones from staging.narrow in the order it lists them, so
    // within a call no two planes share a buffer and nothing outlives the call. The widest calls:
    // vcrt_reproject_moments takes eight wide planes (six float4 planes in, two out) and two
    // lengths; vcrt_occlude_rays takes four narrow ones (origins, directions, reaches, answers).
    StagingPool staging;
    // the image passes (image_passes.cpp; a null kernel: the code object predates the pass)
    // the denoiser (vcrt_denoise): the two scratch planes the passes between the first and the
    // last go through and the events around the passes
    hipFunction_t k_denoise_pass = nullptr, k_denoise_pass_lds = nullptr;
    DeviceBuffer<float4> d_dn_scratch[2];
    Event ev_dn[9];
    // temporal accumulation (vcrt_reproject) and its tally slots
    hipFunction_t k_reproject_pass = nullptr;
    DeviceBuffer<unsigned long long> d_rp_counters;
    // variance-guided denoising (vcrt_reproject_moments, vcrt_variance, vcrt_denoise_variance;
    // each pair both or neither) and the variance pass's tally slots; the steered filter's
    // scratch planes and events are the denoiser's
    hipFunction_t k_reproject_moments_pass = nullptr, k_variance_pass = nullptr,
                  k_variance_pass_lds = nullptr, k_denoise_var_pass = nullptr,
                  k_denoise_var_pass_lds = nullptr;
    DeviceBuffer<unsigned long long> d_vr_counters;
    // adaptive sampling (vcrt_draw_samples, vcrt_sample_counts; null: the code object predates
    // them): the scan's block sums, offsets and item table, the tracer's scratch (16 B per
    // item), the counters (totals, work index, tally slots) and the events around the three
    // kernels; kept and grown only. The jitter and lens tables are the feature buffers'.
    hipFunction_t k_sample_scan = nullptr, k_trace_samples = nullptr, k_sample_resolve = nullptr,
                  k_sample_counts_pass = nullptr;
    DeviceBuffer<uint4> d_sm_block_sums;
    DeviceBuffer<uint32_t> d_sm_offsets;
    DeviceBuffer<uint2> d_sm_items;
    DeviceBuffer<float4> d_sm_scratch;
    DeviceBuffer<unsigned long long> d_sm_counters;
    Event ev_sm[5];
    // VCRT_CULL_LANE_TABLES: 0 = auto, 1 = LDS, 2 = global, 3 = boxes in LDS (flat scan)
    int cull_lane_tables = 0;
    bool accum_ring = true;      // VCRT_ACCUM_RING=0: chunk sums straight to global memory
    bool stage_tables = true;    // VCRT_STAGE_TABLES=0: the SMEM scan reads its tables globally
    uint32_t ring_max = kRingMaxEntries;
    int max_blocks_per_cu = 0;  // VCRT_MAX_BLOCKS_PER_CU: caps the occupancy rule (0: none)
    // the cost-ordered schedule ("cost order" in vcrt_draw_next_frame): -1 auto, 0 off, 1 on
    // (VCRT_WORK_ORDER=cost / static); the first frame of a configuration measures each pixel's
    // segments, later frames hand out the blocks most expensive first
    int cost_order = -1;
    bool cost_partition = false;  // the partition is the cost partition (default_chunk)
    DeviceBuffer<uint32_t> d_pixel_cost;   // [total_pixels] segments (TraceParams.pixel_cost)
    DeviceBuffer<uint32_t> d_block_order;  // [blocks] TraceParams.block_order
    uint64_t order_key = 0;  // the configuration the order was measured for (0: none)
    uint32_t nch_magic[2] = {0u, 0u};  // TraceParams.nch_magic of the partition
    // deferred fetches (TraceParams.fetch_min / fetch_wait; VCRT_FETCH_MIN, VCRT_FETCH_WAIT;
    // fetch_min 0: the rule in trace_frame)
    uint32_t fetch_min = 0u, fetch_wait = 0u;
    int flat_block = 0;  // VCRT_FLAT_BLOCK: threads per group of the LDS flat scan (0: 256)
    uint32_t lds_per_cu = 0;     // LDS bytes per CU (160 KB on gfx950)
    // diagnostics (environment: VCRT_DEBUG_STATS=1, VCRT_WORK_ORDER=forward)
    int debug_stats = 0;  // 1: the stats kernels; 2: the product kernels with a debug buffer
                          //    (builds with VCRT_WAVE_END_TIMES record wave start/end times)
    uint32_t work_flags = 0;
    DeviceBuffer<unsigned long long> d_debug;  // vcrt_stats.debug's image
    DeviceBuffer<uint32_t> d_region;  // stats kernels: [waves][kRegionCount] region entry counts
    // scene
    int32_t nspheres = 0;
    bool scene_bounded = false;  // every |center|, radius <= 2^30: discriminants stay finite
    bool radii_safe = false;     // every |radius| in [2^-40, 2^30] (kFlagRadiiSafe)
    int32_t accum_log2 = kAccumMaxScaleLog2;  // the scale s pixels start at (flags)
    DeviceBuffer<float4> d_geom;  // pair-SoA groups of four (+1 padding group)
    DeviceBuffer<float4> d_center_radius, d_shade;
    DeviceBuffer<float4> d_material;  // (material id, 1 / param, Schlick r0^2, 0) per sphere
    // culled-scan tables (cluster.hpp); ncgroups == 0 when culling does not apply
    int32_t ncgroups = 0, ncbig = 0;
    float cmargin[4] = {0, 0, 0, 0};  // box margin constants (CullTables::margin)
    bool cslab_on = false;            // the shared y slab (CullTables::slab, slab_lohi)
    float cslab[2] = {0, 0};
    DeviceBuffer<float4> d_cgroup, d_cbound, d_cbound_nf, d_cnode;
    DeviceBuffer<float4> d_cnode_nf;  // node-pair boxes, near/far layout, padded to whole chunks
    DeviceBuffer<float4> d_ctop;
    // the footprint tables of the LDS-table flat scan (CullTables::fp_*), packed to their width
    DeviceBuffer<uint32_t> d_fp_tab;
    float cfp_x[2] = {1, 0}, cfp_z[2] = {1, 0}, cfp_y[2] = {0, 0}, cfp_k2 = 0;
    uint32_t cfp_always = 0xffffffffu;
    // the group-level footprint tables (CullTables::gf_*) and whether a frame may use them
    DeviceBuffer<uint4> d_gf_tab;
    float cgf_x[2] = {1, 0}, cgf_z[2] = {1, 0}, cgf_k2 = 0;
    uint32_t cgf_n = 0, cgf_always[4] = {0, 0, 0, 0};
    bool cgf_ok = false;
    // camera-ray tile lists (primary.cpp), flat scan only; vcrt_set_camera reuses the buffers
    // and grows them only
    DeviceBuffer<uint32_t> d_prim_info;
    DeviceBuffer<uint16_t> d_prim_ids;
    DeviceBuffer<float> d_cam_rec;  // camera-relative records: big groups, sphere lists
    bool primary_lists = true;      // VCRT_PRIMARY_LISTS=0 turns them off
    size_t prim_nids = 0, prim_npairs = 0;  // the installed lists' sizes: ids, pair records
    // the scene as vcrt_set_scene got it and its culling tables: vcrt_set_camera's host builders
    // (VCRT_CAMERA_LISTS=host, or a code object without the list kernels) and sizes
    std::vector<vcrt_sphere> h_spheres;
    CullTables h_ct;
    // the camera-list kernels (camera_lists.hip; null: the code object predates them) and their
    // scratch: grown boxes and sphere entries, counts + offsets + totals; kept and grown only
    hipFunction_t k_cl_prepare = nullptr, k_cl_count = nullptr, k_cl_scan = nullptr,
                  k_cl_fill = nullptr;
    DeviceBuffer<double> d_cl_boxes, d_cl_spheres;
    DeviceBuffer<uint32_t> d_cl_counts;
    PinnedBuffer<uint32_t> h_cl_totals;  // [2]
    Event ev_cl[2];
    vcrt_camera_stats cam_stats{};
    // vcrt_update_spheres: the refit kernels (scene_update.hip; null: the code object predates
    // them), the staged spheres, the summary and its pinned copy; kept and grown only
    hipFunction_t k_su_rows = nullptr, k_su_groups = nullptr, k_su_levels = nullptr,
                  k_su_footprint = nullptr;
    DeviceBuffer<float> d_su_spheres;
    DeviceBuffer<SceneSummary> d_su_summary;
    PinnedBuffer<SceneSummary> h_su_summary;
    Event ev_su[2];
    vcrt_scene_update_stats su_stats{};
    // h_ct holds the grouping but not yet the tables of h_spheres: the device refit leaves them
    // on the device, and current_tables() restates them when the host needs them
    bool h_ct_stale = false;
    // work decomposition
    int32_t quantum = 1;  // the accumulation quantum G (a power of two)
    int32_t chunk = 1, nchunks = 1;
    int32_t tail_start = 0, tail_chunk = 1, tail_nchunks = 0;  // TraceParams' tail
    uint32_t total_pixels = 0, total_items = 0;
    bool direct = false;  // one item per pixel, not progressive: lanes write pixels (kFlagDirect)
    DeviceBuffer<double> d_accum;  // [total_pixels][4] exact sums of the quantized chunk sums
    // d_accum holds zeros: a memset, or the last resolve wrote them back (vcrt_resolve
    // zero_accum), so a non-progressive frame needs no memset of its own
    bool accum_clean = false;
    // Outlier quanta (vcrt_math.h "Accumulation"): [total_pixels] the float bits of each pixel's
    // largest |quantum sum| that passed 2^12 (0: none); once one has, every frame of the
    // configuration quantizes each pixel at its own scale (pixel_scale, kFlagPixelScale)
    DeviceBuffer<uint32_t> d_pixel_emax;
    bool pixel_scale = false;
    int32_t min_scale = kAccumMaxScaleLog2;  // the smallest pixel scale so far
    uint64_t accumulated = 0;               // samples per pixel accumulated (progressive)
    // the host's jitter (jx, jy) of a frame's sample indices: two pinned buffers used in turn,
    // each reused only once the copy recorded by its event is done (progressive frames set up
    // their jitter without waiting for the stream)
    PinnedBuffer<float2> h_jitter[2];
    // the lens origins of the same sample indices (desc.lens_radius > 0, else null), built on
    // the host (vcrt_math.h lens_offset) in the same two turns and under the same events
    PinnedBuffer<float4> h_lens[2];
    DeviceBuffer<float4> d_lens;  // TraceParams.lens
    Event ev_jitter[2];
    int jitter_slot = 0;
    DeviceBuffer<float> d_srgb_thresholds;
    DeviceBuffer<uchar4> d_srgb;  // vcrt_read_framebuffer_srgb8's staging, kept and grown only
    // per-frame inputs / outputs
    DeviceBuffer<float2> d_jitter_in;  // the host's jitter (jx, jy) of the frame's sample indices
    DeviceBuffer<float4> d_jitter;     // TraceParams.jitter (vcrt_setup_jitter)
    DeviceBuffer<float4> d_corner;     // TraceParams.corner (vcrt_setup_jitter, at vcrt_begin)
    DeviceBuffer<float4> d_fb_own;
    float4* d_fb = nullptr;  // current render target (own, the gather's or caller-provided)
    size_t fb_bytes = 0;
    DeviceBuffer<unsigned long long> d_counters;  // kCounterBytes
    // the counters' first four u64 (outlier max, segments, work tallies), read back each frame:
    // host-pinned, written by vcrt_resolve (which then zeroes d_counters: counters_clean) or
    // copied when no resolve runs
    PinnedBuffer<unsigned long long> h_counters;
    bool counters_clean = false;
    uint32_t tiles_x = 0, local_tiles = 0;
    uint32_t local_elems = 0;   // float4 elements of the rank-local framebuffer
    uint64_t local_pixels = 0;  // frame pixels this rank renders
    uint32_t pad_tiles = 0;     // tiles of the largest rank: the packed framebuffers' size
    // multi-GPU, one process per GPU (vcrt_comm_init): the ranks' packed framebuffers go to
    // rank 0 in one grouped RCCL send/recv inside vcrt_draw_next_frame; rank 0 assembles them
    ncclComm_t comm = nullptr;  // non-blocking (comm_wait.hpp): every wait has a deadline
    bool comm_lost = false;     // the communicator failed or timed out and was aborted: every
                                // later draw returns VK_ERROR_DEVICE_LOST (until vcrt_begin)
    DeviceBuffer<float4> d_gather;  // rank 0: [world][pad_tiles][64], its own tiles in slot 0
    DeviceBuffer<float4> d_frame;   // rank 0: the assembled frame [height][width]
    Event ev_gather_start, ev_gather;
    Camera cam{};
    vcrt_stats stats{};
};

// The state lives on the heap and is never deleted: a file-static RendererState would run its
// members' destructors at process exit, and a process that ends without vcrt_end would then call
// hipFree and hipEventDestroy from a static destructor, possibly after the HIP runtime has torn
// itself down. As it is, such a process makes no HIP call at exit; the resources are released in
// vcrt_end alone, by move-assigning a fresh state. Defined once, in capi.cpp.
extern RendererState& g;

template <typename Params>
VkResult launch(hipFunction_t f, uint32_t grid, uint32_t block, uint32_t lds, Params& params) {
    void* args[] = {&params};
    VCRT_TRY(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, lds, g.stream, args, nullptr));
    return VK_SUCCESS;
}

// One timed launch of a query, guide or image-pass kernel with tallies of its own, waited for:
// `counters` (words u64, allocated on first use) is zeroed and handed to `bind`, which points the
// params at it; the launch runs between ev_start and ev_stop. With a host destination the
// counters come back into it and *ms is the kernel time; without one neither is read.
template <typename Params, typename Bind>
VkResult timed_launch(hipFunction_t f, uint32_t grid, uint32_t block, uint32_t lds, Params& params,
                      DeviceBuffer<unsigned long long>& counters, size_t words, Bind&& bind,
                      unsigned long long* host, float* ms) {
    const size_t bytes = words * sizeof(unsigned long long);
    VCRT_TRY(counters.reserve(words));
    bind(counters.data());
    VCRT_TRY(hipMemsetAsync(counters.data(), 0, bytes, g.stream));
    VCRT_TRY(hipEventRecord(g.ev_start.get(), g.stream));
    const VkResult r = launch(f, grid, block, lds, params);
    if (r != VK_SUCCESS) return r;
    VCRT_TRY(hipEventRecord(g.ev_stop.get(), g.stream));
    if (host)
        VCRT_TRY(hipMemcpyAsync(host, counters.data(), bytes, hipMemcpyDeviceToHost, g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    if (host) VCRT_TRY(hipEventElapsedTime(ms, g.ev_start.get(), g.ev_stop.get()));
    return VK_SUCCESS;
}

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Whether any of the planes' addresses has a bit of `mask` set (the kernels' 16-byte loads and
// stores of float4 planes: 15; 4-byte ones: 3; 2-byte ones: 1). A null plane is aligned.
inline bool misaligned(std::initializer_list<const void*> planes, uintptr_t mask) {
    uintptr_t bits = 0;
    for (const void* p : planes) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & mask) != 0;
}

inline float* plane_of(const DeviceBuffer<float4>& b) { return reinterpret_cast<float*>(b.data()); }

// The stats preamble of a pass: the struct zeroed, the kernel named.
template <typename Stats>
void name_stats(Stats* stats, const char* kernel) {
    if (!stats) return;
    *stats = Stats{};
    std::snprintf(stats->kernel, sizeof(stats->kernel), "%s", kernel);
}

// ---- what capi.cpp defines for the frame and ray_passes.cpp uses too ---------------------------

bool lens_on();  // desc.lens_radius > 0
// Jitter of sample indices base .. base+n-1 (shader.comp:48 depends only on the index).
void make_jitter(uint64_t base, int n, float2* out);
// pixel00, delta_u, delta_v, centre: TraceParams.cam
std::array<float, 12> camera_array();
// Whether a frame of camera `cam` (camera_array) gets the camera-ray lists (the range guard).
bool lists_allowed(const std::array<float, 12>& cam);
// The camera of a width x height frame as vcrt_begin builds it.
Camera camera_of(int32_t width, int32_t height, const vcrt_camera& c);
// The scene's part of a kernel's argument block: the scan tables, the shading rows, the margins
// and the flags' scene bits (frames and ray queries).
void scene_params(TraceParams& p);
// The scene's and the frame's part of the argument block of a kernel that traces the frame's own
// camera rays: scene_params, the jitter and lens tables given (of `spp` samples), the corners,
// the camera-ray lists (null when the camera fails lists_allowed), size, rank, tiles and camera.
void frame_params(TraceParams& p, const float4* jitter, const float4* lens, int32_t spp,
                  int32_t max_depth);
// The jitter terms (and, with d_lens, the lens origins: centre + lens_offset) of sample indices
// base .. base + n - 1 into tables the caller owns: built on the host in h_jitter (and h_lens),
// copied to d_jitter_in (and d_lens), `copied` (may be null) recorded behind the copies, then
// vcrt_setup_jitter's launch into d_jitter (and, when d_corner is given, the pixels' corners).
struct JitterTables {
    float2* h_jitter;
    float4* h_lens;
    float2* d_jitter_in;
    float4 *d_jitter, *d_lens, *d_corner;
    hipEvent_t copied;
};
VkResult jitter_tables(uint64_t base, uint32_t n, const JitterTables& t);

// FeatureParams.tallies and its like: slots of 64 B, summed by the callers (sum_tallies)
constexpr size_t kFeatureCounterWords = 8 * kFeatureTallySlots;  // u64

// The timed launch of a kernel that traces the frame's own camera rays (vcrt_draw_features,
// vcrt_draw_occlusion, vcrt_draw_motion): one wave per local tile, its tallies' slots in
// d_ft_counters. A rank without tiles launches nothing, and *ms stays 0.
template <typename Params>
VkResult frame_ray_launch(hipFunction_t f, Params& p, unsigned long long* slots, float* ms) {
    if (g.local_tiles == 0) {
        VCRT_TRY(hipStreamSynchronize(g.stream));
        return VK_SUCCESS;
    }
    return timed_launch(f, (g.local_tiles + 3u) / 4u, 256, 0, p, g.d_ft_counters,
                        kFeatureCounterWords, [&p](unsigned long long* c) { p.tallies = c; },
                        slots, ms);
}

}  // namespace vcrt
