// ray_passes.cpp -- the host side of the passes that trace rays against the renderer's scene: the
// queries over caller-supplied rays (vcrt_trace_rays, vcrt_occlude_rays) and the passes over the
// frame's own camera rays (vcrt_draw_features, vcrt_draw_occlusion, vcrt_draw_motion,
// vcrt_draw_samples). One body per pass behind both exported forms, the host form staging its
// planes through the pool the image passes use (pass_staging.hpp). The order in which a pass
// checks its arguments is its own, pinned by the refused-call tests: the queries look at the
// renderer first, the frame passes at the arguments' own faults first, so that they read the same
// with and without a renderer; the device forms then check alignment, the host forms do not.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "renderer_state.hpp"

namespace {

using vcrt::frame_params;
using vcrt::frame_ray_launch;
using vcrt::g;
using vcrt::kFeatureCounterWords;
using vcrt::launch;
using vcrt::lens_on;
using vcrt::misaligned;
using vcrt::name_stats;
using vcrt::out4;
using vcrt::pass_ready;
using vcrt::Plane;
using vcrt::Staging;
using vcrt::timed_launch;
using Clock = std::chrono::steady_clock;

constexpr uint32_t kRayQueryMax = 1u << 30;
constexpr size_t kRayCounterWords = 4;  // u64: the u32 work index in [0], tallies in [1..3]
constexpr uint64_t kFeatureMaxIndex = uint64_t{1} << 19;  // vcrt_lens_offsets' index bound
constexpr uint64_t kAmbientMaxRays = 4096;                // n * m of one call
constexpr uint64_t kAmbientMaxIndex = uint64_t{1} << 22;  // j + 0.5f is exact below 2^23
constexpr int64_t kMotionMaxSpheres = (int64_t{1} << 24) - 2;  // key = (float)(s + 2) stays exact

// The grid of a persistent launch over `count` rays or items: the blocks of kQueryBlock threads
// the occupancy query admits per CU (at most `cap` of them, when given), on every CU, capped at
// the blocks the batch fills.
constexpr uint32_t kQueryBlock = 256;
uint32_t query_grid(hipFunction_t f, uint32_t count, int cap = 0) {
    int per_cu = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, kQueryBlock, 0) !=
            hipSuccess ||
        per_cu <= 0)
        per_cu = 1;
    if (cap > 0) per_cu = std::min(per_cu, cap);
    return std::min<uint32_t>(static_cast<uint32_t>(per_cu) * static_cast<uint32_t>(g.num_cus),
                              (count + kQueryBlock - 1) / kQueryBlock);
}

// The first k words of every 64-byte tally slot, summed into out[0 .. k).
void sum_tallies(const unsigned long long* slots, size_t words, int k, unsigned long long* out) {
    for (size_t s = 0; s < words; s += 8)
        for (int c = 0; c < k; c++) out[c] += slots[s + c];
}

// ---- the queries over caller-supplied rays -----------------------------------------------------

// Both take a persistent grid sized as a frame's is and return when the kernel is done. A batch
// of no rays launches nothing: the stats come back zeroed and named.

vcrt_result trace_rays(bool host, const float* origins, const float* dirs, uint32_t count,
                       int32_t max_depth, float* radiance, vcrt_ray_hit* hits,
                       vcrt_ray_stats* stats) {
    static_assert(sizeof(vcrt_ray_hit) == 32, "two 16-byte stores per record");
    // the arguments, in the order of the header's table
    if (!g.begun || !g.stage.module) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (count > 0 && (!origins || !dirs)) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (!radiance && !hits) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (max_depth < 0 || count > kRayQueryMax) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!g.k_trace_rays) return VCRT_ERROR_FEATURE_NOT_PRESENT;
    // the kernel's 16-byte stores
    if (!host && misaligned({radiance, hits}, 15u)) return VCRT_ERROR_INITIALIZATION_FAILED;
    // (the larger optional plane first: whichever planes a call leaves out, the pool holds no
    // more than a buffer of each plane's own would)
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, count, {Plane{origins, 12, false}, Plane{dirs, 12, false},
                                       Plane{hits, 32, true}, Plane{radiance, 16, true}});
    if (r != VK_SUCCESS) return r;
    name_stats(stats, "vcrt_trace_rays");
    if (count == 0) return VCRT_SUCCESS;
    vcrt::RayQueryParams p{};
    vcrt::scene_params(p.scene);
    p.scene.max_depth = max_depth;
    p.origins = s.at(0);
    p.dirs = s.at(1);
    p.hits = s.at<uint4>(2);
    p.radiance = s.at<float4>(3);
    p.count = count;
    unsigned long long counters[kRayCounterWords] = {};
    float ms = 0.f;
    r = timed_launch(
        g.k_trace_rays, query_grid(g.k_trace_rays, count), kQueryBlock, 0, p, g.d_rq_counters,
        kRayCounterWords,
        [&p](unsigned long long* c) {
            p.work = reinterpret_cast<uint32_t*>(c);
            p.tallies = c + 1;
        },
        stats ? counters : nullptr, &ms);
    if (r != VK_SUCCESS) return r;
    if (stats) {
        stats->kernel_ms = ms;
        stats->segments = counters[1];
        stats->group_tests = counters[2];
        stats->bound_tests = counters[3];
    }
    return s.end();
}

// Every ray is one scan.
vcrt_result occlude_rays(bool host, const float* origins, const float* dirs, const float* tmax,
                         uint32_t count, uint8_t* occluded, vcrt_ray_stats* stats) {
    if (!g.begun || !g.stage.module) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (count > 0 && (!origins || !dirs || !occluded)) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (count > kRayQueryMax) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!g.k_occlude_rays) return VCRT_ERROR_FEATURE_NOT_PRESENT;
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, count, {Plane{origins, 12, false}, Plane{dirs, 12, false},
                                       vcrt::in1(tmax), Plane{occluded, 1, true}});
    if (r != VK_SUCCESS) return r;
    name_stats(stats, "vcrt_occlude_rays");
    if (count == 0) return VCRT_SUCCESS;
    vcrt::OcclusionParams p{};
    vcrt::scene_params(p.scene);
    p.origins = s.at(0);
    p.dirs = s.at(1);
    p.tmax = s.at(2);
    p.occluded = s.at<uint8_t>(3);
    p.count = count;
    unsigned long long counters[kRayCounterWords] = {};
    float ms = 0.f;
    r = timed_launch(
        g.k_occlude_rays, query_grid(g.k_occlude_rays, count), kQueryBlock, 0, p, g.d_rq_counters,
        kRayCounterWords, [&p](unsigned long long* c) { p.tallies = c + 1; },
        stats ? counters : nullptr, &ms);
    if (r != VK_SUCCESS) return r;
    if (stats) {
        stats->kernel_ms = ms;
        stats->segments = count;  // one scan per ray
        stats->group_tests = counters[1];
        stats->bound_tests = counters[2];
    }
    return s.end();
}

// ---- the passes over the frame's own camera rays -----------------------------------------------

// Their planes have the rank-local framebuffer's g.local_elems elements. With packed tiles (a
// world size above 1) the slots outside the frame keep what the caller's planes hold, so the host
// forms upload their outputs first.
bool packed_tiles() { return g.desc.world_size > 1; }

// The jitter terms (vcrt_setup_jitter, the frame's kernel) and, for a lens renderer, the lens
// origins of sample indices first .. first + n - 1 in the call's own tables (the frame's are left
// alone), and the scene block of a kernel that traces those samples of the frame's camera rays.
VkResult feature_tables(uint32_t first, uint32_t n, int32_t max_depth, vcrt::TraceParams& scene) {
    VCRT_TRY(g.d_ft_jitter_in.reserve(n));
    VCRT_TRY(g.d_ft_jitter.reserve(n));
    g.h_ft_jitter.resize(n);
    if (lens_on()) {
        VCRT_TRY(g.d_ft_lens.reserve(n));
        g.h_ft_lens.resize(n);
    }
    float4* const lens = lens_on() ? g.d_ft_lens.data() : nullptr;
    frame_params(scene, g.d_ft_jitter.data(), lens, static_cast<int32_t>(n), max_depth);
    return vcrt::jitter_tables(first, n,
                               {g.h_ft_jitter.data(), g.h_ft_lens.data(), g.d_ft_jitter_in.data(),
                                g.d_ft_jitter.data(), lens, nullptr, nullptr});
}

vcrt_result draw_features(bool host, uint32_t first, uint32_t n, float* albedo,
                          float* normal_depth, int32_t* sphere, vcrt_feature_stats* stats) {
    const auto t0 = Clock::now();
    // the arguments' own faults first, so that they read the same with and without a renderer
    if (!albedo && !normal_depth && !sphere) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (n == 0 || static_cast<uint64_t>(first) + n > kFeatureMaxIndex)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    // the kernel's 16-byte stores (and the ids' 4-byte ones)
    const vcrt_result c = pass_ready(
        !host && (misaligned({albedo, normal_depth}, 15u) || misaligned({sphere}, 3u)),
        g.begun && g.stage.module, g.k_frame_features);
    if (c != VCRT_SUCCESS) return c;
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, g.local_elems,
                         {out4(albedo, packed_tiles()), out4(normal_depth, packed_tiles()),
                          Plane{sphere, 4, true, packed_tiles()}});
    if (r != VK_SUCCESS) return r;
    name_stats(stats, "vcrt_frame_features");
    vcrt::FeatureParams p{};
    r = feature_tables(first, n, 1, p.scene);
    if (r != VK_SUCCESS) return r;
    p.albedo = s.at<float4>(0);
    p.normal_depth = s.at<float4>(1);
    p.sphere = s.at<int32_t>(2);
    p.n = n;
    p.use_lists = g.feature_lists ? 1u : 0u;
    unsigned long long slots[kFeatureCounterWords] = {};
    float ms = 0.f;
    r = frame_ray_launch(g.k_frame_features, p, stats ? slots : nullptr, &ms);
    if (r == VK_SUCCESS && stats) {
        unsigned long long counters[3] = {};
        sum_tallies(slots, kFeatureCounterWords, 3, counters);
        stats->kernel_ms = ms;
        stats->rays = g.local_pixels * n;
        stats->listed_rays = counters[0];
        stats->group_tests = counters[1];
        stats->bound_tests = counters[2];
    }
    return finish(r, s, stats, t0);
}

vcrt_result draw_occlusion(bool host, uint32_t first, uint32_t n, uint32_t m, float reach,
                           float* visibility, vcrt_occlusion_buffer_stats* stats) {
    const auto t0 = Clock::now();
    // the ranges first, so that they read the same with and without a renderer
    const uint64_t end = static_cast<uint64_t>(first) + n;
    if (n == 0 || m == 0 || m > 256 || end > kFeatureMaxIndex ||
        static_cast<uint64_t>(n) * m > kAmbientMaxRays || end * m > kAmbientMaxIndex)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!visibility || std::isnan(reach)) return VCRT_ERROR_INITIALIZATION_FAILED;
    // the kernel's 16-byte stores
    const vcrt_result c = pass_ready(!host && misaligned({visibility}, 15u),
                                     g.begun && g.stage.module, g.k_frame_occlusion);
    if (c != VCRT_SUCCESS) return c;
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, g.local_elems, {out4(visibility, packed_tiles())});
    if (r != VK_SUCCESS) return r;
    name_stats(stats, "vcrt_frame_occlusion");
    vcrt::OcclusionBufferParams p{};
    r = feature_tables(first, n, 1, p.scene);
    if (r != VK_SUCCESS) return r;
    // u_j of j = first m .. (first + n) m - 1, sample-major (vcrt_ambient_dirs' values)
    const uint32_t ndirs = n * m;
    VCRT_TRY(g.d_ao_dirs.reserve(ndirs));
    g.h_ao_dirs.resize(ndirs);
    for (uint32_t k = 0; k < ndirs; k++) {
        const vcrt::f3 u = vcrt::ambient_dir(first * m + k);
        g.h_ao_dirs[k] = make_float4(u.x, u.y, u.z, 0.0f);
    }
    VCRT_TRY(hipMemcpyAsync(g.d_ao_dirs.data(), g.h_ao_dirs.data(), sizeof(float4) * ndirs,
                            hipMemcpyHostToDevice, g.stream));
    p.visibility = s.at<float4>(0);
    p.dirs = g.d_ao_dirs.data();
    p.n = n;
    p.m = m;
    p.reach = reach;
    p.use_lists = g.feature_lists ? 1u : 0u;
    unsigned long long slots[kFeatureCounterWords] = {};
    float ms = 0.f;
    r = frame_ray_launch(g.k_frame_occlusion, p, stats ? slots : nullptr, &ms);
    if (r == VK_SUCCESS && stats) {
        unsigned long long counters[5] = {};
        sum_tallies(slots, kFeatureCounterWords, 5, counters);
        stats->kernel_ms = ms;
        stats->rays = g.local_pixels * n;
        stats->hit_rays = counters[3];
        stats->secondary_rays = counters[3] * m;
        stats->occluded = counters[4];
        stats->listed_rays = counters[0];
        stats->group_tests = counters[1];
        stats->bound_tests = counters[2];
    }
    return finish(r, s, stats, t0);
}

// prev_spheres: null (the current values); the device form reads the caller's records where they
// lie, the host form packs their centres and radii into d_mo_prev.
vcrt_result draw_motion(bool host, const vcrt_camera* prev_camera, const vcrt_sphere* prev_spheres,
                        int32_t count, float* motion, float* surface, vcrt_motion_stats* stats) {
    static_assert(sizeof(vcrt_sphere) == 40 && offsetof(vcrt_sphere, radius) == 12,
                  "the kernel reads centre and radius at the head of a 10-float record");
    const auto t0 = Clock::now();
    if (!motion && !surface) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (!g.begun || !g.stage.module) return VCRT_ERROR_INITIALIZATION_FAILED;
    if ((prev_spheres && count != g.nspheres) || g.nspheres >= kMotionMaxSpheres)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    // the kernel's 16-byte stores and its 4-byte loads of the records
    const vcrt_result c = pass_ready(
        !host && (misaligned({motion, surface}, 15u) || misaligned({prev_spheres}, 3u)), true,
        g.k_frame_motion);
    if (c != VCRT_SUCCESS) return c;
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, g.local_elems,
                         {out4(motion, packed_tiles()), out4(surface, packed_tiles())});
    if (r != VK_SUCCESS) return r;
    const float* prev = host ? nullptr : reinterpret_cast<const float*>(prev_spheres);
    if (host && prev_spheres && count > 0) {
        VCRT_TRY(g.d_mo_prev.reserve(static_cast<size_t>(count)));
        g.h_mo_prev.resize(static_cast<size_t>(count));
        for (int32_t i = 0; i < count; i++)
            g.h_mo_prev[i] = make_float4(prev_spheres[i].center[0], prev_spheres[i].center[1],
                                         prev_spheres[i].center[2], prev_spheres[i].radius);
        VCRT_TRY(hipMemcpyAsync(g.d_mo_prev.data(), g.h_mo_prev.data(), sizeof(float4) * count,
                                hipMemcpyHostToDevice, g.stream));
        prev = reinterpret_cast<const float*>(g.d_mo_prev.data());
    }
    name_stats(stats, "vcrt_frame_motion");
    vcrt::MotionParams p{};
    // the centre ray has no jitter and no lens offset
    frame_params(p.scene, nullptr, nullptr, 1, 1);
    p.motion = s.at<float4>(0);
    p.surface = s.at<float4>(1);
    p.prev = prev ? prev : reinterpret_cast<const float*>(g.d_center_radius.data());
    p.prev_stride = !prev || host ? 4u : 10u;
    p.same_camera =
        !prev_camera || std::memcmp(prev_camera, &g.desc.camera, sizeof(vcrt_camera)) == 0;
    // (a lens renderer has no lists: its rays do not share an origin)
    p.use_lists = g.feature_lists && !lens_on() ? 1u : 0u;
    const vcrt::MotionCamera mc = vcrt::motion_camera(
        p.same_camera ? g.cam : vcrt::camera_of(g.desc.width, g.desc.height, *prev_camera));
    const vcrt::f3 v[5] = {mc.center, mc.e, mc.nw, mc.nu, mc.nv};
    for (int i = 0; i < 5; i++) {
        p.prev_cam[3 * i + 0] = v[i].x;
        p.prev_cam[3 * i + 1] = v[i].y;
        p.prev_cam[3 * i + 2] = v[i].z;
    }
    p.prev_cam[15] = mc.num;
    unsigned long long slots[kFeatureCounterWords] = {};
    float ms = 0.f;
    r = frame_ray_launch(g.k_frame_motion, p, stats ? slots : nullptr, &ms);
    if (r == VK_SUCCESS && stats) {
        unsigned long long counters[6] = {};
        sum_tallies(slots, kFeatureCounterWords, 6, counters);
        stats->kernel_ms = ms;
        stats->rays = g.local_pixels;
        stats->hit_rays = counters[3];
        stats->projected = counters[4];
        stats->identity = counters[5];
        stats->listed_rays = counters[0];
        stats->group_tests = counters[1];
        stats->bound_tests = counters[2];
    }
    return finish(r, s, stats, t0);
}

// ---- adaptive sampling -------------------------------------------------------------------------

// d_sm_counters: the scan's totals (4 u64), the tracer's work index (u32, a slot of its own),
// then the tally slots
constexpr size_t kSampleTotalsWord = 0, kSampleWorkWord = 8, kSampleTallyWord = 16;
constexpr size_t kSampleCounterWords = kSampleTallyWord + kFeatureCounterWords;

// vcrt_draw_samples' three kernels on device planes; returns when the resolve is done.
VkResult run_samples(uint32_t first, uint32_t max_count, const uint16_t* counts,
                     int32_t accumulate, float4* sums, float4* mean, vcrt_sample_stats* stats) {
    if (g.local_tiles == 0) {  // a rank without tiles has no slot to write
        VCRT_TRY(hipStreamSynchronize(g.stream));
        return VK_SUCCESS;
    }
    for (vcrt::Event& e : g.ev_sm) VCRT_TRY(e.create());
    const uint32_t blocks =
        (g.total_pixels + vcrt::kSampleScanSlots - 1u) / vcrt::kSampleScanSlots;
    VCRT_TRY(g.d_sm_block_sums.reserve(blocks));
    VCRT_TRY(g.d_sm_offsets.reserve(g.total_pixels));
    VCRT_TRY(g.d_sm_counters.reserve(kSampleCounterWords));
    unsigned long long* counters = g.d_sm_counters.data();
    VCRT_TRY(hipMemsetAsync(counters, 0, kSampleCounterWords * sizeof(unsigned long long),
                            g.stream));
    // ---- the scan: block sums, their prefix and the totals; one read-back sizes the rest ----
    vcrt::SampleScanParams sp{};
    sp.counts = counts;
    sp.block_sums = g.d_sm_block_sums.data();
    sp.totals = counters + kSampleTotalsWord;
    sp.offsets = g.d_sm_offsets.data();
    sp.blocks = blocks;
    sp.max_count = max_count;
    sp.total_pixels = g.total_pixels;
    sp.width = g.desc.width;
    sp.height = g.desc.height;
    sp.rank = g.desc.rank;
    sp.world = g.desc.world_size;
    sp.tiles_x = g.tiles_x;
    VCRT_TRY(hipEventRecord(g.ev_sm[0].get(), g.stream));
    sp.phase = 0;
    VkResult r = launch(g.k_sample_scan, blocks, vcrt::kSampleScanBlock, 0, sp);
    if (r != VK_SUCCESS) return r;
    sp.phase = 1;
    r = launch(g.k_sample_scan, 1, vcrt::kSampleScanBlock, 0, sp);
    if (r != VK_SUCCESS) return r;
    unsigned long long totals[4] = {};
    VCRT_TRY(hipMemcpyAsync(totals, sp.totals, sizeof(totals), hipMemcpyDeviceToHost, g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    const uint64_t items = totals[2];
    if (items > vcrt::kSampleMaxItems) return VK_ERROR_FORMAT_NOT_SUPPORTED;
    VCRT_TRY(g.d_sm_items.reserve(items));
    VCRT_TRY(g.d_sm_scratch.reserve(items));
    if (items) {
        sp.items = g.d_sm_items.data();
        sp.phase = 2;
        r = launch(g.k_sample_scan, blocks, vcrt::kSampleScanBlock, 0, sp);
        if (r != VK_SUCCESS) return r;
    }
    VCRT_TRY(hipEventRecord(g.ev_sm[1].get(), g.stream));
    // ---- the tracer: the tables of [first, first + max_count), then the persistent grid ----
    vcrt::SampleTraceParams tp{};
    if (items) {
        r = feature_tables(first, max_count, g.desc.max_depth, tp.scene);
        if (r != VK_SUCCESS) return r;
        tp.items = g.d_sm_items.data();
        tp.scratch = g.d_sm_scratch.data();
        tp.count = static_cast<uint32_t>(items);
        tp.use_lists = g.feature_lists ? 1u : 0u;
        tp.work = reinterpret_cast<uint32_t*>(counters + kSampleWorkWord);
        tp.tallies = counters + kSampleTallyWord;
        const uint32_t grid = query_grid(g.k_trace_samples, tp.count, g.desc.blocks_per_cu);
        VCRT_TRY(hipEventRecord(g.ev_sm[2].get(), g.stream));
        r = launch(g.k_trace_samples, grid, kQueryBlock, 0, tp);
        if (r != VK_SUCCESS) return r;
    } else {
        VCRT_TRY(hipEventRecord(g.ev_sm[2].get(), g.stream));
    }
    VCRT_TRY(hipEventRecord(g.ev_sm[3].get(), g.stream));
    // ---- the resolve ----
    vcrt::SampleResolveParams rp{};
    rp.counts = counts;
    rp.offsets = g.d_sm_offsets.data();
    rp.scratch = g.d_sm_scratch.data();
    rp.sums = sums;
    rp.mean = mean;
    rp.max_count = max_count;
    rp.accumulate = accumulate != 0 ? 1u : 0u;
    rp.total_pixels = g.total_pixels;
    rp.width = g.desc.width;
    rp.height = g.desc.height;
    rp.rank = g.desc.rank;
    rp.world = g.desc.world_size;
    rp.tiles_x = g.tiles_x;
    r = launch(g.k_sample_resolve, (g.total_pixels + 255u) / 256u, 256, 0, rp);
    if (r != VK_SUCCESS) return r;
    VCRT_TRY(hipEventRecord(g.ev_sm[4].get(), g.stream));
    unsigned long long slots[kFeatureCounterWords] = {};
    if (stats && items)
        VCRT_TRY(hipMemcpyAsync(slots, counters + kSampleTallyWord, sizeof(slots),
                                hipMemcpyDeviceToHost, g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    if (stats) {
        unsigned long long tallies[4] = {};
        sum_tallies(slots, kFeatureCounterWords, 4, tallies);
        stats->samples = totals[0];
        stats->pixels = totals[1];
        stats->items = items;
        stats->listed_rays = tallies[0];
        stats->group_tests = tallies[1];
        stats->bound_tests = tallies[2];
        stats->segments = tallies[3];
        float ms = 0.f;
        VCRT_TRY(hipEventElapsedTime(&ms, g.ev_sm[0].get(), g.ev_sm[1].get()));
        stats->scan_ms = ms;
        VCRT_TRY(hipEventElapsedTime(&ms, g.ev_sm[2].get(), g.ev_sm[3].get()));
        stats->kernel_ms = ms;
        VCRT_TRY(hipEventElapsedTime(&ms, g.ev_sm[3].get(), g.ev_sm[4].get()));
        stats->resolve_ms = ms;
    }
    return VK_SUCCESS;
}

vcrt_result draw_samples(bool host, uint32_t first, uint32_t max_count, const uint16_t* counts,
                         int32_t accumulate, float* sums, float* mean, vcrt_sample_stats* stats) {
    const auto t0 = Clock::now();
    // the format errors first, so that they read the same with and without a renderer
    if (max_count == 0 || max_count > vcrt::kSampleMaxCount ||
        static_cast<uint64_t>(first) + max_count > kFeatureMaxIndex)
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!g.begun || !g.stage.module) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (!counts || !sums || mean == sums) return VCRT_ERROR_INITIALIZATION_FAILED;
    // the kernels' 16-byte loads and stores, 2-byte loads of the counts
    const vcrt_result c = pass_ready(
        !host && (misaligned({sums, mean}, 15u) || misaligned({counts}, 1u)), true,
        g.k_trace_samples);
    if (c != VCRT_SUCCESS) return c;
    // the slots the call leaves alone keep what the caller's planes hold: those outside the
    // frame (packed tiles) and, accumulating, every pixel's old sums
    Staging s(g.staging, g.stream);
    VkResult r = s.begin(host, g.local_elems,
                         {Plane{counts, 2, false}, out4(sums, accumulate != 0 || packed_tiles()),
                          out4(mean, packed_tiles())});
    if (r != VK_SUCCESS) return r;
    name_stats(stats, "vcrt_trace_samples");
    r = run_samples(first, max_count, s.at<uint16_t>(0), accumulate, s.at<float4>(1),
                    s.at<float4>(2), stats);
    return finish(r, s, stats, t0);
}

}  // namespace

extern "C" {

vcrt_result vcrt_trace_rays(const float* origins, const float* dirs, uint32_t count,
                            int32_t max_depth, float* radiance, vcrt_ray_hit* hits,
                            vcrt_ray_stats* stats) {
    return trace_rays(true, origins, dirs, count, max_depth, radiance, hits, stats);
}

vcrt_result vcrt_trace_rays_device(const float* origins, const float* dirs, uint32_t count,
                                   int32_t max_depth, float* radiance, vcrt_ray_hit* hits,
                                   vcrt_ray_stats* stats) {
    return trace_rays(false, origins, dirs, count, max_depth, radiance, hits, stats);
}

vcrt_result vcrt_occlude_rays(const float* origins, const float* dirs, const float* tmax,
                              uint32_t count, uint8_t* occluded, vcrt_ray_stats* stats) {
    return occlude_rays(true, origins, dirs, tmax, count, occluded, stats);
}

vcrt_result vcrt_occlude_rays_device(const float* origins, const float* dirs, const float* tmax,
                                     uint32_t count, uint8_t* occluded, vcrt_ray_stats* stats) {
    return occlude_rays(false, origins, dirs, tmax, count, occluded, stats);
}

vcrt_result vcrt_draw_features(uint32_t first, uint32_t n, float* albedo, float* normal_depth,
                               int32_t* sphere, vcrt_feature_stats* stats) {
    return draw_features(true, first, n, albedo, normal_depth, sphere, stats);
}

vcrt_result vcrt_draw_features_device(uint32_t first, uint32_t n, float* albedo,
                                      float* normal_depth, int32_t* sphere,
                                      vcrt_feature_stats* stats) {
    return draw_features(false, first, n, albedo, normal_depth, sphere, stats);
}

vcrt_result vcrt_draw_occlusion(uint32_t first, uint32_t n, uint32_t m, float reach,
                                float* visibility, vcrt_occlusion_buffer_stats* stats) {
    return draw_occlusion(true, first, n, m, reach, visibility, stats);
}

vcrt_result vcrt_draw_occlusion_device(uint32_t first, uint32_t n, uint32_t m, float reach,
                                       float* visibility, vcrt_occlusion_buffer_stats* stats) {
    return draw_occlusion(false, first, n, m, reach, visibility, stats);
}

vcrt_result vcrt_draw_motion(const vcrt_camera* prev_camera, const vcrt_sphere* prev_spheres,
                             int32_t count, float* motion, float* surface,
                             vcrt_motion_stats* stats) {
    return draw_motion(true, prev_camera, prev_spheres, count, motion, surface, stats);
}

vcrt_result vcrt_draw_motion_device(const vcrt_camera* prev_camera,
                                    const vcrt_sphere* prev_spheres, int32_t count, float* motion,
                                    float* surface, vcrt_motion_stats* stats) {
    return draw_motion(false, prev_camera, prev_spheres, count, motion, surface, stats);
}

vcrt_result vcrt_draw_samples(uint32_t first, uint32_t max_count, const uint16_t* counts,
                              int32_t accumulate, float* sums, float* mean,
                              vcrt_sample_stats* stats) {
    return draw_samples(true, first, max_count, counts, accumulate, sums, mean, stats);
}

vcrt_result vcrt_draw_samples_device(uint32_t first, uint32_t max_count, const uint16_t* counts,
                                     int32_t accumulate, float* sums, float* mean,
                                     vcrt_sample_stats* stats) {
    return draw_samples(false, first, max_count, counts, accumulate, sums, mean, stats);
}

}  // extern "C"
