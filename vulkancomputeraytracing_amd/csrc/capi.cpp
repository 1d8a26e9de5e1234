// capi.cpp -- the C ABI (include/vcrt.h): renderer state, device buffers, launches.
//
// Replaces the compute half of the reference's Renderer.cpp: the rgba32f storage image
// (Renderer.cpp:433-468) becomes a device float4 buffer, the compute pipeline
// (:532-543) a HIP module, and the per-frame vkCmdDispatch(W/16,H/16,1) + vkQueueSubmit
// (:204-225, :673-686) one persistent-kernel launch on a HIP stream. All state is one object
// (renderer_state.hpp), as in the reference (Renderer.cpp:13-33): one renderer per process. Its
// device buffers, pinned buffers and events are owners (device_resources.hpp) that free
// themselves, so teardown is an assignment of a fresh state (vcrt_end) and there is no list of
// frees to maintain. The ray and occlusion queries and the passes that trace the frame's own rays
// (vcrt_draw_features, vcrt_draw_occlusion, vcrt_draw_motion, vcrt_draw_samples) are in
// ray_passes.cpp, the passes over caller-supplied planes (vcrt_denoise, vcrt_reproject, the
// variance chain, vcrt_sample_counts) in image_passes.cpp.
#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include "Shader.hpp"
#include "camera_lists_abi.h"
#include "cluster.hpp"
#include "comm_wait.hpp"
#include "device_resources.hpp"
#include "hip_status.hpp"
#include "renderer_state.hpp"
#include "scene.hpp"
#include "scene_update_abi.h"
#include "vcrt.h"
#include "vcrt_kernel_abi.h"
#include "vcrt_math.h"

// The one state (renderer_state.hpp, where the comment on why it is never deleted stands).
vcrt::RendererState& vcrt::g = *new vcrt::RendererState;

namespace {

using vcrt::DeviceBuffer;
using vcrt::Event;
using vcrt::camera_array;
using vcrt::camera_of;
using vcrt::g;
using vcrt::launch;
using vcrt::lens_on;
using vcrt::make_jitter;
using vcrt::PinnedBuffer;
using vcrt::RendererState;
using vcrt::to_vk;

// segments (u64 at 8), work_done[2] (u64 at 16), then the work-queue counters from 256
constexpr size_t kCounterBytes = 256 + vcrt::kMaxQueues * 4 * vcrt::kQueueStride;
// LDS for the SMEM scan's staged tables (a few spheres' shading rows and the jitter table)
constexpr uint32_t kStageMaxBytes = 8192;
constexpr int32_t kDefaultChunk = 64;        // samples per work item (upper end)
constexpr uint32_t kRegionCount = 88;       // tracer.hip kRegions: region counters per wave
constexpr uint32_t kRegionDebugBase = 40;   // their sums in vcrt_stats.debug[40..127]

// Samples per work item when the caller leaves it to us: 64, halved (down to 16) while the
// largest rank's share of the frame would be fewer than kChunkItems = 2^24 - 2^21 items (~45 per
// lane of the persistent grid, ~330k lanes on MI355X); at least spp / 512 (at most
// kAccumMaxChunks chunks per pixel). Smaller items cost more than they save in balance: every
// item start and end (slot fetch, pixel set-up, three f64 atomics whose completion later loads
// wait for) is paid by the whole wave, and the tail of the partition (work_tail) now absorbs the
// drain that small items used to shorten. Measured at round 2 with the tail
// (profiles/r02_tail_sweep.txt, kernel ms per rank at the C4 workload): one GPU K = 64 127.0 /
// K = 32 129.3 -> 64; 2-way shards 64.3 / 65.2 -> 64; 4-way K = 32 33.4 / K = 16 33.9 -> 32;
// 8-way K = 16 17.6 / K = 32 17.7-18.1 -> 16; C3 (256 spp) K = 32 33.55 / K = 16 33.80 -> 32.
// All ranks of a frame use the same K (the largest rank's share decides); the image depends on
// the accumulation quantum alone (work_quantum), whatever K and the tail are.
// Round 3 stopped small frames (fewer than 2^22 items at K = 32) at K = 32, measured then at C2
// (K = 32 1.35 ms against K = 16 1.47 ms, when the item was also the accumulation quantum and
// every item end read its ring entry back). Round 4 dropped that floor: with the quantum
// decoupled and the claim-time ring clearing, C2 takes 0.878-0.894 ms at K = 16 against
// 0.936-0.959 at K = 32 (K = 8: 0.882-0.896; profiles/r04_ab_log.md).
constexpr uint64_t kChunkItems = (uint64_t{1} << 24) - (uint64_t{1} << 21);
// Round 5: also halved (down to 16) while a pixel has fewer than kMinChunksPerPixel items: a
// block (64 items, all chunks of 64 / nchunks pixels) then spans few pixels, so the wave's
// 14-entry accumulation ring covers the pixels of its last ~3 blocks and long items keep their
// entries (C3: K = 32 gave 9-pixel blocks, and most quanta missed the ring: 2.5 GB of atomics
// per frame; VCRT_CHUNK_RULE=items restores the item-count rule alone).
constexpr int32_t kMinChunksPerPixel = 16;
// Round 5, the cost partition: where the item count would halve K below the per-pixel rule's K
// (the 8- and 4-way shards of C4), K stays at the per-pixel rule's value, the partition has no
// tail and the frame runs the cost order (vcrt_draw_next_frame): the last items of a sharded frame
// are then cheap ones, not the deep pixels whose 64-sample items outlast the queue by ~3 ms
// (profiles/r05_ab_log.md: 8-way max rank 11.78 ms against 12.16 with K = 16 + 128 x 4, 4-way
// 22.94 against 23.11). `allow_cost`: the desc may take it (cost_allowed); `cost` (may be null)
// reports whether it does.
int32_t default_chunk(uint64_t rank_slots, int32_t spp, bool allow_cost = false,
                      bool* cost = nullptr) {
    const char* rule = std::getenv("VCRT_CHUNK_RULE");
    const bool per_pixel = !(rule && std::strcmp(rule, "items") == 0);
    int32_t k = kDefaultChunk;
    // the per-pixel rule, then the item-count rule (both conditions are monotone in K)
    while (k > 16 && per_pixel && spp / k < kMinChunksPerPixel) k /= 2;
    const int32_t k_pixel = k;
    while (k > 16 && rank_slots * static_cast<uint64_t>((spp + k - 1) / k) < kChunkItems) k /= 2;
    const bool c = allow_cost && k < k_pixel;
    if (cost) *cost = c;
    if (c) k = k_pixel;
    const int32_t k_min = (spp + vcrt::kAccumMaxChunks - 1) / vcrt::kAccumMaxChunks;
    return std::max(k, k_min);
}

// 8x8 tiles of a W x H frame owned by `rank`: (tx, ty) with (tx + ty) % world == rank
// (vcrt_math.h tile_of / owner_of).
uint32_t tiles_for_rank(int32_t width, int32_t height, int32_t world, int32_t rank) {
    const uint32_t tiles_x = static_cast<uint32_t>((width + 7) / 8);
    const uint32_t tiles_y = static_cast<uint32_t>((height + 7) / 8);
    uint64_t n = 0;
    for (uint32_t ty = 0; ty < tiles_y; ty++)
        n += vcrt::tiles_in_row((static_cast<uint32_t>(rank) + static_cast<uint32_t>(world) -
                                 ty % static_cast<uint32_t>(world)) %
                                    static_cast<uint32_t>(world),
                                tiles_x, static_cast<uint32_t>(world));
    return static_cast<uint32_t>(n);
}

// The accumulation quantum G (vcrt.h accumulate_quantum): the image depends on G alone. A
// pixel's samples are summed in fp32 within each run of G consecutive samples, and the runs'
// sums are quantized and added exactly (vcrt_math.h "Accumulation"), at most kAccumMaxChunks of
// them per pixel: 4, doubled while the frame's samples would need more. G does not depend on
// the number of GPUs, so a sharded frame equals the one-GPU frame bit for bit with default descs
// (round 4; before, the chunk was the quantum and followed the rank's share: K = 64 on one GPU,
// 16 at N = 8, so the default images differed). Work items (chunks, the tail) hold whole quanta,
// so G bounds the tail's item size from below, which sets the drain at N = 8: with G = 4 the
// default partitions are round 3's (K = 64 + 64 x 8 on one GPU, K = 16 + 128 x 4 at N = 8);
// measured at C4, the 8-way max rank 13.42 / 13.48 / 14.39 ms with G = 4 / 8 / 16, and the one-GPU
// frame within 0.5% for the three (profiles/r04_ab_log.md).
constexpr int32_t kDefaultQuantum = 4;

int32_t work_quantum(const vcrt_render_desc& d) {
    if (d.accumulate_quantum > 0) return d.accumulate_quantum;
    int32_t q = kDefaultQuantum;
    while ((d.samples_per_pixel + q - 1) / q > vcrt::kAccumMaxChunks) q *= 2;
    return q;
}

int32_t round_up(int32_t x, int32_t q) { return static_cast<int32_t>((int64_t{x} + q - 1) / q * q); }

uint32_t max_rank_tiles(const vcrt_render_desc& d) {
    uint32_t max_tiles = 0;
    for (int32_t rr = 0; rr < d.world_size; rr++)
        max_tiles = std::max(max_tiles, tiles_for_rank(d.width, d.height, d.world_size, rr));
    return max_tiles;
}

// Whether a desc may take the cost partition (default_chunk): chunk and tail left to the rules, a
// kernel variant with a cost-order build (the linear and flat scans; AUTO picks one of them), and
// no static order asked for (VCRT_WORK_ORDER set to anything but "cost").
bool cost_allowed(const vcrt_render_desc& d) {
    if (d.accumulate_chunk > 0 || d.accumulate_tail != 0) return false;
    if (d.kernel_variant != VCRT_KERNEL_AUTO && d.kernel_variant != VCRT_KERNEL_SMEM &&
        d.kernel_variant != VCRT_KERNEL_LDS && d.kernel_variant != VCRT_KERNEL_CULL_FLAT)
        return false;
    const char* order = std::getenv("VCRT_WORK_ORDER");
    return !order || std::strcmp(order, "cost") == 0;
}

bool cost_partition(const vcrt_render_desc& d) {
    bool cost = false;
    (void)default_chunk(64ull * max_rank_tiles(d), d.samples_per_pixel, cost_allowed(d), &cost);
    return cost;
}

// Samples per work item for a desc: its accumulate_chunk, else the default for the largest rank's
// share of the frame; rounded up to whole quanta and capped at spp.
int32_t work_chunk(const vcrt_render_desc& d) {
    const int32_t k = d.accumulate_chunk > 0
                          ? d.accumulate_chunk
                          : default_chunk(64ull * max_rank_tiles(d), d.samples_per_pixel,
                                          cost_allowed(d));
    return std::min(round_up(k, work_quantum(d)), d.samples_per_pixel);
}

// The tail of the partition (vcrt.h vcrt_work_tail): the last T samples of every pixel in items
// of KT samples, handed out after the head. An item started just before the queue drains runs to
// its end while the rest of the chip idles, and its latency is K samples' worth of wave
// iterations (~13 us each at full occupancy: up to ~2 ms at K = 16, ~8 ms at K = 64). The tail
// keeps every lane busy with short items until the head's last items are done, so the head must
// cover ~6 of its items per lane: T ~ 6 K L / P for the L = 327680 lanes of the persistent grid and
// the P pixel slots of the largest rank. Measured at C4 (profiles/r02_tail_sweep.txt, kernel ms):
// one GPU K = 64 128.2 -> 127.0 with T = 64, KT = 8; 8-way shards K = 16 18.0 -> 17.6 with
// T = 128, KT = 4 (a head of K = 64 stays above 21 ms at N = 8 with any tail up to 384).
constexpr uint64_t kTailLaneItems = 6ull * 327680ull;

int32_t work_tail(const vcrt_render_desc& d, int32_t chunk, int32_t* tail_chunk) {
    const int32_t spp = d.samples_per_pixel;
    const int32_t q = work_quantum(d);
    *tail_chunk = 1;
    if (d.accumulate_tail < 0 || chunk >= spp) return 0;
    int32_t t = 0, kt = d.accumulate_tail_chunk;
    if (d.accumulate_tail > 0) {
        t = std::min(d.accumulate_tail, spp - 1);
    } else {
        if (cost_partition(d)) return 0;  // the cost order runs the cheap items last instead
        const uint32_t max_tiles = max_rank_tiles(d);
        // none when the head alone gives every lane many items (>= 2 kChunkItems: ~90 per lane):
        // the drain is then a small part of the frame and the tail's short items cost more than
        // they save. Measured round 5 (tools/ab.py, kernel ms, same bits): one GPU C4 89.68 ->
        // 89.40 without the tail, C3 23.52 -> 23.14, C5 2518 -> 2497; with it, C4 2-way shards
        // 45.18 against 46.07 and 4-way 23.21 against 23.33, 8-way 12.01 against 12.16.
        const uint64_t head_items = 64ull * max_tiles *
                                    static_cast<uint64_t>((spp + chunk - 1) / chunk);
        if (head_items >= 2ull * kChunkItems) return 0;
        const double raw = static_cast<double>(kTailLaneItems) * chunk / (64.0 * max_tiles);
        if (raw < 1.0) return 0;
        t = 1 << static_cast<int>(std::lround(std::log2(raw)));  // nearest power of two
        if (4 * static_cast<int64_t>(t) > spp) return 0;
    }
    // whole quanta: the head ends on a quantum boundary (the tail grows to it), tail items of
    // max(4, K / 8) samples (the rule) or as given, rounded up to whole quanta, the last one
    // ending at spp
    const int32_t head_end = (spp - t) / q * q;
    if (head_end <= 0) return 0;
    t = spp - head_end;
    kt = round_up(kt <= 0 ? std::max(4, chunk / 8) : kt, q);
    *tail_chunk = std::min(kt, t);
    return t;
}

// A multiplier m with (i * m) >> 32 == i / n for every item index i < 64 n of a part (the
// chunk-minor slot split, TraceParams.nch_magic), checked here for every such i; 0 when there is
// none (n <= 1, or n too large for the error term).
uint32_t division_magic(uint32_t n) {
    if (n <= 1u || n > 8192u) return 0u;
    const uint64_t m = ((uint64_t{1} << 32) + n - 1u) / n;  // ceil(2^32 / n) < 2^32
    for (uint64_t i = 0; i < 64ull * n; i++)
        if (((i * m) >> 32) != i / n) return 0u;
    return static_cast<uint32_t>(m);
}

// sRGB8 thresholds: T_k = the smallest float >= the linear value whose exact sRGB encode is
// (k - 0.5) / 255, k = 1..255, so that #{k : c >= T_k} is round-to-nearest of 255 * encode(c).
void srgb_thresholds(float out[255]) {
    for (int k = 1; k <= 255; k++) {
        const double s = (k - 0.5) / 255.0;
        const double lin = s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4);
        float t = static_cast<float>(lin);
        if (static_cast<double>(t) < lin) t = std::nextafter(t, 2.0f);
        out[k - 1] = t;
    }
}

// Directory of this shared object (for the default code-object path).
std::string library_dir() {
    Dl_info info;
    if (dladdr(reinterpret_cast<void*>(&tiles_for_rank), &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        const size_t slash = p.find_last_of('/');
        if (slash != std::string::npos) return p.substr(0, slash);
    }
    return ".";
}

void free_scene() {
    for (DeviceBuffer<float4>* b : {&g.d_geom, &g.d_center_radius, &g.d_shade, &g.d_material,
                                    &g.d_cgroup, &g.d_cbound, &g.d_cbound_nf, &g.d_cnode,
                                    &g.d_cnode_nf, &g.d_ctop})
        b->reset();
    g.d_fp_tab.reset();
    g.d_gf_tab.reset();
    g.cgf_ok = false;
    g.cgf_n = 0;
    g.d_prim_info.reset();
    g.d_prim_ids.reset();
    g.d_cam_rec.reset();
    g.prim_nids = g.prim_npairs = 0;
    g.ncgroups = 0;
    g.ncbig = 0;
    g.nspheres = 0;
}

// CullTables::fp_tab as the LDS-table kernel copies it (vcrt::foot_lds_bytes): two 16-bit masks
// per word when the scene has at most 16 nodes, else one 32-bit mask per word.
std::vector<uint32_t> pack_footprint(const vcrt::CullTables& ct) {
    static_assert(vcrt::kFootCells == static_cast<uint32_t>(vcrt::kFootprintCells) &&
                      vcrt::kFootCells % 2u == 0u,
                  "footprint cells");
    if (ct.ngroups > 128) return ct.fp_tab;
    std::vector<uint32_t> out(ct.fp_tab.size() / 2);
    for (size_t i = 0; i < out.size(); i++)
        out[i] = (ct.fp_tab[2 * i] & 0xffffu) | (ct.fp_tab[2 * i + 1] << 16);
    return out;
}

// A pair-SoA box table (cluster.hpp: 16 floats per pair of boxes) in the near/far layout of
// TraceParams.cbound_nf (20 floats per pair: per axis lo0 lo1 hi0 hi1 lo0 lo1, then K0 K1).
std::vector<float> near_far(const std::vector<float>& pairs) {
    const size_t n = pairs.size() / 16;
    std::vector<float> nf(n * 20);
    for (size_t i = 0; i < n; i++) {
        const float* b = &pairs[i * 16];
        float* o = &nf[i * 20];
        for (int a = 0; a < 3; a++) {  // lo of axis a at b[2a], hi at b[6 + 2a]
            o[6 * a + 0] = o[6 * a + 4] = b[2 * a];
            o[6 * a + 1] = o[6 * a + 5] = b[2 * a + 1];
            o[6 * a + 2] = b[6 + 2 * a];
            o[6 * a + 3] = b[6 + 2 * a + 1];
        }
        o[18] = b[12];
        o[19] = b[13];
    }
    return nf;
}

// the flat scan's chunk passes read a chunk's 4 node pairs: the node table padded to whole chunks
std::vector<float> node_near_far(const vcrt::CullTables& ct) {
    std::vector<float> nodes = ct.node;
    const size_t pairs = nodes.size() / 16, padded = (pairs + 3) / 4 * 4;
    nodes.resize(padded * 16, 0.0f);
    return near_far(nodes);
}

// A host table into an (empty) scene buffer of its size, on the null stream.
template <typename T, typename H>
hipError_t upload(DeviceBuffer<T>& out, const std::vector<H>& table) {
    const size_t bytes = sizeof(H) * table.size();
    const hipError_t e = out.reserve((bytes + sizeof(T) - 1) / sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemcpy(out.data(), table.data(), bytes, hipMemcpyHostToDevice);
}

// Every |center component| and |radius| <= 2^30: discriminants stay finite (scene_bounded).
bool values_bounded(const vcrt_sphere* s, int32_t count) {
    for (int32_t i = 0; i < count; i++)
        for (float v : {s[i].center[0], s[i].center[1], s[i].center[2], s[i].radius})
            if (!(std::fabs(v) <= 0x1p30f)) return false;  // also rejects NaN
    return true;
}

// Every |radius| in [2^-40, 2^30] (kFlagRadiiSafe).
bool values_radii_safe(const vcrt_sphere* s, int32_t count) {
    for (int32_t i = 0; i < count; i++)
        if (!(std::fabs(s[i].radius) >= 0x1p-40f && std::fabs(s[i].radius) <= 0x1p30f))
            return false;
    return true;
}

// The linear scan table of a scene (vcrt_set_scene): count / 4 groups rounded up, one more for
// the prefetch, padding entries (0, 0, 0, r² = -3e38).
std::vector<float> linear_table(const vcrt_sphere* spheres, int32_t count) {
    const int32_t ngroups = (count + 3) / 4;
    std::vector<float> table(static_cast<size_t>(ngroups + 1) * 16, 0.0f);
    for (int32_t j = 0; j < 4 * (ngroups + 1); j++) {
        float* gq = &table[static_cast<size_t>(j / 4) * 16];
        const int pair = (j % 4) / 2, e = j % 2;
        float cx = 0.f, cy = 0.f, cz = 0.f, r2 = -3.0e38f;
        if (j < count) {
            const vcrt_sphere& sp = spheres[j];
            cx = sp.center[0];
            cy = sp.center[1];
            cz = sp.center[2];
            r2 = sp.radius * sp.radius;
        }
        float* base = gq + 8 * pair;
        base[0 + e] = cx;
        base[2 + e] = cy;
        base[4 + e] = cz;
        base[6 + e] = r2;
    }
    return table;
}

// The per-sphere rows: (centre, radius), (colour, param), (material id, 1 / param, r0², 0).
void sphere_rows(const vcrt_sphere* spheres, int32_t count, std::vector<float4>& cr,
                 std::vector<float4>& shade, std::vector<float4>& mat) {
    cr.resize(count);
    shade.resize(count);
    mat.resize(count);
    for (int32_t i = 0; i < count; i++) {
        const vcrt_sphere& sp = spheres[i];
        cr[i] = make_float4(sp.center[0], sp.center[1], sp.center[2], sp.radius);
        shade[i] = make_float4(sp.colour[0], sp.colour[1], sp.colour[2], sp.texture[1]);
        // the glass scatter's two per-sphere quotients (textures.glsl:49-50, functions.glsl:58-60),
        // fp32 and correctly rounded as the kernel would compute them
        const float ior = sp.texture[1];
        float r0 = (1.0f - ior) / (1.0f + ior);
        r0 = r0 * r0;
        mat[i] = make_float4(sp.texture[0], 1.0f / ior, r0, 0.0f);
    }
}

// group records: the four pair-SoA float4s + the member indices (int bits); big groups first
std::vector<float> group_records(const vcrt::CullTables& ct) {
    const int32_t nall = ct.nbig + ct.ngroups;
    std::vector<float> rec(static_cast<size_t>(nall) * 20);
    for (int32_t gi = 0; gi < nall; gi++) {
        std::memcpy(&rec[gi * 20], &ct.geom[gi * 16], 16 * sizeof(float));
        std::memcpy(&rec[gi * 20 + 16], &ct.index[gi * 4], 4 * sizeof(int32_t));
    }
    return rec;
}

// Every entry point the library binds. Group 0 is required: a code object without one (e.g. an
// A/B build of an older tree) is an incompatible shader binary, not an unknown error
// (hipErrorNotFound used to map to VK_ERROR_UNKNOWN: profiles/r04_ab_log.md, run 7). Every other
// group is optional (code objects built before the feature lack it, and the call that needs it
// answers VK_ERROR_FEATURE_NOT_PRESENT or takes its host path) and all or nothing: a group with
// a miss has none of its kernels.
struct KernelRow {
    hipFunction_t RendererState::*field;
    const char* name;
    int group;
};
using RS = RendererState;
constexpr KernelRow kKernels[] = {
    {&RS::k_trace_lds, "vcrt_trace_lds", 0},
    {&RS::k_trace_smem, "vcrt_trace_smem", 0},
    {&RS::k_assemble, "vcrt_assemble", 0},
    {&RS::k_fill, "vcrt_fill", 0},
    {&RS::k_resolve, "vcrt_resolve", 0},
    {&RS::k_encode, "vcrt_encode_srgb8", 0},
    {&RS::k_setup_jitter, "vcrt_setup_jitter", 0},
    {&RS::k_trace_lds_stats, "vcrt_trace_lds_stats", 0},
    {&RS::k_trace_smem_stats, "vcrt_trace_smem_stats", 0},
    {&RS::k_trace_cull, "vcrt_trace_cull", 0},
    {&RS::k_trace_cull_stats, "vcrt_trace_cull_stats", 0},
    {&RS::k_trace_cull_lane_lds, "vcrt_trace_cull_lane_lds", 0},
    {&RS::k_trace_cull_lane_lds_stats, "vcrt_trace_cull_lane_lds_stats", 0},
    {&RS::k_trace_cull_lane, "vcrt_trace_cull_lane", 0},
    {&RS::k_trace_cull_lane_stats, "vcrt_trace_cull_lane_stats", 0},
    {&RS::k_trace_cull_lane_lds_wide, "vcrt_trace_cull_lane_lds_wide", 0},
    {&RS::k_trace_cull_lane_lds_wide_stats, "vcrt_trace_cull_lane_lds_wide_stats", 0},
    {&RS::k_trace_cull_flat, "vcrt_trace_cull_flat", 0},
    {&RS::k_trace_cull_flat_stats, "vcrt_trace_cull_flat_stats", 0},
    {&RS::k_trace_cull_flat_global, "vcrt_trace_cull_flat_global", 0},
    {&RS::k_trace_cull_flat_global_stats, "vcrt_trace_cull_flat_global_stats", 0},
    // the boxes-in-LDS flat scan and its stats build, both or neither
    {&RS::k_trace_cull_flat_boxes, "vcrt_trace_cull_flat_boxes", 1},
    {&RS::k_trace_cull_flat_boxes_stats, "vcrt_trace_cull_flat_boxes_stats", 1},
    // the flat scans' cost-order builds, each on its own
    {&RS::k_trace_cull_flat_cost, "vcrt_trace_cull_flat_cost", 2},
    {&RS::k_trace_cull_flat_global_cost, "vcrt_trace_cull_flat_global_cost", 3},
    {&RS::k_trace_cull_flat_boxes_cost, "vcrt_trace_cull_flat_boxes_cost", 4},
    {&RS::k_trace_rays, "vcrt_trace_rays", 5},
    // the thin-lens frame kernels, each on its own (lens_kernels_bound asks for all seven)
    {&RS::k_smem_lens, "vcrt_trace_smem_lens", 6},
    {&RS::k_flat_lens, "vcrt_trace_cull_flat_lens", 7},
    {&RS::k_flat_lens_cost, "vcrt_trace_cull_flat_lens_cost", 8},
    {&RS::k_flat_global_lens, "vcrt_trace_cull_flat_global_lens", 9},
    {&RS::k_flat_global_lens_cost, "vcrt_trace_cull_flat_global_lens_cost", 10},
    {&RS::k_flat_boxes_lens, "vcrt_trace_cull_flat_boxes_lens", 11},
    {&RS::k_flat_boxes_lens_cost, "vcrt_trace_cull_flat_boxes_lens_cost", 12},
    {&RS::k_occlude_rays, "vcrt_occlude_rays", 13},
    {&RS::k_frame_features, "vcrt_frame_features", 14},
    {&RS::k_frame_occlusion, "vcrt_frame_occlusion", 15},
    // the denoise kernels, both or neither
    {&RS::k_denoise_pass, "vcrt_denoise_pass", 16},
    {&RS::k_denoise_pass_lds, "vcrt_denoise_pass_lds", 16},
    {&RS::k_reproject_pass, "vcrt_reproject_pass", 25},
    {&RS::k_frame_motion, "vcrt_frame_motion", 26},
    // variance-guided denoising: the moments pass, the two variance passes and the two steered
    // denoise passes, each pair both or neither
    {&RS::k_reproject_moments_pass, "vcrt_reproject_moments_pass", 27},
    {&RS::k_variance_pass, "vcrt_variance_pass", 28},
    {&RS::k_variance_pass_lds, "vcrt_variance_pass_lds", 28},
    {&RS::k_denoise_var_pass, "vcrt_denoise_var_pass", 29},
    {&RS::k_denoise_var_pass_lds, "vcrt_denoise_var_pass_lds", 29},
    // adaptive sampling: the scan, the tracer and the resolve, all or none; the count rule
    {&RS::k_sample_scan, "vcrt_sample_scan", 30},
    {&RS::k_trace_samples, "vcrt_trace_samples", 30},
    {&RS::k_sample_resolve, "vcrt_sample_resolve", 30},
    {&RS::k_sample_counts_pass, "vcrt_sample_counts_pass", 31},
    // the camera-list kernels, each on its own (vcrt_set_camera asks for all four, else it runs
    // the host builders)
    {&RS::k_cl_prepare, "vcrt_camlist_prepare", 17},
    {&RS::k_cl_count, "vcrt_camlist_count", 18},
    {&RS::k_cl_scan, "vcrt_camlist_scan", 19},
    {&RS::k_cl_fill, "vcrt_camlist_fill", 20},
    // the scene-refit kernels, likewise (vcrt_update_spheres else rebuilds as vcrt_set_scene)
    {&RS::k_su_rows, "vcrt_scene_rows", 21},
    {&RS::k_su_groups, "vcrt_scene_groups", 22},
    {&RS::k_su_levels, "vcrt_scene_levels", 23},
    {&RS::k_su_footprint, "vcrt_scene_footprint", 24},
};
constexpr size_t kKernelCount = sizeof(kKernels) / sizeof(kKernels[0]);

// The table's entry points of module m into fn (parallel to kKernels); the state is not touched.
VkResult bind_kernels(hipModule_t m, hipFunction_t (&fn)[kKernelCount]) {
    for (size_t i = 0; i < kKernelCount; i++) {
        const hipError_t e = hipModuleGetFunction(&fn[i], m, kKernels[i].name);
        if (e == hipSuccess) continue;
        fn[i] = nullptr;
        if (kKernels[i].group == 0)
            return e == hipErrorNotFound ? VK_ERROR_INCOMPATIBLE_SHADER_BINARY_EXT : to_vk(e);
        (void)hipGetLastError();
    }
    for (size_t i = 0; i < kKernelCount; i++)
        if (fn[i] == nullptr)
            for (size_t j = 0; j < kKernelCount; j++)
                if (kKernels[j].group == kKernels[i].group) fn[j] = nullptr;
    return VK_SUCCESS;
}

// Loads a code object (path; null: the one beside the library, else the embedded copy) and binds
// its kernels, then commits: only when every required kernel is there does the new module take
// the old one's place. A failed load leaves the stage and every kernel as they were.
VkResult load_code_object(const char* path) {
    VkPipelineShaderStageCreateInfo stage{};
    VkResult r;
    if (path) {
        r = CreateShaderStageFromFile(path, VK_SHADER_STAGE_COMPUTE_BIT, &stage);
    } else {
        const std::string def = library_dir() + "/vcrt_tracer.hsaco";
        r = access(def.c_str(), R_OK) == 0
                ? CreateShaderStageFromFile(def.c_str(), VK_SHADER_STAGE_COMPUTE_BIT, &stage)
                : VK_ERROR_INCOMPATIBLE_SHADER_BINARY_EXT;
        if (r != VK_SUCCESS)  // embedded copy, as LOAD_SHADER_FROM_MEMORY
            r = CreateShaderStageFromFile(nullptr, VK_SHADER_STAGE_COMPUTE_BIT, &stage);
    }
    if (r != VK_SUCCESS) return r;
    hipFunction_t fn[kKernelCount];
    r = bind_kernels(static_cast<hipModule_t>(stage.module), fn);
    if (r != VK_SUCCESS) {
        DestroyShaderStage(&stage);
        return r;
    }
    DestroyShaderStage(&g.stage);
    g.stage = stage;
    for (size_t i = 0; i < kKernelCount; i++) g.*kKernels[i].field = fn[i];
    return VK_SUCCESS;
}

// The caller's description as this library's struct. struct_size is sizeof(vcrt_render_desc), or
// the size of the struct before lens_radius was appended (a binary built against that header):
// the field then reads 0. (Where the field fits the struct's tail padding -- LP64 -- the two
// sizes are equal and the field is read.)
constexpr size_t kDescSizeNoLens = (offsetof(vcrt_render_desc, lens_radius) +
                                    alignof(vcrt_render_desc) - 1) /
                                   alignof(vcrt_render_desc) * alignof(vcrt_render_desc);
bool read_desc(const vcrt_render_desc* in, vcrt_render_desc& out) {
    if (!in) return false;
    if (in->struct_size == sizeof(vcrt_render_desc)) {
        out = *in;
        return true;
    }
    if (in->struct_size != kDescSizeNoLens) return false;
    out = vcrt_render_desc{};
    std::memcpy(&out, in, offsetof(vcrt_render_desc, lens_radius));
    out.struct_size = sizeof(vcrt_render_desc);
    return true;
}

bool lens_kernels_bound() {
    return g.k_smem_lens && g.k_flat_lens && g.k_flat_lens_cost && g.k_flat_global_lens &&
           g.k_flat_global_lens_cost && g.k_flat_boxes_lens && g.k_flat_boxes_lens_cost;
}

bool desc_valid(const vcrt_render_desc& d) {
    if (d.struct_size != sizeof(vcrt_render_desc)) return false;
    if (!(d.lens_radius >= 0.0f) || std::isinf(d.lens_radius)) return false;  // (NaN: false)
    if (d.width <= 0 || d.height <= 0 || d.samples_per_pixel <= 0 || d.max_depth < 0)
        return false;
    if (static_cast<int64_t>(d.width) * d.height > (int64_t{1} << 31)) return false;
    if (d.width > 65535 || d.height > 65535) return false;  // kernels pack y << 16 | x
    if (d.world_size <= 0 || d.rank < 0 || d.rank >= d.world_size) return false;
    if (d.blocks_per_cu < 0 || d.accumulate_chunk < 0) return false;
    if (d.accumulate_quantum < 0 || (d.accumulate_quantum & (d.accumulate_quantum - 1)) != 0)
        return false;  // a power of two (the kernel masks the sample index with G - 1)
    if (d.accumulate_tail < -1 || d.accumulate_tail_chunk < 0) return false;
    if (d.progressive != 0 && d.progressive != 1) return false;
    if (d.kernel_variant < VCRT_KERNEL_AUTO || d.kernel_variant > VCRT_KERNEL_CULL_FLAT) return false;
    return true;
}

// The framebuffer the caller sees: rank 0 of a gathering communicator holds the assembled
// frame [height][width]; otherwise the rank-local framebuffer.
struct FbView {
    float4* ptr;
    uint32_t elems;
};
FbView fb_view() {
    if (g.d_frame.data())
        return {g.d_frame.data(),
                static_cast<uint32_t>(g.desc.width) * static_cast<uint32_t>(g.desc.height)};
    return {g.d_fb, g.local_elems};
}

VkResult nccl_vk(ncclResult_t e) {
    if (e == ncclSuccess) return VK_SUCCESS;
    if (e == ncclSystemError || e == ncclRemoteError) return VK_ERROR_DEVICE_LOST;
    return e == ncclInvalidArgument || e == ncclInvalidUsage ? VK_ERROR_INITIALIZATION_FAILED
                                                             : VK_ERROR_UNKNOWN;
}

// Zero the pixels' sums and their outlier record (a new scene, vcrt_begin, a reset): every
// pixel starts again at the scale 2^32 (vcrt_math.h "Accumulation"). On the render stream, and
// waited for: the render stream is non-blocking, so a memset on the null stream would not be
// ordered before the next frame's kernels (a 2-GiB memset still running then zeroed the last
// rows' sums of an 8192 x 8192 frame).
hipError_t reset_sums() {
    if (g.d_accum.data()) {
        const hipError_t e = hipMemsetAsync(g.d_accum.data(), 0,
                                            32u * static_cast<size_t>(g.total_pixels), g.stream);
        if (e != hipSuccess) return e;
        g.accum_clean = true;
    }
    if (g.d_pixel_emax.data()) {
        const hipError_t e =
            hipMemsetAsync(g.d_pixel_emax.data(), 0,
                           sizeof(uint32_t) * static_cast<size_t>(g.total_pixels), g.stream);
        if (e != hipSuccess) return e;
    }
    if (g.stream) {
        const hipError_t e = hipStreamSynchronize(g.stream);
        if (e != hipSuccess) return e;
    }
    g.pixel_scale = false;
    g.min_scale = vcrt::kAccumMaxScaleLog2;
    g.stats.accumulate_scale_log2 = vcrt::kAccumMaxScaleLog2;
    return hipSuccess;
}

// TraceParams.jitter (vcrt_kernel_abi.h SetupJitterParams): the jitter term of the frame's
// sample indices base .. base + spp - 1 (shader.comp:48), on the device with the tracer's own
// operations, and TraceParams.lens of a lens renderer.
VkResult setup_jitter(uint64_t base, bool corners = false) {
    const int slot = g.jitter_slot;
    g.jitter_slot ^= 1;
    // its last copy (two frames ago) is done
    VCRT_TRY(hipEventSynchronize(g.ev_jitter[slot].get()));
    return vcrt::jitter_tables(
        base, static_cast<uint32_t>(g.desc.samples_per_pixel),
        {g.h_jitter[slot].data(), g.h_lens[slot].data(), g.d_jitter_in.data(), g.d_jitter.data(),
         g.d_lens.data(), corners ? g.d_corner.data() : nullptr, g.ev_jitter[slot].get()});
}

// State of the non-blocking communicator's last operations (comm_wait.hpp): done, still in
// progress, or failed (an asynchronous error: a peer died, a network error).
vcrt::PollState comm_state(ncclComm_t comm) {
    ncclResult_t a = ncclSuccess;
    if (ncclCommGetAsyncError(comm, &a) != ncclSuccess) return vcrt::PollState::kFailed;
    return a == ncclSuccess      ? vcrt::PollState::kDone
           : a == ncclInProgress ? vcrt::PollState::kPending
                                 : vcrt::PollState::kFailed;
}

// Drops the communicator and the gather buffers. abort: ncclCommAbort, which also stops
// operations still running on the device (a receive whose peer is gone), so that the render
// stream drains; else a finalize (bounded) and destroy. Rank 0 renders into its own buffer again.
void comm_release(bool abort) {
    if (g.comm) {
        if (!abort) {
            const ncclResult_t f = ncclCommFinalize(g.comm);
            abort = (f != ncclSuccess && f != ncclInProgress) ||
                    vcrt::wait_with_deadline([] { return comm_state(g.comm); },
                                             vcrt::comm_timeout_ms()) != vcrt::WaitResult::kDone;
        }
        (void)(abort ? ncclCommAbort(g.comm) : ncclCommDestroy(g.comm));
        g.comm = nullptr;
    }
    if (g.stream) (void)hipStreamSynchronize(g.stream);
    g.d_gather.reset();
    g.d_frame.reset();
    g.ev_gather.reset();
    g.ev_gather_start.reset();
    g.d_fb = g.d_fb_own.data();
}

// A communicator failure inside a draw: abort it and report the device lost (the reference's
// errors bubble up as VkResult, VulkanComputeRayTracing.cpp:20-35).
VkResult comm_fail() {
    comm_release(true);
    g.comm_lost = true;
    return VK_ERROR_DEVICE_LOST;
}

// The frame gather, stream-ordered after the trace and resolve: every rank's
// packed tiles (pad_tiles x 64 float4, 4.1 MB per rank at 1080p / 8 GPUs) go to rank 0 in one
// grouped send/recv, so rank 0 receives from all peers at once over their own xGMI links
// (a ring all-gather would move the whole frame through every rank); rank 0 then
// re-interleaves the frame (vcrt_assemble). Every rank takes part, whatever its share. The
// communicator is non-blocking: the group is enqueued when its state leaves ncclInProgress
// (bounded wait), and the caller waits for ev_gather with a deadline (wait_gather).
VkResult gather_frame() {
    VCRT_TRY(hipEventRecord(g.ev_gather_start.get(), g.stream));
    const size_t n = static_cast<size_t>(g.pad_tiles) * 64 * 4;  // floats per rank
    auto ok = [](ncclResult_t e) { return e == ncclSuccess || e == ncclInProgress; };
    bool good = ok(ncclGroupStart());
    if (good) {
        if (g.desc.rank == 0) {
            for (int32_t peer = 1; peer < g.desc.world_size && good; peer++)
                good = ok(ncclRecv(reinterpret_cast<float*>(g.d_gather.data()) + n * peer, n,
                                   ncclFloat32, peer, g.comm, g.stream));
        } else {
            good = ok(ncclSend(g.d_fb, n, ncclFloat32, 0, g.comm, g.stream));
        }
        good = ok(ncclGroupEnd()) && good;
    }
    if (!good || vcrt::wait_with_deadline([] { return comm_state(g.comm); },
                                          vcrt::comm_timeout_ms()) != vcrt::WaitResult::kDone)
        return comm_fail();
    if (g.desc.rank == 0) {
        vcrt::AssembleParams ap{g.d_gather.data(),    g.d_frame.data(),         g.desc.width,
                                g.desc.height, g.desc.world_size, g.tiles_x,
                                g.pad_tiles};
        const uint64_t total = static_cast<uint64_t>(g.desc.width) * g.desc.height;
        const VkResult r = launch(
            g.k_assemble, static_cast<uint32_t>(std::min<uint64_t>((total + 255) / 256, 8192)),
            256, 0, ap);
        if (r != VK_SUCCESS) return r;
    }
    VCRT_TRY(hipEventRecord(g.ev_gather.get(), g.stream));
    return VK_SUCCESS;
}

// Waits for the gather recorded by gather_frame, polling the communicator's asynchronous error
// beside the event: a peer that never sends makes this return VK_ERROR_DEVICE_LOST (after
// aborting the communicator) at the deadline instead of blocking forever.
VkResult wait_gather() {
    hipError_t ev = hipSuccess;
    const vcrt::WaitResult w = vcrt::wait_with_deadline(
        [&ev] {
            ev = hipEventQuery(g.ev_gather.get());
            if (ev == hipSuccess) return vcrt::PollState::kDone;
            if (ev != hipErrorNotReady) return vcrt::PollState::kFailed;
            return comm_state(g.comm) == vcrt::PollState::kFailed ? vcrt::PollState::kFailed
                                                                  : vcrt::PollState::kPending;
        },
        vcrt::gather_timeout_ms(vcrt::comm_timeout_ms(), g.stats.kernel_ms + g.stats.resolve_ms));
    if (w == vcrt::WaitResult::kDone) return VK_SUCCESS;
    if (w == vcrt::WaitResult::kFailed && ev != hipSuccess && ev != hipErrorNotReady) {
        const VkResult r = to_vk(ev);  // the device itself failed
        comm_fail();
        return r;
    }
    return comm_fail();
}

// The tracer kernel a draw launches for the current scene and desc: variant (AUTO resolved),
// entry point, block size and dynamic LDS.
struct KernelChoice {
    hipFunction_t f, stats;
    // the pinhole kernel of the same kind: f itself, or for a lens renderer the kernel whose
    // *_lens build f is (the rules of a draw ask what kind of kernel runs)
    hipFunction_t base;
    // the build a cost-ordered frame launches (it counts pixel segments into
    // TraceParams.pixel_cost and follows TraceParams.block_order); null: no cost order
    hipFunction_t cost;
    const char* name;
    uint32_t block, lds;
    int variant;
};

KernelChoice select_kernel() {
    // scan table: (groups + 1 padding group) x 64 B
    const uint32_t geom_lds = static_cast<uint32_t>(64 * ((g.nspheres + 3) / 4 + 1));
    // per-lane culled scan: tables in LDS. Up to 32 KB with 256-thread workgroups (5 per
    // CU, each with its copy); up to the CU's whole LDS with 1024-thread workgroups (one
    // copy for 16 waves); beyond that from global memory.
    const uint32_t tab_lds = static_cast<uint32_t>(16 * (g.ncgroups / 2 * 4 + g.ncgroups * 5));
    // flat: near/far boxes (80 B per pair, 336 B per node of 4 pairs: 16 B of bank padding),
    // 80-B group records (the uint16 member indices inside), the footprint tables of the node
    // level (672 B, or 1344 B beyond 16 nodes), and where the group-level tables leave their zero
    // row no room in those bytes, 16 B for it (vcrt_kernel_abi.h group_foot_zero_pad; none at the
    // final scene)
    const uint32_t tab_lds_flat =
        static_cast<uint32_t>(16 * (g.ncgroups / 8 * 21 + g.ncgroups * 5)) +
        vcrt::foot_lds_bytes(g.ncgroups) + 16u * vcrt::group_foot_zero_pad(g.ncgroups);
    const bool lane_lds = tab_lds <= g.max_lds && g.cull_lane_tables != 2;
    const bool lane_wide = lane_lds && tab_lds > 32768u;
    int variant = g.desc.kernel_variant;
    // Measured on MI355X (1080p, box hierarchy): of the linear scans the scalar-cache
    // variant (sphere data in SGPRs, no LDS traffic) beats LDS staging by 15% (485
    // spheres) and 18% (4100); the culled scans beat both (same bits). AUTO: the flattened
    // scan (485 spheres: 3.3x SMEM, +14% over CULL_LANE, +28% over CULL; 4100 spheres with
    // its tables in global memory), and SMEM when the scene has no tables (< 16 spheres or
    // unbounded).
    if (variant == VCRT_KERNEL_AUTO)
        variant = g.ncgroups == 0 ? VCRT_KERNEL_SMEM : VCRT_KERNEL_CULL_FLAT;
    if (variant == VCRT_KERNEL_LDS && geom_lds > g.max_lds) variant = VCRT_KERNEL_SMEM;
    if ((variant == VCRT_KERNEL_CULL || variant == VCRT_KERNEL_CULL_LANE ||
         variant == VCRT_KERNEL_CULL_FLAT) &&
        g.ncgroups == 0)
        variant = VCRT_KERNEL_SMEM;
    // The flat scan keeps 4.25 KB of stacks per wave in LDS beside its tables when they fit
    // in 32 KB (16-bit entries), in 256-thread workgroups (five per CU, each with its copy of
    // the tables). Up to 1024 groups (16-bit entries) it keeps only the boxes in LDS, one copy
    // per 1024-thread workgroup; beyond that the tables stay in global memory and the stacks
    // take 32-bit entries (6.75 KB per wave).
    const bool flat_lds = tab_lds_flat <= 32768u && g.cull_lane_tables != 2 &&
                          g.cull_lane_tables != 3 && g.ncgroups <= vcrt::kFlatMaxGroups8;
    // Boxes only (near/far group boxes + node boxes of whole chunks) in LDS, one copy for the
    // 16 waves of a 1024-thread workgroup, beside their 16-bit stacks; the records from global.
    const uint32_t box_lds = static_cast<uint32_t>(
        16 * (g.ncgroups / 8 * 21 + (g.ncgroups + 63) / 64 * 21) + 16 * vcrt::kWaveScratchBytes);
    // Measured at C5 (stress scene, 4K, 4096 spp, depth 50): 11415 against 11186 Msamples/s
    // with every table in global memory (same bits; profiles/r03_c5_boxes_*).
    const bool flat_boxes = !flat_lds && g.k_trace_cull_flat_boxes != nullptr &&
                            g.cull_lane_tables != 2 && g.ncgroups <= vcrt::kFlatMaxGroups &&
                            box_lds <= g.max_lds;
    hipFunction_t f = g.k_trace_smem, fs = g.k_trace_smem_stats;
    const char* fname = "vcrt_trace_smem";
    uint32_t block = 256;
    uint32_t lds = 0;
    if (variant == VCRT_KERNEL_LDS) {
        f = g.k_trace_lds;
        fs = g.k_trace_lds_stats;
        fname = "vcrt_trace_lds";
        lds = geom_lds;
    } else if (variant == VCRT_KERNEL_CULL) {
        f = g.k_trace_cull;
        fs = g.k_trace_cull_stats;
        fname = "vcrt_trace_cull";
    } else if (variant == VCRT_KERNEL_CULL_FLAT && flat_lds) {
        f = g.k_trace_cull_flat;
        fs = g.k_trace_cull_flat_stats;
        fname = "vcrt_trace_cull_flat";
        // (experiments: a code object built with -DVCRT_FLAT_BLOCK=n launches n-thread groups)
        int max_threads = 0;  // only a code object built for that size takes it
        if (g.flat_block > 0 &&
            hipFuncGetAttribute(&max_threads, HIP_FUNC_ATTRIBUTE_MAX_THREADS_PER_BLOCK, f) ==
                hipSuccess &&
            max_threads >= g.flat_block)
            block = static_cast<uint32_t>(g.flat_block);
        lds = tab_lds_flat + (block / 64) * vcrt::kWaveScratchBytes8;
    } else if (variant == VCRT_KERNEL_CULL_FLAT && flat_boxes) {
        f = g.k_trace_cull_flat_boxes;
        fs = g.k_trace_cull_flat_boxes_stats;
        fname = "vcrt_trace_cull_flat_boxes";
        block = 1024;
        lds = box_lds;
    } else if (variant == VCRT_KERNEL_CULL_FLAT) {
        f = g.k_trace_cull_flat_global;
        fs = g.k_trace_cull_flat_global_stats;
        fname = "vcrt_trace_cull_flat_global";
        lds = 4 * vcrt::kWaveScratchBytesWide;
    } else if (variant == VCRT_KERNEL_CULL_LANE && lane_wide) {
        f = g.k_trace_cull_lane_lds_wide;
        fs = g.k_trace_cull_lane_lds_wide_stats;
        fname = "vcrt_trace_cull_lane_lds_wide";
        block = 1024;
        lds = tab_lds;
    } else if (variant == VCRT_KERNEL_CULL_LANE && lane_lds) {
        f = g.k_trace_cull_lane_lds;
        fs = g.k_trace_cull_lane_lds_stats;
        fname = "vcrt_trace_cull_lane_lds";
        lds = tab_lds;
    } else if (variant == VCRT_KERNEL_CULL_LANE) {
        f = g.k_trace_cull_lane;
        fs = g.k_trace_cull_lane_stats;
        fname = "vcrt_trace_cull_lane";
    }
    // the cost order (vcrt_draw_next_frame): the linear scans' product builds have it, the flat
    // scans have separate builds (the hooks cost the product kernel ~0.3% at C4)
    hipFunction_t fc = f == g.k_trace_smem || f == g.k_trace_lds        ? f
                       : f == g.k_trace_cull_flat                        ? g.k_trace_cull_flat_cost
                       : f == g.k_trace_cull_flat_global ? g.k_trace_cull_flat_global_cost
                       : f == g.k_trace_cull_flat_boxes  ? g.k_trace_cull_flat_boxes_cost
                                                         : nullptr;
    const hipFunction_t base = f;
    if (lens_on()) {
        // the thin lens: the *_lens build of the same kernel (vcrt_begin admits AUTO, SMEM and
        // CULL_FLAT only, and no stats builds); null when the code object has none
        fs = nullptr;
        if (f == g.k_trace_smem) {
            f = fc = g.k_smem_lens;
            fname = "vcrt_trace_smem_lens";
        } else if (f == g.k_trace_cull_flat) {
            f = g.k_flat_lens;
            fc = g.k_flat_lens_cost;
            fname = "vcrt_trace_cull_flat_lens";
        } else if (f == g.k_trace_cull_flat_boxes) {
            f = g.k_flat_boxes_lens;
            fc = g.k_flat_boxes_lens_cost;
            fname = "vcrt_trace_cull_flat_boxes_lens";
        } else if (f == g.k_trace_cull_flat_global) {
            f = g.k_flat_global_lens;
            fc = g.k_flat_global_lens_cost;
            fname = "vcrt_trace_cull_flat_global_lens";
        } else {
            f = fc = nullptr;
        }
    }
    return KernelChoice{f, fs, base, fc, fname, block, lds, variant};
}

// The camera-ray lists of primary.cpp into the buffers a frame reads (TraceParams.prim_info,
// prim_ids, cam_rec): the two infos interleaved; the big groups' camera-relative records, then the
// sphere lists' pairs, then 12 zero floats. The buffers are kept and only grow (free_scene drops
// them), so a camera move allocates nothing once they are large enough.
VkResult install_camera_lists(const vcrt::CullTables& ct, const vcrt::PrimaryLists& pl,
                              const vcrt::PrimarySphereLists& sl) {
    // camera rays of a tile start from its quarter's lists (primary.cpp): the groups
    // for the main scan, the spheres for the camera fast trace; info interleaved
    std::vector<uint32_t> info(2 * pl.info.size());
    for (size_t e = 0; e < pl.info.size(); e++) {
        info[2 * e] = pl.info[e];
        info[2 * e + 1] = sl.info[e];
    }
    VCRT_TRY(g.d_prim_info.reserve(info.size()));
    VCRT_TRY(hipMemcpy(g.d_prim_info.data(), info.data(), sizeof(uint32_t) * info.size(),
                       hipMemcpyHostToDevice));
    VCRT_TRY(g.d_prim_ids.reserve(pl.ids.size() + 1));
    if (!pl.ids.empty())
        VCRT_TRY(hipMemcpy(g.d_prim_ids.data(), pl.ids.data(), sizeof(uint16_t) * pl.ids.size(),
                           hipMemcpyHostToDevice));
    // the camera fast trace's records: the big groups', then the sphere lists' pairs
    std::vector<float> crec;
    vcrt::build_camera_records(ct, camera_array().data(), crec);
    crec.resize(static_cast<size_t>(ct.nbig) * 16);
    crec.insert(crec.end(), sl.rec.begin(), sl.rec.end());
    crec.resize(crec.size() + 12, 0.0f);  // never empty
    VCRT_TRY(g.d_cam_rec.reserve(crec.size()));
    VCRT_TRY(hipMemcpy(g.d_cam_rec.data(), crec.data(), sizeof(float) * crec.size(),
                       hipMemcpyHostToDevice));
    g.prim_nids = pl.ids.size();
    g.prim_npairs = sl.rec.size() / 12;
    return VK_SUCCESS;
}

// The scene's tables on the host: vcrt_set_scene's, or after a device refit the host's
// restatement of them for the same grouping and the current spheres (equal bytes).
const vcrt::CullTables& current_tables() {
    if (g.h_ct_stale) {
        vcrt::tables_of_grouping(g.h_spheres.data(), static_cast<int32_t>(g.h_spheres.size()),
                                 g.h_ct);
        g.h_ct_stale = false;
    }
    return g.h_ct;
}

// The lists of the current scene and camera from the host builders, installed.
VkResult build_camera_lists_host() {
    const vcrt::CullTables& ct = current_tables();
    vcrt::PrimaryLists pl;
    vcrt::build_primary_lists(ct, camera_array().data(), g.desc.width, g.desc.height, g.desc.rank,
                              g.desc.world_size, pl);
    vcrt::PrimarySphereLists sl;
    vcrt::build_primary_sphere_lists(ct, g.h_spheres.data(), camera_array().data(), g.desc.width,
                                     g.desc.height, g.desc.rank, g.desc.world_size, sl);
    const VkResult r = install_camera_lists(ct, pl, sl);
    if (r != VK_SUCCESS) return r;
    // (the uploads ran on the null stream; the render stream does not wait for it)
    VCRT_TRY(hipStreamSynchronize(nullptr));
    return VK_SUCCESS;
}

// The same lists built on the device (camera_lists.hip) from the tables vcrt_set_scene uploaded,
// on the render stream: prepare, count, scan; the two totals come back (8 bytes) to size the
// buffers; fill. The per-camera scalars are QuarterWalker's (primary.cpp), evaluated here once.
VkResult build_camera_lists_device() {
    const std::array<float, 12> cam = camera_array();
    vcrt::CameraListParams p{};
    for (int i = 0; i < 12; i++) p.cam[i] = cam[i];
    const double* o = &p.cam[9];
    const double on = std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
    p.Q = (on + g.cmargin[0]) * (on + g.cmargin[0]) + g.cmargin[1];
    const double* du = &p.cam[3];
    const double* dv = &p.cam[6];
    const double ndu = std::sqrt(du[0] * du[0] + du[1] * du[1] + du[2] * du[2]);
    const double ndv = std::sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
    constexpr double kExtra = 1e-3;
    p.ex = kExtra / ndu;
    p.ey = kExtra / ndv;
    for (int a = 0; a < 3; a++) p.o[a] = cam[9 + a];
    p.n = 4u * g.local_tiles;
    p.ngroups = static_cast<uint32_t>(g.ncgroups);
    p.nnodes = p.ngroups / static_cast<uint32_t>(vcrt::kNodeGroups);
    p.ntops = (p.ngroups + 63u) / 64u;
    p.nbig = static_cast<uint32_t>(g.ncbig);
    p.nspheres = static_cast<uint32_t>(g.nspheres);
    p.rank = static_cast<uint32_t>(g.desc.rank);
    p.world = static_cast<uint32_t>(g.desc.world_size);
    p.tiles_x = g.tiles_x;
    p.ids_ok = p.ngroups <= 0xFFFFu ? 1u : 0u;
    p.ctop = reinterpret_cast<const float*>(g.d_ctop.data());
    p.cnode = reinterpret_cast<const float*>(g.d_cnode.data());
    p.cbound = reinterpret_cast<const float*>(g.d_cbound.data());
    p.cgroup = reinterpret_cast<const float*>(g.d_cgroup.data());
    p.center_radius = reinterpret_cast<const float*>(g.d_center_radius.data());
    const size_t nbox = static_cast<size_t>(p.ngroups) + p.nnodes + p.ntops;
    VCRT_TRY(g.d_cl_boxes.reserve(nbox * vcrt::kCamListBox));
    VCRT_TRY(g.d_cl_spheres.reserve(static_cast<size_t>(p.nspheres) * vcrt::kCamListBox));
    VCRT_TRY(g.d_cl_counts.reserve(4 * static_cast<size_t>(p.n) + 2));
    VCRT_TRY(g.h_cl_totals.reserve(2));
    for (Event& e : g.ev_cl) VCRT_TRY(e.create());
    p.boxes = g.d_cl_boxes.data();
    p.spheres = g.d_cl_spheres.data();
    p.counts = g.d_cl_counts.data();
    p.offsets = p.counts + 2 * static_cast<size_t>(p.n);
    p.totals = p.offsets + 2 * static_cast<size_t>(p.n);
    VCRT_TRY(g.d_prim_info.reserve(2 * static_cast<size_t>(p.n)));
    p.prim_info = g.d_prim_info.data();
    VCRT_TRY(hipEventRecord(g.ev_cl[0].get(), g.stream));
    const uint32_t quarter_blocks = (p.n + 255u) / 256u;
    VkResult r = launch(g.k_cl_prepare,
                        static_cast<uint32_t>(std::min<size_t>((nbox + p.nspheres + 255) / 256, 4096)),
                        256, 0, p);
    if (r != VK_SUCCESS) return r;
    if ((r = launch(g.k_cl_count, quarter_blocks, 256, 0, p)) != VK_SUCCESS) return r;
    if ((r = launch(g.k_cl_scan, 1, vcrt::kCamListScanThreads, 0, p)) != VK_SUCCESS) return r;
    uint32_t* totals = g.h_cl_totals.data();
    VCRT_TRY(hipMemcpyAsync(totals, p.totals, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    const size_t nids = totals[0], npairs = totals[1];
    VCRT_TRY(g.d_prim_ids.reserve(nids + 1));
    VCRT_TRY(g.d_cam_rec.reserve(static_cast<size_t>(p.nbig) * 16 + npairs * 12 + 12));
    p.prim_ids = g.d_prim_ids.data();
    p.cam_rec = g.d_cam_rec.data();
    const uint32_t fill_threads = std::max(std::max(p.n, p.nbig), 12u);
    if ((r = launch(g.k_cl_fill, (fill_threads + 255u) / 256u, 256, 0, p)) != VK_SUCCESS) return r;
    VCRT_TRY(hipEventRecord(g.ev_cl[1].get(), g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    float ms = 0.0f;
    VCRT_TRY(hipEventElapsedTime(&ms, g.ev_cl[0].get(), g.ev_cl[1].get()));
    g.cam_stats.lists_ms = ms;
    g.prim_nids = nids;
    g.prim_npairs = npairs;
    return VK_SUCCESS;
}

}  // namespace

// ---- what ray_passes.cpp uses too (declared in renderer_state.hpp) -----------------------------

namespace vcrt {

bool lens_on() { return g.desc.lens_radius > 0.0f; }

void make_jitter(uint64_t base, int n, float2* out) {
    for (int k = 0; k < n; k++) {
        const float i = static_cast<float>(base + k), i1 = static_cast<float>(base + k + 1);
        out[k].x = kJitterOffset + rand2(i, i);  // shader.comp:48
        out[k].y = kJitterOffset + rand2(i1, i1);
    }
}

std::array<float, 12> camera_array() {
    const f3 v[4] = {g.cam.pixel00, g.cam.delta_u, g.cam.delta_v, g.cam.center};
    std::array<float, 12> c{};
    for (int i = 0; i < 4; i++) {
        c[3 * i + 0] = v[i].x;
        c[3 * i + 1] = v[i].y;
        c[3 * i + 2] = v[i].z;
    }
    return c;
}

// The camera phase of the flat scans traces a fresh camera ray from its quarter's list when the
// ray is in the guarded range. Its origin is the camera centre, a frame constant, so that half of
// the guard (every |component| <= 2^30, in a bounded scene; also rejects NaN) is decided here: a
// frame that fails it gets no lists, and its camera rays take the main scan, which tests their
// origin itself.
bool lists_allowed(const std::array<float, 12>& cam) {
    return g.scene_bounded && std::fabs(cam[9]) <= 0x1p30f && std::fabs(cam[10]) <= 0x1p30f &&
           std::fabs(cam[11]) <= 0x1p30f;
}

Camera camera_of(int32_t width, int32_t height, const vcrt_camera& c) {
    return make_camera(width, height, mk(c.lookfrom[0], c.lookfrom[1], c.lookfrom[2]),
                       mk(c.lookat[0], c.lookat[1], c.lookat[2]), mk(c.vup[0], c.vup[1], c.vup[2]),
                       c.vfov, [](double x) { return std::tan(x); });
}

// The scene's part of a kernel's argument block: the scan tables, the shading rows, the margins
// and the flags' scene bits (frames and ray queries).
void scene_params(TraceParams& p) {
    p.geom = g.d_geom.data();
    p.center_radius = g.d_center_radius.data();
    p.shade = g.d_shade.data();
    p.material = g.d_material.data();
    p.cgroup = g.d_cgroup.data();
    p.cbound = g.d_cbound.data();
    p.cbound_nf = g.d_cbound_nf.data();
    p.cnode = g.d_cnode.data();
    p.cnode_nf = g.d_cnode_nf.data();
    p.ctop = g.d_ctop.data();
    p.ncgroups = g.ncgroups;
    p.nbig = g.ncbig;
    for (int k = 0; k < 4; k++) p.box_margin[k] = g.cmargin[k];
    p.slab[0] = g.cslab[0];
    p.slab[1] = g.cslab[1];
    p.fp_tab = g.d_fp_tab.data();
    for (int k = 0; k < 2; k++) {
        p.fp_x[k] = g.cfp_x[k];
        p.fp_z[k] = g.cfp_z[k];
        p.fp_y[k] = g.cfp_y[k];
    }
    p.fp_k2 = g.cfp_k2;
    p.fp_always = g.cfp_always;
    p.gf_tab = g.d_gf_tab.data();
    for (int k = 0; k < 2; k++) {
        p.gf_x[k] = g.cgf_x[k];
        p.gf_z[k] = g.cgf_z[k];
    }
    p.gf_k2 = g.cgf_k2;
    p.gf_n = g.cgf_n;
    for (int k = 0; k < 4; k++) p.gf_always[k] = g.cgf_always[k];
    p.nspheres = g.nspheres;
    p.flags = (g.scene_bounded ? kFlagSceneBounded : 0u) |
              (g.radii_safe ? kFlagRadiiSafe : 0u) |
              (g.ncgroups > 0 && g.cslab_on ? kFlagSlab : 0u);
    for (int j = 0; j < 13; j++) p.sin_c[j] = kSinC[j];
}

void frame_params(TraceParams& p, const float4* jitter, const float4* lens, int32_t spp,
                  int32_t max_depth) {
    scene_params(p);
    p.jitter = jitter;
    p.lens = lens;
    p.corner = g.d_corner.data();
    p.prim_info = g.d_prim_info.data();
    p.prim_ids = g.d_prim_ids.data();
    p.cam_rec = reinterpret_cast<const float4*>(g.d_cam_rec.data());
    p.width = g.desc.width;
    p.height = g.desc.height;
    p.spp = spp;
    p.max_depth = max_depth;
    p.rank = g.desc.rank;
    p.world = g.desc.world_size;
    p.tiles_x = g.tiles_x;
    p.local_tiles = g.local_tiles;
    const std::array<float, 12> cam = camera_array();
    for (int i = 0; i < 12; i++) p.cam[i] = cam[i];
    // (The group footprint keeps to the lists the scene has: a frame without them sends no
    // camera ray to a culled scan.)
    if (!lists_allowed(cam)) p.prim_info = nullptr;
}

VkResult jitter_tables(uint64_t base, uint32_t n, const JitterTables& t) {
    make_jitter(base, static_cast<int>(n), t.h_jitter);
    VCRT_TRY(hipMemcpyAsync(t.d_jitter_in, t.h_jitter, sizeof(float2) * n, hipMemcpyHostToDevice,
                            g.stream));
    if (t.d_lens) {  // the lens origins of the same sample indices: centre + offset_i
        for (uint32_t k = 0; k < n; k++) {
            const f3 o = add(g.cam.center, lens_offset(static_cast<uint32_t>(base + k),
                                                       g.desc.lens_radius, g.cam.u, g.cam.v));
            t.h_lens[k] = make_float4(o.x, o.y, o.z, 0.0f);
        }
        VCRT_TRY(hipMemcpyAsync(t.d_lens, t.h_lens, sizeof(float4) * n, hipMemcpyHostToDevice,
                                g.stream));
    }
    if (t.copied) VCRT_TRY(hipEventRecord(t.copied, g.stream));
    SetupJitterParams sp{};
    sp.jitter_in = t.d_jitter_in;
    sp.jitter = t.d_jitter;
    sp.nsamples = n;
    const std::array<float, 12> cam = camera_array();
    for (int i = 0; i < 12; i++) sp.cam[i] = cam[i];
    sp.corner = t.d_corner;
    sp.slots = g.total_pixels;
    sp.tiles_x = g.tiles_x;
    sp.rank = static_cast<uint32_t>(g.desc.rank);
    sp.world = static_cast<uint32_t>(g.desc.world_size);
    const uint64_t total = static_cast<uint64_t>(n) + (sp.corner ? sp.slots : 0u);
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((total + 255) / 256, 8192));
    return launch(g.k_setup_jitter, grid, 256, 0, sp);
}

}  // namespace vcrt

extern "C" {

vcrt_result vcrt_default_desc(vcrt_render_desc* d) {
    if (!d) return VCRT_ERROR_INITIALIZATION_FAILED;
    std::memset(d, 0, sizeof(*d));
    d->struct_size = sizeof(vcrt_render_desc);
    d->width = vcrt::kRefImageWidth;  // globals.glsl:16-17
    d->height = vcrt::kRefImageHeight;
    d->samples_per_pixel = vcrt::kRefSamplesPerPixel;  // globals.glsl:9-13 (#if 0 -> 1)
    d->max_depth = vcrt::kRefMaxRecursion;             // globals.glsl:14
    std::memcpy(d->camera.lookfrom, vcrt::kRefLookfrom, sizeof(d->camera.lookfrom));  // :21-24
    std::memcpy(d->camera.lookat, vcrt::kRefLookat, sizeof(d->camera.lookat));
    std::memcpy(d->camera.vup, vcrt::kRefVup, sizeof(d->camera.vup));
    d->camera.vfov = vcrt::kRefVfov;
    d->device = -1;
    d->rank = 0;
    d->world_size = 1;
    d->kernel_variant = VCRT_KERNEL_AUTO;
    return VCRT_SUCCESS;
}

int32_t vcrt_work_chunk(const vcrt_render_desc* desc) {
    vcrt_render_desc d;
    if (!read_desc(desc, d) || !desc_valid(d)) return VCRT_ERROR_INITIALIZATION_FAILED;
    return work_chunk(d);
}

int32_t vcrt_work_quantum(const vcrt_render_desc* desc) {
    vcrt_render_desc d;
    if (!read_desc(desc, d) || !desc_valid(d)) return VCRT_ERROR_INITIALIZATION_FAILED;
    return work_quantum(d);
}

int32_t vcrt_work_tail(const vcrt_render_desc* desc, int32_t* tail_chunk) {
    vcrt_render_desc d;
    if (!read_desc(desc, d) || !desc_valid(d) || !tail_chunk)
        return VCRT_ERROR_INITIALIZATION_FAILED;
    return work_tail(d, work_chunk(d), tail_chunk);
}

int32_t vcrt_pixel_scale_log2(float max_abs_quantum_sum) {
    const float e = std::fabs(max_abs_quantum_sum);
    uint32_t bits = 0;
    std::memcpy(&bits, &e, sizeof(bits));
    return vcrt::pixel_scale_log2(e >= 0x1p12f && std::isfinite(e) ? bits : 0u);
}

vcrt_result vcrt_begin(const vcrt_render_desc* desc) {
    vcrt_render_desc dv;
    if (!read_desc(desc, dv) || !desc_valid(dv)) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (dv.lens_radius > 0.0f) {
        // the thin lens has builds of the SMEM and flat scans only, and no stats builds
        const char* ds = std::getenv("VCRT_DEBUG_STATS");
        if (dv.kernel_variant == VCRT_KERNEL_LDS || dv.kernel_variant == VCRT_KERNEL_CULL ||
            dv.kernel_variant == VCRT_KERNEL_CULL_LANE || (ds && std::atoi(ds) == 1))
            return VCRT_ERROR_FEATURE_NOT_PRESENT;
    }
    if (g.begun) vcrt_end();
    g = RendererState{};
    g.desc = dv;
    g.begun = true;  // from here on vcrt_end() cleans up whatever was created

    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        vcrt_end();
        return VCRT_ERROR_INITIALIZATION_FAILED;
    }
    if (g.desc.device >= 0) {
        if (g.desc.device >= count || hipSetDevice(g.desc.device) != hipSuccess) {
            vcrt_end();
            return VCRT_ERROR_INITIALIZATION_FAILED;
        }
    }
    VkResult r = VK_SUCCESS;
    auto fail = [&](VkResult rr) {
        vcrt_end();
        return rr;
    };
    if ((r = to_vk(hipGetDevice(&g.device))) != VK_SUCCESS) return fail(r);
    hipDeviceProp_t prop;
    if ((r = to_vk(hipGetDeviceProperties(&prop, g.device))) != VK_SUCCESS) return fail(r);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(VCRT_ERROR_FEATURE_NOT_PRESENT);  // code object is gfx950-only
    g.num_cus = prop.multiProcessorCount;
    g.max_lds = prop.sharedMemPerBlock;
    g.lds_per_cu = static_cast<uint32_t>(prop.maxSharedMemoryPerMultiProcessor);
    if ((r = to_vk(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking))) != VK_SUCCESS)
        return fail(r);
    for (Event* e : {&g.ev_start, &g.ev_stop, &g.ev_resolve})
        if ((r = to_vk(e->create())) != VK_SUCCESS) return fail(r);
    if ((r = load_code_object(g.desc.code_object_path)) != VK_SUCCESS) return fail(r);
    g.desc.code_object_path = nullptr;  // not owned
    if (lens_on() && !lens_kernels_bound()) return fail(VCRT_ERROR_FEATURE_NOT_PRESENT);

    // Camera (shader.comp:18-39): uniform per dispatch, computed once here.
    const vcrt_camera& c = g.desc.camera;
    g.cam = vcrt::make_camera(g.desc.width, g.desc.height,
                              vcrt::mk(c.lookfrom[0], c.lookfrom[1], c.lookfrom[2]),
                              vcrt::mk(c.lookat[0], c.lookat[1], c.lookat[2]),
                              vcrt::mk(c.vup[0], c.vup[1], c.vup[2]), c.vfov,
                              [](double x) { return std::tan(x); });
    // Jitter (shader.comp:48) depends only on the sample index: one table per frame config.
    const int spp = g.desc.samples_per_pixel;
    // (the state is fresh, so every reserve here and below allocates exactly what it names)
    if ((r = to_vk(g.d_jitter_in.reserve(spp))) != VK_SUCCESS) return fail(r);
    for (int k = 0; k < 2; k++) {
        if ((r = to_vk(g.h_jitter[k].reserve(spp))) != VK_SUCCESS) return fail(r);
        if ((r = to_vk(g.ev_jitter[k].create(hipEventDisableTiming))) != VK_SUCCESS)
            return fail(r);
    }
    if ((r = to_vk(g.d_jitter.reserve(spp))) != VK_SUCCESS) return fail(r);
    if (lens_on()) {  // the lens origins, a table like the jitter's
        for (int k = 0; k < 2; k++)
            if ((r = to_vk(g.h_lens[k].reserve(spp))) != VK_SUCCESS) return fail(r);
        if ((r = to_vk(g.d_lens.reserve(spp))) != VK_SUCCESS) return fail(r);
    }
    {
        std::vector<float> th(255);
        srgb_thresholds(th.data());
        if ((r = to_vk(upload(g.d_srgb_thresholds, th))) != VK_SUCCESS) return fail(r);
    }

    // Frame sharding: 8x8 tiles, (tx, ty) to rank (tx + ty) % world (DESIGN.md "Multi-GPU").
    g.tiles_x = static_cast<uint32_t>((g.desc.width + 7) / 8);
    g.local_tiles = tiles_for_rank(g.desc.width, g.desc.height, g.desc.world_size, g.desc.rank);
    // a lane keeps its item's slot in the low kRingQBits bits of one register (the ring entry
    // above it): at most 2^26 slots per rank (8192 x 8192 on one GPU)
    if (static_cast<uint64_t>(g.local_tiles) * 64u > (uint64_t{1} << vcrt::kRingQBits))
        return fail(VCRT_ERROR_FORMAT_NOT_SUPPORTED);
    g.local_elems = g.desc.world_size == 1
                        ? static_cast<uint32_t>(g.desc.width) * static_cast<uint32_t>(g.desc.height)
                        : g.local_tiles * 64u;
    g.fb_bytes = static_cast<size_t>(g.local_elems) * sizeof(float4);
    for (int32_t rr = 0; rr < g.desc.world_size; rr++)
        g.pad_tiles = std::max(g.pad_tiles, tiles_for_rank(g.desc.width, g.desc.height,
                                                           g.desc.world_size, rr));
    for (uint32_t lt = 0; lt < g.local_tiles; lt++) {
        uint32_t tx, ty;
        vcrt::tile_of(lt, static_cast<uint32_t>(g.desc.rank),
                      static_cast<uint32_t>(g.desc.world_size), g.tiles_x, &tx, &ty);
        g.local_pixels += std::min<uint64_t>(8, g.desc.width - 8 * tx) *
                          std::min<uint64_t>(8, g.desc.height - 8 * ty);
    }
    // sharded: padded to the largest rank, the size every rank sends -- also a rank that owns
    // no tile (a frame of fewer tiles than ranks) sends that many zero bytes to the gather
    const size_t own = g.desc.world_size == 1 ? g.fb_bytes
                                              : static_cast<size_t>(g.pad_tiles) * 64 * 16;
    if (own) {
        if ((r = to_vk(g.d_fb_own.reserve(own / sizeof(float4)))) != VK_SUCCESS) return fail(r);
        if ((r = to_vk(hipMemsetAsync(g.d_fb_own.data(), 0, own, g.stream))) != VK_SUCCESS)
            return fail(r);
    }
    g.d_fb = g.d_fb_own.data();
    // Work decomposition: (local tile, chunk of K samples) items holding whole quanta; a pixel's
    // quantum sums are combined exactly (vcrt_math.h "Accumulation"), at most kAccumMaxChunks.
    g.total_pixels = g.local_tiles * 64u;  // local element slots incl. partial-tile padding
    // the camera-ray tables: the jitter terms and the local slots' pixel corners
    if ((r = to_vk(g.d_corner.reserve(g.total_pixels))) != VK_SUCCESS) return fail(r);
    if ((r = setup_jitter(0, g.total_pixels != 0)) != VK_SUCCESS) return fail(r);
    g.quantum = work_quantum(g.desc);
    if ((spp + g.quantum - 1) / g.quantum > vcrt::kAccumMaxChunks)
        return fail(VCRT_ERROR_FORMAT_NOT_SUPPORTED);
    g.chunk = work_chunk(g.desc);
    g.cost_partition = cost_partition(g.desc);
    {
        const int32_t t = work_tail(g.desc, g.chunk, &g.tail_chunk);
        g.tail_start = spp - t;
        g.tail_nchunks = t > 0 ? (t + g.tail_chunk - 1) / g.tail_chunk : 0;
    }
    g.nchunks = (g.tail_start + g.chunk - 1) / g.chunk;
    g.nch_magic[0] = division_magic(static_cast<uint32_t>(g.nchunks));
    g.nch_magic[1] = division_magic(static_cast<uint32_t>(g.tail_nchunks));
    if (g.nchunks >= 0x10000 || g.tail_nchunks >= 0x10000)  // the kernel's 16-bit chunk field
        return fail(VCRT_ERROR_FORMAT_NOT_SUPPORTED);
    // one quantum covers the pixel: the lane divides its fp32 sum (the reference's arithmetic)
    g.direct = g.quantum >= spp && !g.desc.progressive;
    {
        const uint64_t items = static_cast<uint64_t>(g.total_pixels) *
                               static_cast<uint64_t>(g.nchunks + g.tail_nchunks);
        if (items >= (uint64_t{1} << 31)) return fail(VCRT_ERROR_FORMAT_NOT_SUPPORTED);
        g.total_items = static_cast<uint32_t>(items);
    }
    if (!g.direct && g.total_pixels) {  // 32 B per pixel, whatever the spp
        const size_t bytes = 32u * static_cast<size_t>(g.total_pixels);
        if ((r = to_vk(g.d_accum.reserve(bytes / sizeof(double)))) != VK_SUCCESS) return fail(r);
        if ((r = to_vk(hipMemsetAsync(g.d_accum.data(), 0, bytes, g.stream))) != VK_SUCCESS)
            return fail(r);
        g.accum_clean = true;
        const size_t eb = sizeof(uint32_t) * static_cast<size_t>(g.total_pixels);
        if ((r = to_vk(g.d_pixel_emax.reserve(g.total_pixels))) != VK_SUCCESS) return fail(r);
        if ((r = to_vk(hipMemsetAsync(g.d_pixel_emax.data(), 0, eb, g.stream))) != VK_SUCCESS)
            return fail(r);
    }
    if ((r = to_vk(g.d_counters.reserve(kCounterBytes / 8))) != VK_SUCCESS) return fail(r);
    if ((r = to_vk(g.h_counters.reserve(4))) != VK_SUCCESS) return fail(r);
    if (const char* e = std::getenv("VCRT_DEBUG_STATS")) g.debug_stats = std::atoi(e);
    if (const char* e = std::getenv("VCRT_PRIMARY_LISTS")) g.primary_lists = std::atoi(e) != 0;
    if (const char* e = std::getenv("VCRT_FEATURE_LISTS")) g.feature_lists = std::atoi(e) != 0;
    if (const char* e = std::getenv("VCRT_CULL_LANE_TABLES"))
        g.cull_lane_tables = std::strcmp(e, "lds") == 0      ? 1
                             : std::strcmp(e, "global") == 0 ? 2
                             : std::strcmp(e, "boxes") == 0  ? 3
                                                             : 0;
    // Blocks run from the last local tile to the first: the bottom of the frame (ground and
    // spheres, many bounces) first, the sky last, which shortens the drain at the end of the
    // queue (N = 8: 34.8 -> 33.8 ms per rank). VCRT_WORK_ORDER=forward restores top-down.
    g.work_flags |= vcrt::kFlagReverseOrder;
    if (const char* e = std::getenv("VCRT_WORK_ORDER"))
        if (std::strcmp(e, "forward") == 0) g.work_flags &= ~vcrt::kFlagReverseOrder;
    if (const char* e = std::getenv("VCRT_WORK_ORDER"))
        g.cost_order = std::strcmp(e, "cost") == 0 ? 1 : 0;  // any other value: static order
    // A block's 64 items are all the chunks of 64 / nchunks pixels (chunk-minor): the camera
    // rays of a wave then come from a few pixels (+2.8% at the C4 workload against one chunk of
    // a whole tile, same bits). VCRT_ITEM_ORDER=tile restores the tile-wide blocks.
    g.work_flags |= vcrt::kFlagChunkMinor;
    if (const char* e = std::getenv("VCRT_ITEM_ORDER"))
        if (std::strcmp(e, "tile") == 0) g.work_flags &= ~vcrt::kFlagChunkMinor;
    if (const char* e = std::getenv("VCRT_STAGE_TABLES")) g.stage_tables = std::atoi(e) != 0;
    if (const char* e = std::getenv("VCRT_FLAT_BLOCK")) {  // the LDS flat scan's group size
        const int v = std::atoi(e) / 64 * 64;
        g.flat_block = v <= 0 ? 0 : std::min(1024, v);
    }
    if (const char* e = std::getenv("VCRT_FETCH_MIN"))
        g.fetch_min = static_cast<uint32_t>(std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("VCRT_FETCH_WAIT"))
        g.fetch_wait = static_cast<uint32_t>(std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("VCRT_MAX_BLOCKS_PER_CU"))  // cap on the occupancy rule
        g.max_blocks_per_cu = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("VCRT_ACCUM_RING")) {  // 0: off; n > 1: at most n entries
        // (clamped to kRingMaxEntries: a lane keeps its entry + 1 in the top bits of its pixel
        // index, so a larger ring would silently stop serving most pixels)
        g.accum_ring = std::atoi(e) != 0;
        if (std::atoi(e) > 1)
            g.ring_max = std::min<uint32_t>(static_cast<uint32_t>(std::atoi(e)),
                                            vcrt::kRingMaxEntries);
    }
    if (g.debug_stats &&
        (r = to_vk(g.d_debug.reserve(sizeof(g.stats.debug) / sizeof(g.stats.debug[0])))) !=
            VK_SUCCESS)
        return fail(r);

    // The reference's world[] is compiled in; default to the same final scene.
    std::vector<vcrt_sphere> world;
    vcrt::builtin_scene(VCRT_SCENE_FINAL, world);
    if ((r = vcrt_set_scene(world.data(), static_cast<int32_t>(world.size()))) != VK_SUCCESS)
        return fail(r);
    g.stats.local_tiles = static_cast<int32_t>(g.local_tiles);
    g.stats.accumulate_chunk = g.chunk;
    g.stats.accumulate_quantum = g.quantum;
    g.stats.accumulate_tail = spp - g.tail_start;
    g.stats.accumulate_tail_chunk = g.tail_nchunks > 0 ? g.tail_chunk : 0;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_set_scene(const vcrt_sphere* spheres, int32_t count) {
    if (!g.begun) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (count < 0 || (count > 0 && !spheres)) return VCRT_ERROR_INITIALIZATION_FAILED;
    // Scan table: groups of four spheres in pair-SoA form
    //   (cx0,cx1,cy0,cy1) (cz0,cz1,r0²,r1²) (cx2,cx3,cy2,cy3) (cz2,cz3,r2²,r3²),
    // r² = radius*radius as hit_sphere computes it (functions.glsl:18). The last group is
    // padded with far-away empty spheres and one extra group follows for the prefetch; the
    // kernel never accepts a padding index anyway.
    const std::vector<float> table = linear_table(spheres, count);
    std::vector<float4> cr, shade, mat;
    sphere_rows(spheres, count, cr, shade, mat);
    vcrt::CullTables ct;
    vcrt::build_cull_tables(spheres, count, ct);
    (void)hipStreamSynchronize(g.stream);
    free_scene();
    if (ct.ngroups > 0) {
        VCRT_TRY(upload(g.d_cgroup, group_records(ct)));
        VCRT_TRY(upload(g.d_cbound, ct.bound));
        VCRT_TRY(upload(g.d_cnode, ct.node));
        VCRT_TRY(upload(g.d_ctop, ct.top));
        // near/far layout of the group boxes for the flat scan (vcrt_kernel_abi.h, cbound_nf)
        VCRT_TRY(upload(g.d_cbound_nf, near_far(ct.bound)));
        VCRT_TRY(upload(g.d_cnode_nf, node_near_far(ct)));
        g.ncgroups = ct.ngroups;
        g.ncbig = ct.nbig;
        std::memcpy(g.cmargin, ct.margin, sizeof(ct.margin));
        g.cslab_on = ct.slab;
        g.cslab[0] = ct.slab_lohi[0];
        g.cslab[1] = ct.slab_lohi[1];
        {
            // footprint tables: 16-bit masks up to 16 nodes, as the kernel's LDS image holds them
            VCRT_TRY(upload(g.d_fp_tab, pack_footprint(ct)));
            std::memcpy(g.cfp_x, ct.fp_x, sizeof(g.cfp_x));
            std::memcpy(g.cfp_z, ct.fp_z, sizeof(g.cfp_z));
            std::memcpy(g.cfp_y, ct.fp_y, sizeof(g.cfp_y));
            g.cfp_k2 = ct.fp_k2;
            g.cfp_always = ct.fp_always;
        }
        if (ct.gf_cells > 0) {
            // group-level footprint tables (fact (5g)): in the LDS image they take the place of
            // the group boxes and the node tables
            static_assert(vcrt::kGroupFootMaxGroups ==
                              static_cast<uint32_t>(vcrt::kGroupFootprintMaxGroups),
                          "group footprint limit");
            if (static_cast<uint32_t>(ct.gf_cells) != vcrt::group_foot_cells(ct.ngroups))
                return VCRT_ERROR_INITIALIZATION_FAILED;
            // behind the four tables their zero row (tracer.hip group_foot_mask; cell 4 gf_n of
            // the LDS image, select_kernel's tab_lds_flat): it must lie ahead of the records
            const size_t tab_bytes = sizeof(uint32_t) * ct.gf_tab.size();
            if (tab_bytes != 64u * static_cast<size_t>(ct.gf_cells) ||
                tab_bytes + 16u > 16u * (static_cast<size_t>(ct.ngroups) / 8u * 21u +
                                         vcrt::group_foot_zero_pad(ct.ngroups)) +
                                      vcrt::foot_lds_bytes(ct.ngroups))
                return VCRT_ERROR_INITIALIZATION_FAILED;
            VCRT_TRY(g.d_gf_tab.reserve(tab_bytes / sizeof(uint4) + 1));
            VCRT_TRY(hipMemcpy(g.d_gf_tab.data(), ct.gf_tab.data(), tab_bytes,
                               hipMemcpyHostToDevice));
            VCRT_TRY(hipMemset(reinterpret_cast<char*>(g.d_gf_tab.data()) + tab_bytes, 0, 16u));
            std::memcpy(g.cgf_x, ct.gf_x, sizeof(g.cgf_x));
            std::memcpy(g.cgf_z, ct.gf_z, sizeof(g.cgf_z));
            std::memcpy(g.cgf_always, ct.gf_always, sizeof(g.cgf_always));
            g.cgf_k2 = ct.gf_k2;
            g.cgf_n = static_cast<uint32_t>(ct.gf_cells);
            g.cgf_ok = ct.gf_ok;
        }
        // (not for a lens: its camera rays do not share an origin, so they have no lists, no
        // camera-relative records and, for want of the lists, no group-level footprint)
        if (g.primary_lists && g.local_tiles > 0 && !lens_on()) {
            // camera rays of a tile start from its quarter's lists (primary.cpp): the groups
            // for the main scan, the spheres for the camera fast trace; info interleaved
            vcrt::PrimaryLists pl;
            vcrt::build_primary_lists(ct, camera_array().data(), g.desc.width, g.desc.height,
                                      g.desc.rank, g.desc.world_size, pl);
            vcrt::PrimarySphereLists sl;
            vcrt::build_primary_sphere_lists(ct, spheres, camera_array().data(), g.desc.width,
                                             g.desc.height, g.desc.rank, g.desc.world_size, sl);
            const VkResult ru = install_camera_lists(ct, pl, sl);
            if (ru != VK_SUCCESS) return ru;
        }
    }
    VCRT_TRY(upload(g.d_geom, table));
    if (count > 0) {
        VCRT_TRY(upload(g.d_center_radius, cr));
        VCRT_TRY(upload(g.d_shade, shade));
        VCRT_TRY(upload(g.d_material, mat));
    }
    // (the uploads above ran on the null stream; the render stream does not wait for it)
    VCRT_TRY(hipStreamSynchronize(nullptr));
    g.nspheres = count;
    g.stats.nspheres = count;
    if (spheres != g.h_spheres.data()) g.h_spheres.assign(spheres, spheres + count);
    g.h_ct = std::move(ct);
    g.h_ct_stale = false;
    if (g.desc.progressive && g.accumulated > 0) {
        // a new scene restarts progressive accumulation at sample 0: the jitter table holds
        // the last frame's sample indices
        const VkResult rj = setup_jitter(0);
        if (rj != VK_SUCCESS) return rj;
    }
    g.accumulated = 0;
    g.order_key = 0;    // and its cost order is measured again
    VCRT_TRY(reset_sums());
    g.scene_bounded = values_bounded(spheres, count);
    g.radii_safe = values_radii_safe(spheres, count);
    g.stage.pName = select_kernel().name;  // the entry point draws of this scene dispatch
    return VCRT_SUCCESS;
}

// Cost order (vcrt_draw_next_frame): at most this many items per lane of the persistent grid
// make a frame drain-bound (C2: 3.7; C3, C4 on one GPU: ~100; C4 8-way shards: ~50).
constexpr uint64_t kCostOrderItemsPerLane = 8;
// Waves per SIMD of such frames (C2, measured round 5: 0.792 ms at 6 waves, 0.763-0.769 at 5,
// 0.773 at 4, with the cost order; 0.829 / 0.797 without it).
constexpr uint32_t kDrainWavesPerSimd = 5;

// The configuration a measured order belongs to: kernel, grid and partition (a new scene or
// vcrt_begin resets it through order_key = 0).
uint64_t order_key_of(hipFunction_t f, uint32_t grid, uint32_t total_blocks) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    mix(reinterpret_cast<uintptr_t>(f));
    mix(grid);
    mix(total_blocks);
    mix(static_cast<uint64_t>(g.nchunks));
    mix(static_cast<uint64_t>(g.tail_nchunks));
    mix(g.local_tiles);
    return h | 1u;
}

// From the pixels' segment counts of the frame just rendered: every block (head and tail
// together) by decreasing cost of its items, longest first (the makespan heuristic), so that the
// items still running when the queue drains are the shortest: the tail's items of cheap pixels.
// A block's item cost is the mean segment count of the pixels its 64 chunk-minor items belong to
// (item i of tile lt's part with n chunks per pixel: slot i / n) times the part's samples per
// item; ties in the static order (head, then tail, each bottom-up: the highest block first).
VkResult build_block_order(uint32_t total_blocks) {
    std::vector<uint32_t> cost(g.total_pixels);
    VCRT_TRY(hipMemcpy(cost.data(), g.d_pixel_cost.data(), cost.size() * sizeof(uint32_t),
                       hipMemcpyDeviceToHost));
    std::vector<uint32_t> order(total_blocks);
    std::vector<uint64_t> bc(total_blocks, 0);
    const uint32_t head = g.local_tiles * static_cast<uint32_t>(g.nchunks);
    auto part = [&](uint32_t base, uint32_t nblocks, uint32_t nch, uint32_t samples) {
        for (uint32_t b = 0; b < nblocks; b++) {
            const uint32_t lt = b / nch, c = b - lt * nch;
            // chunk-minor: slots (64 c) / nch .. (64 c + 63) / nch; tile-wide blocks
            // (VCRT_ITEM_ORDER=tile): one chunk of all 64 slots
            const bool cm = (g.work_flags & vcrt::kFlagChunkMinor) != 0u;
            const uint32_t s0 = cm ? (64u * c) / nch : 0u;
            const uint32_t s1 = cm ? std::min((64u * c + 63u) / nch, 63u) : 63u;
            uint64_t sum = 0;
            for (uint32_t sl = s0; sl <= s1; sl++) sum += cost[lt * 64u + sl];
            bc[base + b] = sum * samples * 64u / (s1 - s0 + 1u);
        }
    };
    if (head > 0)
        part(0, head, static_cast<uint32_t>(g.nchunks), static_cast<uint32_t>(g.chunk));
    if (total_blocks > head)
        part(head, total_blocks - head, static_cast<uint32_t>(g.tail_nchunks),
             static_cast<uint32_t>(g.tail_chunk));
    uint32_t k = 0;
    for (uint32_t b = head; b-- > 0;) order[k++] = b;
    for (uint32_t b = total_blocks; b-- > head;) order[k++] = b;
    std::stable_sort(order.begin(), order.end(),
                     [&bc](uint32_t x, uint32_t y) { return bc[x] > bc[y]; });
    VCRT_TRY(g.d_block_order.reserve(total_blocks));
    VCRT_TRY(hipMemcpy(g.d_block_order.data(), order.data(), total_blocks * sizeof(uint32_t),
                       hipMemcpyHostToDevice));
    VCRT_TRY(hipStreamSynchronize(nullptr));  // before the render stream's next frame reads it
    return VK_SUCCESS;
}

// One render of the frame's samples (the tracer kernel and, when the pixels sum quanta, the
// resolve pass) on the render stream, waited for; *outlier_max receives the float bits of the
// largest |quantum sum| that did not fit its pixel's scale (0: none; vcrt_math.h
// "Accumulation").
static VkResult trace_frame(uint64_t spp_total, uint32_t* outlier_max) {
    const uint32_t pixels = g.total_pixels;
    vcrt::TraceParams p{};
    vcrt::frame_params(p, g.d_jitter.data(), g.d_lens.data(), g.desc.samples_per_pixel,
                       g.desc.max_depth);
    p.out = g.d_fb;
    p.accum = g.d_accum.data();
    unsigned long long* const counters64 = g.d_counters.data();  // (the layout: kCounterBytes)
    p.work = reinterpret_cast<uint32_t*>(counters64 + 256 / 8);
    p.segments = counters64 + 1;
    p.debug = g.d_debug.data();
    p.work_done = counters64 + 2;
    p.total_items = g.total_items;
    p.chunk = g.chunk;
    p.quantum_mask = static_cast<uint32_t>(g.quantum - 1);
    p.nchunks = g.nchunks;
    p.tail_start = g.tail_start;
    p.tail_chunk = g.tail_chunk;
    p.tail_nchunks = g.tail_nchunks;
    p.blocks_head = g.local_tiles * static_cast<uint32_t>(g.nchunks);
    p.flags |= g.work_flags | (g.direct ? vcrt::kFlagDirect : 0u) |
              (g.pixel_scale ? vcrt::kFlagPixelScale : 0u) |
              (static_cast<uint32_t>(g.accum_log2 + vcrt::kFlagScaleBias)
               << vcrt::kFlagScaleShift);
    // the group-level footprint (fact (5g)) takes the node level's place when the scene allows
    // it (CullTables::gf_ok) and the camera rays have their lists: without them camera rays
    // cross the scan on long grazing stretches, where a rectangle is loose
    if (g.cgf_ok && g.d_gf_tab.data() != nullptr && g.d_prim_info.data() != nullptr)
        p.flags |= vcrt::kFlagGroupFoot;
    // outlier quanta (vcrt_math.h "Accumulation"); the kernel's quantizing retire writes them
    p.pixel_emax = g.d_pixel_emax.data();
    p.outlier_max = reinterpret_cast<uint32_t*>(counters64);  // u32 at 0 (zeroed every launch)
    if (!g.direct && (p.pixel_emax == nullptr || g.d_accum.data() == nullptr))
        return VK_ERROR_INITIALIZATION_FAILED;
    p.spp_total = static_cast<float>(spp_total);
    p.region = nullptr;
    p.nch_magic[0] = g.nch_magic[0];
    p.nch_magic[1] = g.nch_magic[1];
    const KernelChoice kc = select_kernel();
    hipFunction_t f = g.debug_stats == 1 ? kc.stats : kc.f;
    if (f == nullptr) return VK_ERROR_FEATURE_NOT_PRESENT;  // (a lens, no lens kernels loaded)
    // Deferred fetches (tracer.hip, the flat scans): the LDS-table flat scan waits until 4 lanes
    // need an item (at most one iteration): C3 -0.6 % kernel time (its 16 items per pixel make
    // the fetch frequent), C4 and the 8-way shards within 0.1 %, same bits; the global-table and
    // boxes-in-LDS scans fetch at once (C5 +0.6 % with it). profiles/r06_ab_log.md. Swept again
    // on round 14's scan (profiles/r14_ab_log.md): fetching at once costs C4 0.3-0.5 ms and C3
    // 0.15-0.2 ms, and no other rule is ahead of this one by more than the spread.
    const bool lds_flat = kc.base == g.k_trace_cull_flat;
    p.fetch_min = g.fetch_min > 0u ? g.fetch_min : (lds_flat ? 4u : 1u);
    p.fetch_wait = g.fetch_min > 0u ? g.fetch_wait : (lds_flat ? 1u : 0u);
    const uint32_t block = kc.block;
    uint32_t lds = kc.lds;
    // the linear SMEM scan of a small scene stages its shading and jitter tables in LDS
    // (TraceParams.stage_*): C2 (4 spheres, 64 spp) is latency-bound on those reads
    p.stage_spheres = 0u;
    p.stage_spp = 0u;
    if (kc.base == g.k_trace_smem && g.nspheres > 0 && g.stage_tables) {
        // in 64 bits: 16 * spp wraps 32 bits for spp >= 2^28; a lens renderer
        // stages its origins after the jitter (16 B more per sample)
        const uint64_t bytes = 48ull * static_cast<uint64_t>(g.nspheres) +
                               (lens_on() ? 32ull : 16ull) *
                                   static_cast<uint64_t>(g.desc.samples_per_pixel);
        if (bytes <= kStageMaxBytes) {
            p.stage_spheres = static_cast<uint32_t>(g.nspheres);
            p.stage_spp = static_cast<uint32_t>(g.desc.samples_per_pixel);
            lds = static_cast<uint32_t>((bytes + 15u) & ~15ull);
        }
    }
    const int variant = kc.variant;
    // the stage names the entry point this draw dispatches (Shader.cpp:89 names "main")
    g.stage.pName = kc.name;
    std::snprintf(g.stats.kernel, sizeof(g.stats.kernel), "%s%s", kc.name,
                  g.debug_stats == 1 ? "_stats" : "");
    int per_cu = g.desc.blocks_per_cu;
    if (per_cu <= 0) {
        per_cu = 0;
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, block, lds) !=
                hipSuccess ||
            per_cu <= 0)
            per_cu = 1;
        if (g.max_blocks_per_cu > 0) per_cu = std::min(per_cu, g.max_blocks_per_cu);
    }
    // Cost order. When the frame gives each lane of the persistent grid few items, its end
    // is set by the last expensive items to start (an item's segments run one per wave
    // iteration: a glass pixel's 16-sample item at depth 8 is ~100 iterations), not by the
    // work. Then the first frame of a configuration counts each pixel's segments
    // (TraceParams.pixel_cost), and later frames hand out the blocks longest items first
    // (TraceParams.block_order, build_block_order); such frames also run at most kDrainWavesPerSimd
    // waves per SIMD, so that the waves holding the last items advance faster. Only the
    // schedule changes: the image depends on the quantum alone. Automatic for the linear
    // scans' frames with few items per lane (C2), and for the cost partition (default_chunk:
    // the 4- and 8-way shards of C4, where the flat scans launch their cost-order builds).
    // Elsewhere the flat scans' static bottom-up order is already roughly cost-ordered (sky
    // last) and keeps neighbouring blocks together: the cost order on their own partitions
    // measured slower (C4 -0.5%, C3 -1.1%, 8-way shards at K = 16 + 128 x 4 -4%;
    // profiles/r05_ab_log.md).
    const uint32_t total_blocks =
        g.local_tiles * static_cast<uint32_t>(g.nchunks + g.tail_nchunks);
    const bool cost_mode =
        g.debug_stats != 1 && total_blocks > 0 && kc.cost != nullptr &&
        (g.cost_order == 1 ||
         (g.cost_order < 0 &&
          (g.cost_partition ||
           (kc.cost == kc.f &&  // (the linear scans)
            static_cast<uint64_t>(g.total_items) <
                kCostOrderItemsPerLane * static_cast<uint64_t>(per_cu) * g.num_cus * block))));
    if (cost_mode && kc.cost != kc.f) {  // the flat scans' cost-order build
        f = kc.cost;
        std::snprintf(g.stats.kernel, sizeof(g.stats.kernel), "%s_cost", kc.name);
    }
    if (cost_mode && g.desc.blocks_per_cu <= 0 && g.max_blocks_per_cu <= 0)
        per_cu = std::min(per_cu, std::max(1, static_cast<int>(kDrainWavesPerSimd * 4u * 64u /
                                                               block)));
    // The accumulation ring (tracer.hip RingEntry): the LDS the workgroups leave free at
    // this occupancy, up to 63 entries of 32 B per wave, when the frame sums chunk sums
    // (not one chunk per pixel), its blocks are chunk-minor and its pixel indices leave the
    // top bits for the entry. The occupancy must not drop for it.
    p.ring_off = 0u;
    p.ring_n = 0u;
    uint32_t lds_launch = lds;
    if (g.accum_ring && !g.direct && (g.work_flags & vcrt::kFlagChunkMinor) != 0u &&
        static_cast<uint64_t>(g.local_tiles) * 64u <= (uint64_t{1} << vcrt::kRingQBits) &&
        g.lds_per_cu > 0 && g.desc.blocks_per_cu <= 0) {
        const uint32_t waves = block / 64u;
        const uint32_t off = (lds + 15u) & ~15u;
        // usable LDS per CU: measured, five 256-thread workgroups of 32512 B ran four per
        // CU (-11% at C4) while 32000 B ran five, although 5 x 32512 < 160 KiB and the
        // occupancy query allows them: budget 160000 B per CU
        const uint32_t per_wg = std::min<uint32_t>(g.lds_per_cu, 160000u) /
                                static_cast<uint32_t>(per_cu);
        uint32_t n = per_wg > off ? std::min<uint32_t>(g.ring_max,
                                                        (per_wg - off) / (32u * waves))
                                  : 0u;
        for (; n >= 8u; n -= 4u) {
            int occ = 0;
            if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(
                    &occ, f, block, off + 32u * n * waves) == hipSuccess &&
                occ >= per_cu)
                break;
        }
        if (n >= 8u) {
            p.ring_off = off;
            p.ring_n = n;
            lds_launch = off + 32u * n * waves;
        }
    }
    g.stats.ring_entries = static_cast<int32_t>(p.ring_n);
    const uint32_t grid = static_cast<uint32_t>(per_cu) * static_cast<uint32_t>(g.num_cus);
    const uint64_t key = cost_mode ? order_key_of(kc.f, grid, total_blocks) : 0;
    bool measure = false;
    p.pixel_cost = nullptr;
    p.block_order = nullptr;
    if (cost_mode && key == g.order_key) {
        p.block_order = g.d_block_order.data();
        p.flags &= ~vcrt::kFlagReverseOrder;  // the order is the whole hand-out sequence
    } else if (cost_mode) {
        VCRT_TRY(g.d_pixel_cost.reserve(pixels));
        VCRT_TRY(hipMemsetAsync(g.d_pixel_cost.data(), 0, pixels * sizeof(uint32_t), g.stream));
        p.pixel_cost = g.d_pixel_cost.data();
        measure = true;
    }
    g.stats.cost_order = p.block_order != nullptr ? 1 : 0;
    if (!g.counters_clean) VCRT_TRY(hipMemsetAsync(counters64, 0, kCounterBytes, g.stream));
    g.counters_clean = false;  // until this frame's resolve has read and zeroed them
    if (g.debug_stats == 1) {  // the stats kernels' region counters, one row per wave
        const size_t words = static_cast<size_t>(grid) * (block / 64u) * kRegionCount;
        VCRT_TRY(g.d_region.reserve(words));
        VCRT_TRY(hipMemsetAsync(g.d_region.data(), 0, words * sizeof(uint32_t), g.stream));
        p.region = g.d_region.data();
    }
    if (!g.direct && !g.desc.progressive && !g.accum_clean)  // every frame sums from zero
        VCRT_TRY(hipMemsetAsync(g.d_accum.data(), 0, 32u * static_cast<size_t>(pixels), g.stream));
    if (!g.direct) g.accum_clean = false;  // until this frame's resolve zeroes it
    if (g.debug_stats) {
        unsigned long long init[128] = {0, 0, 0, 0, 0, ~0ull};
        if (g.debug_stats == 2) init[9] = init[10] = ~0ull;  // wave times: minima
        VCRT_TRY(hipMemcpyAsync(g.d_debug.data(), init, sizeof(init), hipMemcpyHostToDevice,
                                g.stream));
    }
    VCRT_TRY(hipEventRecord(g.ev_start.get(), g.stream));
    VkResult r = launch(f, grid, block, lds_launch, p);
    if (r != VK_SUCCESS) return r;
    VCRT_TRY(hipEventRecord(g.ev_stop.get(), g.stream));
    bool resolved = false;
    if (!g.direct) {
        vcrt::ResolveParams rp{g.d_accum.data(),
                               g.d_fb,
                               std::ldexp(1.0, -g.accum_log2),
                               static_cast<float>(spp_total),
                               g.desc.width,
                               g.desc.height,
                               g.desc.rank,
                               g.desc.world_size,
                               g.tiles_x,
                               g.local_tiles,
                               g.desc.progressive ? 0u : 1u,
                               g.pixel_scale ? g.d_pixel_emax.data() : nullptr,
                               counters64,
                               g.h_counters.data(),
                               static_cast<uint32_t>(kCounterBytes / 4)};
        const uint32_t rgrid = std::min<uint32_t>((pixels + 255) / 256, 8192);
        r = launch(g.k_resolve, rgrid, 256, 0, rp);
        if (r != VK_SUCCESS) return r;
        resolved = true;
        g.accum_clean = !g.desc.progressive;
        VCRT_TRY(hipEventRecord(g.ev_resolve.get(), g.stream));
    }
    if (!resolved)  // (one quantum per pixel: no resolve pass)
        VCRT_TRY(hipMemcpyAsync(g.h_counters.data(), counters64, 4 * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    g.counters_clean = resolved;
    const unsigned long long* counters = g.h_counters.data();
    float ms = 0.f;
    VCRT_TRY(hipEventElapsedTime(&ms, g.ev_start.get(), g.ev_stop.get()));
    g.stats.kernel_ms = ms;
    if (!g.direct) {
        VCRT_TRY(hipEventElapsedTime(&ms, g.ev_stop.get(), g.ev_resolve.get()));
        g.stats.resolve_ms = ms;
    }
    g.stats.segments = counters[1];
    g.stats.group_tests = counters[2];
    g.stats.bound_tests = counters[3];
    if (measure) {
        const VkResult ro = build_block_order(total_blocks);
        if (ro != VK_SUCCESS) return ro;
        g.order_key = key;
    }
    if (g.debug_stats)
        VCRT_TRY(hipMemcpy(g.stats.debug, g.d_debug.data(), sizeof(g.stats.debug),
                           hipMemcpyDeviceToHost));
    if (g.debug_stats == 1 && p.region) {  // region counters summed over the waves
        const size_t words = static_cast<size_t>(grid) * (block / 64u) * kRegionCount;
        std::vector<uint32_t> rows(words);
        VCRT_TRY(hipMemcpy(rows.data(), g.d_region.data(), words * sizeof(uint32_t),
                           hipMemcpyDeviceToHost));
        for (size_t w = 0; w < words / kRegionCount; w++)
            for (uint32_t k = 0; k < kRegionCount; k++)
                g.stats.debug[kRegionDebugBase + k] += rows[w * kRegionCount + k];
    }
    g.stats.grid_blocks = static_cast<int32_t>(grid);
    g.stats.block_threads = static_cast<int32_t>(block);
    g.stats.kernel_variant = variant;
    g.stats.lds_bytes = lds;  // tables and stacks; the ring adds ring_entries x 32 B per wave
    g.stats.tables_in_lds = kc.base == g.k_trace_cull_flat_boxes ? 2 :
                            (kc.base == g.k_trace_cull_flat || kc.base == g.k_trace_cull_lane_lds ||
                             kc.base == g.k_trace_cull_lane_lds_wide) ? 1 : 0;
    *outlier_max = static_cast<uint32_t>(counters[0]);
    return VK_SUCCESS;
}

// Outlier quanta (vcrt_math.h "Accumulation"): the render just done saw a quantum sum too large
// for its pixel's scale (every pixel starts at 2^32: |S| >= 2^12). The kernel recorded each such
// pixel's largest |S| in d_pixel_emax; from now on every frame of this configuration quantizes
// each pixel at its own scale, and this frame is rendered again -- a progressive frame together
// with every frame before it, from zero, since their sums were quantized at the old scales. The
// image then depends on each pixel's own samples only (any rank, any schedule). A render at the
// recorded scales sees no outliers (the same samples); a later progressive frame may raise a
// pixel's maximum, and then the same happens again.
static VkResult rerender_scaled(uint64_t spp_total, uint32_t outlier_max) {
    const uint64_t spp = static_cast<uint64_t>(g.desc.samples_per_pixel);
    for (int attempt = 0; outlier_max != 0u; attempt++) {
        if (attempt == 4) return VK_ERROR_UNKNOWN;  // cannot happen: the maxima only grow
        g.pixel_scale = true;
        g.min_scale = std::min(g.min_scale, vcrt::pixel_scale_log2(outlier_max));
        g.stats.accumulate_scale_log2 = g.min_scale;
        g.stats.scale_rerenders += 1;
        outlier_max = 0u;
        if (!g.desc.progressive) {
            VkResult r = trace_frame(spp_total, &outlier_max);
            if (r != VK_SUCCESS) return r;
            continue;
        }
        VCRT_TRY(hipMemsetAsync(g.d_accum.data(), 0, 32u * static_cast<size_t>(g.total_pixels),
                                g.stream));
        for (uint64_t f = 0; f * spp < spp_total; f++) {
            VkResult r = setup_jitter(f * spp);
            if (r == VK_SUCCESS) {
                uint32_t o = 0u;
                r = trace_frame((f + 1) * spp, &o);
                outlier_max = std::max(outlier_max, o);
            }
            if (r != VK_SUCCESS) return r;
        }
    }
    return VK_SUCCESS;
}

vcrt_result vcrt_draw_next_frame(void) {
    if (!g.begun || !g.stage.module) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (g.comm_lost) return VCRT_ERROR_DEVICE_LOST;  // a peer was lost in an earlier frame
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t pixels = g.total_pixels;
    g.stats.segments = 0;
    g.stats.kernel_ms = 0.0;
    g.stats.resolve_ms = 0.0;
    g.stats.gather_ms = 0.0;
    if (pixels != 0 && g.desc.max_depth == 0) {
        // ray_color with MAX_RECURSION_LEVEL 0 returns its undefined value (canonical 0) for
        // every sample without scanning: the frame is (0,0,0,1).
        vcrt::FillParams fp{g.d_fb, g.local_elems, make_float4(0.f, 0.f, 0.f, 1.f)};
        const uint32_t grid = std::min<uint32_t>((g.local_elems + 255) / 256, 4096);
        VkResult r = launch(g.k_fill, grid, 256, 0, fp);
        if (r != VK_SUCCESS) return r;
    }
    const uint64_t spp_total =
        (g.desc.progressive ? g.accumulated : 0) + static_cast<uint64_t>(g.desc.samples_per_pixel);
    // progressive frames add quanta to the pixels' exact sums: at most kAccumMaxChunks in all
    if (g.desc.progressive &&
        (g.accumulated / static_cast<uint64_t>(g.desc.samples_per_pixel) + 1) *
                static_cast<uint64_t>((g.desc.samples_per_pixel + g.quantum - 1) / g.quantum) >
            static_cast<uint64_t>(vcrt::kAccumMaxChunks))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (g.desc.progressive && g.accumulated > 0) {
        // progressive frames continue the sample sequence: indices accumulated.. (+spp)
        const VkResult rj = setup_jitter(g.accumulated);
        if (rj != VK_SUCCESS) return rj;
    }
    if (pixels != 0 && g.desc.max_depth > 0) {
        g.stats.scale_rerenders = 0;
        uint32_t outlier_max = 0u;
        VkResult r = trace_frame(spp_total, &outlier_max);
        if (r == VK_SUCCESS && outlier_max != 0u) r = rerender_scaled(spp_total, outlier_max);
        if (r != VK_SUCCESS) return r;
    }
    if (g.comm && g.desc.world_size > 1) {
        // this rank's own render is complete (the stream synchronize above, no deadline); the
        // exchange's deadline (wait_gather) scales with the frame time for the peers' renders
        VkResult r = gather_frame();
        if (r == VK_SUCCESS) r = wait_gather();
        if (r != VK_SUCCESS) return r;
        float ms = 0.f;
        VCRT_TRY(hipEventElapsedTime(&ms, g.ev_gather_start.get(), g.ev_gather.get()));
        g.stats.gather_ms = ms;
    }
    VCRT_TRY(hipStreamSynchronize(g.stream));
    g.stats.sphere_tests = g.stats.segments * static_cast<uint64_t>(g.nspheres);
    g.stats.samples =
        static_cast<uint64_t>(g.local_pixels) * static_cast<uint64_t>(g.desc.samples_per_pixel);
    g.stats.frames += 1;
    if (g.desc.progressive && pixels != 0 && g.desc.max_depth > 0)
        g.accumulated += static_cast<uint64_t>(g.desc.samples_per_pixel);
    g.stats.accumulated_spp = g.desc.progressive ? g.accumulated
                                                 : static_cast<uint64_t>(g.desc.samples_per_pixel);
    g.stats.frame_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VCRT_SUCCESS;
}

vcrt_result vcrt_end(void) {
    if (!g.begun) return VCRT_SUCCESS;  // idempotent
    if (g.stream) (void)hipStreamSynchronize(g.stream);
    comm_release(false);
    DestroyShaderStage(&g.stage);
    const hipStream_t stream = g.stream;
    g = RendererState{};  // every buffer and event is released here (device_resources.hpp)
    if (stream) (void)hipStreamDestroy(stream);
    return VCRT_SUCCESS;
}

vcrt_result vcrt_motion_project(const vcrt_render_desc* desc, const vcrt_camera* prev_camera,
                                const float* points, int32_t count, float* out) {
    vcrt_render_desc dv;
    if (!read_desc(desc, dv) || !desc_valid(dv) || count < 0 || (count > 0 && (!points || !out)))
        return VCRT_ERROR_INITIALIZATION_FAILED;
    const vcrt::MotionCamera mc =
        vcrt::motion_camera(camera_of(dv.width, dv.height, prev_camera ? *prev_camera : dv.camera));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int32_t i = 0; i < count; i++) {
        const vcrt::f3 Q = vcrt::mk(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
        vcrt::f3 r = vcrt::mk(nan, nan, nan);
        vcrt::motion_project(mc, vcrt::sub(Q, mc.center), &r);
        out[3 * i] = r.x;
        out[3 * i + 1] = r.y;
        out[3 * i + 2] = r.z;
    }
    return VCRT_SUCCESS;
}

vcrt_result vcrt_comm_unique_id(vcrt_comm_id* id) {
    static_assert(sizeof(vcrt_comm_id) == sizeof(ncclUniqueId), "vcrt_comm_id is an ncclUniqueId");
    if (!id) return VCRT_ERROR_INITIALIZATION_FAILED;
    ncclUniqueId u;
    const VkResult r = nccl_vk(ncclGetUniqueId(&u));
    if (r != VK_SUCCESS) return r;
    std::memcpy(id->internal, u.internal, sizeof(u.internal));
    return VCRT_SUCCESS;
}

vcrt_result vcrt_comm_init(const vcrt_comm_id* id) {
    if (!g.begun || !id) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (g.comm) return VCRT_ERROR_INITIALIZATION_FAILED;  // once per vcrt_begin
    VCRT_TRY(hipSetDevice(g.device));  // RCCL binds the communicator to the current device
    VCRT_TRY(hipStreamSynchronize(g.stream));
    ncclUniqueId u;
    std::memcpy(u.internal, id->internal, sizeof(u.internal));
    // non-blocking: set-up and every later operation are waited for with a deadline
    // (comm_wait.hpp), so a rank that never joins fails this call instead of hanging it
    ncclConfig_t config = NCCL_CONFIG_INITIALIZER;
    config.blocking = 0;
    const ncclResult_t e = ncclCommInitRankConfig(&g.comm, g.desc.world_size, u, g.desc.rank,
                                                  &config);
    if (e != ncclSuccess && e != ncclInProgress) {
        if (g.comm) comm_release(true);
        g.comm = nullptr;
        return nccl_vk(e);
    }
    if (vcrt::wait_with_deadline([] { return comm_state(g.comm); }, vcrt::comm_timeout_ms()) !=
        vcrt::WaitResult::kDone) {
        comm_release(true);
        return VCRT_ERROR_INITIALIZATION_FAILED;
    }
    // from here on every failure drops the communicator and the buffers (comm_release)
    auto fail = [](hipError_t err) {
        comm_release(true);
        return to_vk(err);
    };
    hipError_t err;
    if ((err = g.ev_gather_start.create()) != hipSuccess) return fail(err);
    if ((err = g.ev_gather.create()) != hipSuccess) return fail(err);
    if (g.desc.world_size > 1 && g.desc.rank == 0) {
        // (once per vcrt_begin: both buffers are empty here)
        const size_t all = static_cast<size_t>(g.pad_tiles) * 64 *
                           static_cast<size_t>(g.desc.world_size);  // float4 elements
        if ((err = g.d_gather.reserve(all)) != hipSuccess) return fail(err);
        if ((err = hipMemsetAsync(g.d_gather.data(), 0, all * sizeof(float4), g.stream)) !=
            hipSuccess)
            return fail(err);
        const size_t frame = static_cast<size_t>(g.desc.width) * g.desc.height;
        if ((err = g.d_frame.reserve(frame)) != hipSuccess) return fail(err);
        if ((err = hipMemsetAsync(g.d_frame.data(), 0, frame * sizeof(float4), g.stream)) !=
            hipSuccess)
            return fail(err);
        if ((err = hipStreamSynchronize(g.stream)) != hipSuccess) return fail(err);
        g.d_fb = g.d_gather.data();  // rank 0 renders straight into its slot of the gather buffer
    } else {
        g.d_fb = g.d_fb_own.data();
    }
    return VCRT_SUCCESS;
}

vcrt_result vcrt_local_layout(uint32_t* elements, uint32_t* tiles) {
    if (!g.begun || !elements || !tiles) return VCRT_ERROR_INITIALIZATION_FAILED;
    *elements = fb_view().elems;
    *tiles = g.local_tiles;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_read_framebuffer(float* rgba, size_t count) {
    const FbView v = fb_view();
    const size_t bytes = static_cast<size_t>(v.elems) * sizeof(float4);
    if (!g.begun || (!rgba && bytes)) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (count * sizeof(float) < bytes) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (bytes) VCRT_TRY(hipMemcpy(rgba, v.ptr, bytes, hipMemcpyDeviceToHost));
    return VCRT_SUCCESS;
}

vcrt_result vcrt_framebuffer_device(void** device_ptr, size_t* bytes) {
    if (!g.begun || !device_ptr || !bytes) return VCRT_ERROR_INITIALIZATION_FAILED;
    const FbView v = fb_view();
    *device_ptr = v.ptr;
    *bytes = static_cast<size_t>(v.elems) * sizeof(float4);
    return VCRT_SUCCESS;
}

vcrt_result vcrt_set_framebuffer_device(void* device_ptr, size_t bytes) {
    if (!g.begun) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (g.comm) return VCRT_ERROR_FEATURE_NOT_PRESENT;  // the gather owns the buffers
    if (device_ptr == nullptr) {
        g.d_fb = g.d_fb_own.data();
        return VCRT_SUCCESS;
    }
    if (bytes < g.fb_bytes || (reinterpret_cast<uintptr_t>(device_ptr) & 15u))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    g.d_fb = static_cast<float4*>(device_ptr);
    return VCRT_SUCCESS;
}

vcrt_result vcrt_assemble_tiles(const void* gathered, void* frame, int32_t width,
                                int32_t height, int32_t world_size, uint32_t tiles_per_rank) {
    if (!g.begun || !gathered || !frame) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (width <= 0 || height <= 0 || world_size <= 0) return VCRT_ERROR_INITIALIZATION_FAILED;
    for (int32_t r = 0; r < world_size; r++)  // every rank's tiles must fit its slab
        if (tiles_for_rank(width, height, world_size, r) > tiles_per_rank)
            return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    vcrt::AssembleParams ap{static_cast<const float4*>(gathered),
                            static_cast<float4*>(frame),
                            width,
                            height,
                            world_size,
                            static_cast<uint32_t>((width + 7) / 8),
                            tiles_per_rank};
    const uint64_t total = static_cast<uint64_t>(width) * height;
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((total + 255) / 256, 8192));
    VkResult r = launch(g.k_assemble, grid, 256, 0, ap);
    if (r != VK_SUCCESS) return r;
    VCRT_TRY(hipStreamSynchronize(g.stream));
    return VCRT_SUCCESS;
}

vcrt_result vcrt_reset_accumulation(void) {
    if (!g.begun) return VCRT_ERROR_INITIALIZATION_FAILED;
    VCRT_TRY(hipStreamSynchronize(g.stream));
    VCRT_TRY(reset_sums());
    g.accumulated = 0;
    return setup_jitter(0);
}

vcrt_result vcrt_set_camera(const vcrt_camera* camera) {
    if (!g.begun || !camera) return VCRT_ERROR_INITIALIZATION_FAILED;
    const auto t0 = std::chrono::steady_clock::now();
    VCRT_TRY(hipStreamSynchronize(g.stream));
    g.desc.camera = *camera;
    const vcrt_camera& c = g.desc.camera;
    g.cam = vcrt::make_camera(g.desc.width, g.desc.height,
                              vcrt::mk(c.lookfrom[0], c.lookfrom[1], c.lookfrom[2]),
                              vcrt::mk(c.lookat[0], c.lookat[1], c.lookat[2]),
                              vcrt::mk(c.vup[0], c.vup[1], c.vup[2]), c.vfov,
                              [](double x) { return std::tan(x); });
    g.cam_stats = vcrt_camera_stats{};
    // the pixel corners, and the jitter and lens tables of sample 0 (accumulation restarts)
    VkResult r = setup_jitter(0, g.total_pixels != 0);
    if (r != VK_SUCCESS) return r;
    if (g.d_prim_info.data() && g.ncgroups > 0) {  // the renderer has lists (vcrt_set_scene)
        const char* how = std::getenv("VCRT_CAMERA_LISTS");
        const bool device = !(how && std::strcmp(how, "host") == 0) && g.k_cl_prepare &&
                            g.k_cl_count && g.k_cl_scan && g.k_cl_fill;
        if (device) {
            if ((r = build_camera_lists_device()) != VK_SUCCESS) return r;
        } else {
            if ((r = build_camera_lists_host()) != VK_SUCCESS) return r;
        }
        g.cam_stats.on_device = device ? 1 : 0;
        g.cam_stats.quarters = 4ull * g.local_tiles;
        g.cam_stats.group_ids = g.prim_nids;
        g.cam_stats.pair_records = g.prim_npairs;
    }
    g.accumulated = 0;
    g.order_key = 0;  // the cost order is measured again
    VCRT_TRY(reset_sums());
    g.cam_stats.host_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VCRT_SUCCESS;
}

vcrt_result vcrt_get_camera_stats(vcrt_camera_stats* stats) {
    if (!g.begun || !stats) return VCRT_ERROR_INITIALIZATION_FAILED;
    *stats = g.cam_stats;
    return VCRT_SUCCESS;
}

int32_t vcrt_camera_lists_read(uint32_t* group_info, uint32_t* sphere_info, int32_t cap_entries,
                               uint16_t* ids, int32_t cap_ids, float* rec, int32_t cap_floats,
                               int32_t* num_ids, int32_t* num_pairs) {
    if (!g.begun) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (num_ids) *num_ids = 0;
    if (num_pairs) *num_pairs = 0;
    if (g.d_prim_info.data() == nullptr) return 0;  // no tables, a lens, or VCRT_PRIMARY_LISTS=0
    VCRT_TRY(hipStreamSynchronize(g.stream));
    const size_t n = 4 * static_cast<size_t>(g.local_tiles);
    if (num_ids) *num_ids = static_cast<int32_t>(g.prim_nids);
    if (num_pairs) *num_pairs = static_cast<int32_t>(g.prim_npairs);
    if ((group_info || sphere_info) && cap_entries >= 0 && static_cast<size_t>(cap_entries) >= n) {
        std::vector<uint32_t> info(2 * n);
        VCRT_TRY(hipMemcpy(info.data(), g.d_prim_info.data(), sizeof(uint32_t) * info.size(),
                           hipMemcpyDeviceToHost));
        for (size_t e = 0; e < n; e++) {
            if (group_info) group_info[e] = info[2 * e];
            if (sphere_info) sphere_info[e] = info[2 * e + 1];
        }
    }
    if (ids && g.prim_nids > 0 && cap_ids >= 0 && static_cast<size_t>(cap_ids) >= g.prim_nids)
        VCRT_TRY(hipMemcpy(ids, g.d_prim_ids.data(), sizeof(uint16_t) * g.prim_nids,
                           hipMemcpyDeviceToHost));
    const size_t floats = g.prim_npairs * 12;
    if (rec && floats > 0 && cap_floats >= 0 && static_cast<size_t>(cap_floats) >= floats)
        VCRT_TRY(hipMemcpy(rec, reinterpret_cast<const float*>(g.d_cam_rec.data()) +
                                    static_cast<size_t>(g.ncbig) * 16,
                           sizeof(float) * floats, hipMemcpyDeviceToHost));
    return static_cast<int32_t>(n);
}

// ---- scene updates ------------------------------------------------------------------------

namespace {

// The scalars of refitted tables into the renderer's state, as vcrt_set_scene takes them.
void install_scalars(const vcrt::CullTables& ct, bool bounded, bool radii_safe) {
    std::memcpy(g.cmargin, ct.margin, sizeof(ct.margin));
    g.cslab_on = ct.slab;
    g.cslab[0] = ct.slab_lohi[0];
    g.cslab[1] = ct.slab_lohi[1];
    std::memcpy(g.cfp_x, ct.fp_x, sizeof(g.cfp_x));
    std::memcpy(g.cfp_z, ct.fp_z, sizeof(g.cfp_z));
    std::memcpy(g.cfp_y, ct.fp_y, sizeof(g.cfp_y));
    g.cfp_k2 = ct.fp_k2;
    g.cfp_always = ct.fp_always;
    if (ct.gf_cells > 0 && g.d_gf_tab.data() != nullptr) {
        std::memcpy(g.cgf_x, ct.gf_x, sizeof(g.cgf_x));
        std::memcpy(g.cgf_z, ct.gf_z, sizeof(g.cgf_z));
        std::memcpy(g.cgf_always, ct.gf_always, sizeof(g.cgf_always));
        g.cgf_k2 = ct.gf_k2;
        g.cgf_n = static_cast<uint32_t>(ct.gf_cells);
        g.cgf_ok = ct.gf_ok;
    }
    g.scene_bounded = bounded;
    g.radii_safe = radii_safe;
}

vcrt_scene_scalars scalars_struct(const vcrt::CullTables& ct, bool bounded, bool radii_safe) {
    vcrt_scene_scalars s{};
    s.nbig = ct.nbig;
    s.ngroups = ct.ngroups;
    std::memcpy(s.margin, ct.margin, sizeof(s.margin));
    s.slab_on = ct.slab ? 1 : 0;
    std::memcpy(s.slab, ct.slab_lohi, sizeof(s.slab));
    std::memcpy(s.fp_x, ct.fp_x, sizeof(s.fp_x));
    std::memcpy(s.fp_z, ct.fp_z, sizeof(s.fp_z));
    std::memcpy(s.fp_y, ct.fp_y, sizeof(s.fp_y));
    s.fp_k2 = ct.fp_k2;
    s.fp_always = ct.fp_always;
    s.gf_n = static_cast<uint32_t>(ct.gf_cells);
    std::memcpy(s.gf_x, ct.gf_x, sizeof(s.gf_x));
    std::memcpy(s.gf_z, ct.gf_z, sizeof(s.gf_z));
    s.gf_k2 = ct.gf_k2;
    std::memcpy(s.gf_always, ct.gf_always, sizeof(s.gf_always));
    s.gf_ok = ct.gf_ok ? 1 : 0;
    s.bounded = bounded ? 1 : 0;
    s.radii_safe = radii_safe ? 1 : 0;
    return s;
}

// The renderer's scalars in the same form (a renderer without group tables: their defaults).
vcrt_scene_scalars scalars_struct_state() {
    vcrt::CullTables ct;
    ct.nbig = g.ncbig;
    ct.ngroups = g.ncgroups;
    std::memcpy(ct.margin, g.cmargin, sizeof(ct.margin));
    ct.slab = g.cslab_on;
    if (ct.slab) std::memcpy(ct.slab_lohi, g.cslab, sizeof(ct.slab_lohi));
    std::memcpy(ct.fp_x, g.cfp_x, sizeof(ct.fp_x));
    std::memcpy(ct.fp_z, g.cfp_z, sizeof(ct.fp_z));
    std::memcpy(ct.fp_y, g.cfp_y, sizeof(ct.fp_y));
    ct.fp_k2 = g.cfp_k2;
    ct.fp_always = g.cfp_always;
    if (g.cgf_n > 0) {
        ct.gf_cells = static_cast<int32_t>(g.cgf_n);
        std::memcpy(ct.gf_x, g.cgf_x, sizeof(ct.gf_x));
        std::memcpy(ct.gf_z, g.cgf_z, sizeof(ct.gf_z));
        std::memcpy(ct.gf_always, g.cgf_always, sizeof(ct.gf_always));
        ct.gf_k2 = g.cgf_k2;
        ct.gf_ok = g.cgf_ok;
    }
    return scalars_struct(ct, g.scene_bounded, g.radii_safe);
}

// One table of (values, ct) as the bytes vcrt_set_scene uploads; false: no such table.
bool table_bytes_host(const vcrt_sphere* v, int32_t count, const vcrt::CullTables& ct,
                      int32_t table, std::vector<unsigned char>& out) {
    auto put = [&out](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        out.assign(b, b + n);
        return n > 0;
    };
    auto floats = [&put](const std::vector<float>& t) { return put(t.data(), sizeof(float) * t.size()); };
    auto words = [&put](const std::vector<uint32_t>& t) {
        return put(t.data(), sizeof(uint32_t) * t.size());
    };
    if (table == VCRT_TABLE_LINEAR) return floats(linear_table(v, count));
    if (table == VCRT_TABLE_CENTER_RADIUS || table == VCRT_TABLE_SHADE ||
        table == VCRT_TABLE_MATERIAL) {
        std::vector<float4> cr, shade, mat;
        sphere_rows(v, count, cr, shade, mat);
        const std::vector<float4>& t = table == VCRT_TABLE_CENTER_RADIUS ? cr
                                       : table == VCRT_TABLE_SHADE       ? shade
                                                                         : mat;
        return put(t.data(), sizeof(float4) * t.size());
    }
    if (ct.ngroups <= 0) return false;
    switch (table) {
        case VCRT_TABLE_GROUPS: return floats(group_records(ct));
        case VCRT_TABLE_BOUND: return floats(ct.bound);
        case VCRT_TABLE_BOUND_NF: return floats(near_far(ct.bound));
        case VCRT_TABLE_NODE: return floats(ct.node);
        case VCRT_TABLE_NODE_NF: return floats(node_near_far(ct));
        case VCRT_TABLE_TOP: return floats(ct.top);
        case VCRT_TABLE_FOOT: return words(pack_footprint(ct));
        case VCRT_TABLE_GROUP_FOOT: return words(ct.gf_tab);
        case VCRT_TABLE_SCALARS: {
            const vcrt_scene_scalars s =
                scalars_struct(ct, values_bounded(v, count), values_radii_safe(v, count));
            return put(&s, sizeof(s));
        }
        default: return false;
    }
}

// The device buffer of a table and its size in bytes (null: no such table).
const void* table_device(int32_t table, size_t* bytes) {
    const size_t n = static_cast<size_t>(g.nspheres), ng = static_cast<size_t>(g.ncgroups);
    *bytes = 0;
    if (table == VCRT_TABLE_LINEAR) {
        *bytes = ((n + 3) / 4 + 1) * 64;
        return g.d_geom.data();
    }
    if (table == VCRT_TABLE_CENTER_RADIUS || table == VCRT_TABLE_SHADE ||
        table == VCRT_TABLE_MATERIAL) {
        *bytes = n * 16;
        return table == VCRT_TABLE_CENTER_RADIUS ? g.d_center_radius.data()
               : table == VCRT_TABLE_SHADE       ? g.d_shade.data()
                                                 : g.d_material.data();
    }
    if (ng == 0) return nullptr;
    const size_t node_pairs = ng / vcrt::kNodeGroups / 2, tops = (ng + 63) / 64;
    switch (table) {
        case VCRT_TABLE_GROUPS:
            *bytes = (static_cast<size_t>(g.ncbig) + ng) * 80;
            return g.d_cgroup.data();
        case VCRT_TABLE_BOUND: *bytes = ng / 2 * 64; return g.d_cbound.data();
        case VCRT_TABLE_BOUND_NF: *bytes = ng / 2 * 80; return g.d_cbound_nf.data();
        case VCRT_TABLE_NODE: *bytes = node_pairs * 64; return g.d_cnode.data();
        case VCRT_TABLE_NODE_NF: *bytes = (node_pairs + 3) / 4 * 4 * 80; return g.d_cnode_nf.data();
        case VCRT_TABLE_TOP: *bytes = (tops + (tops & 1)) / 2 * 64; return g.d_ctop.data();
        case VCRT_TABLE_FOOT:
            *bytes = sizeof(uint32_t) * vcrt::kFootCells * (ng > 128 ? 4 : 2);
            return g.d_fp_tab.data();
        case VCRT_TABLE_GROUP_FOOT:
            *bytes = sizeof(uint32_t) * 16 * g.cgf_n;
            return g.d_gf_tab.data();
        default: return nullptr;
    }
}

// The refit on the host: the tables of h_ct's grouping for h_spheres' values (cluster.cpp
// tables_of_grouping), uploaded into the kept buffers on the render stream.
VkResult refit_on_host() {
    vcrt::tables_of_grouping(g.h_spheres.data(), g.nspheres, g.h_ct);
    g.h_ct_stale = false;
    // (the images stay until the stream has taken them)
    std::vector<std::vector<unsigned char>> images(VCRT_TABLE_GROUP_FOOT + 1);
    for (int32_t table = VCRT_TABLE_LINEAR; table <= VCRT_TABLE_GROUP_FOOT; table++) {
        size_t bytes = 0;
        void* dst = const_cast<void*>(table_device(table, &bytes));
        std::vector<unsigned char>& image = images[table];
        if (!dst || bytes == 0 ||
            !table_bytes_host(g.h_spheres.data(), g.nspheres, g.h_ct, table, image))
            continue;
        if (image.size() != bytes) return VK_ERROR_INITIALIZATION_FAILED;  // another grouping
        VCRT_TRY(hipMemcpyAsync(dst, image.data(), bytes, hipMemcpyHostToDevice, g.stream));
    }
    VCRT_TRY(hipStreamSynchronize(g.stream));
    install_scalars(g.h_ct, true, values_radii_safe(g.h_spheres.data(), g.nspheres));
    return VK_SUCCESS;
}

// The refit on the device (scene_update.hip) from `d_values` on the render stream: rows, groups,
// levels and summary; the summary comes back (with the spheres, when `back` is set: the device
// variant's values for h_spheres) in one synchronisation; the host computes the scalars with
// cluster.cpp's own code; footprint tables. *unbounded: a value failed |v| <= 2^30 (the tables
// are then garbage and the caller rebuilds).
VkResult refit_on_device(const float* d_values, vcrt_sphere* back, bool* unbounded) {
    *unbounded = false;
    VCRT_TRY(g.d_su_summary.reserve(1));
    VCRT_TRY(g.h_su_summary.reserve(1));
    for (Event& e : g.ev_su) VCRT_TRY(e.create());
    vcrt::SceneUpdateParams p{};
    p.spheres = d_values;
    p.geom = reinterpret_cast<float*>(g.d_geom.data());
    p.center_radius = reinterpret_cast<float*>(g.d_center_radius.data());
    p.shade = reinterpret_cast<float*>(g.d_shade.data());
    p.material = reinterpret_cast<float*>(g.d_material.data());
    p.cgroup = reinterpret_cast<float*>(g.d_cgroup.data());
    p.cbound = reinterpret_cast<float*>(g.d_cbound.data());
    p.cbound_nf = reinterpret_cast<float*>(g.d_cbound_nf.data());
    p.cnode = reinterpret_cast<float*>(g.d_cnode.data());
    p.cnode_nf = reinterpret_cast<float*>(g.d_cnode_nf.data());
    p.ctop = reinterpret_cast<float*>(g.d_ctop.data());
    p.fp_tab = g.d_fp_tab.data();
    p.gf_tab = reinterpret_cast<uint32_t*>(g.d_gf_tab.data());
    p.summary = g.d_su_summary.data();
    p.nspheres = static_cast<uint32_t>(g.nspheres);
    p.nbig = static_cast<uint32_t>(g.ncbig);
    p.ngroups = static_cast<uint32_t>(g.ncgroups);
    p.nnodes = p.ngroups / static_cast<uint32_t>(vcrt::kNodeGroups);
    p.ntops = (p.ngroups + 63u) / 64u;
    VCRT_TRY(hipEventRecord(g.ev_su[0].get(), g.stream));
    const uint32_t entries = 4u * ((p.nspheres + 3u) / 4u + 1u);
    VkResult r = launch(g.k_su_rows, (entries + 255u) / 256u, 256, 0, p);
    if (r != VK_SUCCESS) return r;
    if ((r = launch(g.k_su_groups, (p.nbig + p.ngroups + 255u) / 256u, 256, 0, p)) != VK_SUCCESS)
        return r;
    if ((r = launch(g.k_su_levels, 1, vcrt::kSceneSummaryThreads, 0, p)) != VK_SUCCESS) return r;
    VCRT_TRY(hipMemcpyAsync(g.h_su_summary.data(), g.d_su_summary.data(),
                            sizeof(vcrt::SceneSummary), hipMemcpyDeviceToHost, g.stream));
    if (back)
        VCRT_TRY(hipMemcpyAsync(back, d_values, sizeof(vcrt_sphere) * p.nspheres,
                                hipMemcpyDeviceToHost, g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    const vcrt::SceneSummary m = *g.h_su_summary.data();
    if (!m.bounded) {
        *unbounded = true;
        return VK_SUCCESS;
    }
    vcrt::CullTables ct;  // the scalars alone
    ct.nbig = g.ncbig;
    ct.ngroups = g.ncgroups;
    vcrt::scalars_of_summary(m, ct);
    install_scalars(ct, true, m.radii_safe != 0u);
    for (int k = 0; k < 2; k++) {
        p.fp_x[k] = ct.fp_x[k];
        p.fp_z[k] = ct.fp_z[k];
        p.gf_x[k] = ct.gf_x[k];
        p.gf_z[k] = ct.gf_z[k];
    }
    p.fp_ok = ct.fp_ok ? 1u : 0u;
    p.gf_n = g.d_gf_tab.data() ? g.cgf_n : 0u;
    p.gf_keep_all = ct.gf_keep_all ? 1u : 0u;
    const uint32_t cells = vcrt::kFootCells * (p.ngroups > 128u ? 4u : 2u) + 4u * p.gf_n;
    if ((r = launch(g.k_su_footprint, (cells + 255u) / 256u, 256, 0, p)) != VK_SUCCESS) return r;
    VCRT_TRY(hipEventRecord(g.ev_su[1].get(), g.stream));
    g.h_ct_stale = true;
    return VK_SUCCESS;
}

vcrt_result update_spheres(const vcrt_sphere* spheres, int32_t count, bool on_device_ptr) {
    if (!g.begun) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (count < 0 || (count > 0 && !spheres)) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (count != g.nspheres) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    const auto t0 = std::chrono::steady_clock::now();
    auto elapsed = [t0]() {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
            .count();
    };
    g.su_stats = vcrt_scene_update_stats{};
    const bool kernels = g.k_su_rows && g.k_su_groups && g.k_su_levels && g.k_su_footprint;
    const char* how = std::getenv("VCRT_SCENE_UPDATE");
    const bool on_host = how && std::strcmp(how, "host") == 0;
    // the values on the host, where the path needs them before it starts
    std::vector<vcrt_sphere> fetched;
    auto host_values = [&]() -> const vcrt_sphere* {
        if (!on_device_ptr) return spheres;
        if (fetched.empty() && count > 0) {
            fetched.resize(count);
            (void)hipStreamSynchronize(g.stream);
            if (hipMemcpy(fetched.data(), spheres, sizeof(vcrt_sphere) * count,
                          hipMemcpyDeviceToHost) != hipSuccess)
                return nullptr;
        }
        return fetched.data();
    };
    auto rebuild = [&](const vcrt_sphere* values) -> vcrt_result {
        if (!values && count > 0) return VCRT_ERROR_UNKNOWN;
        const vcrt_result r = vcrt_set_scene(values, count);
        g.su_stats.rebuilt = 1;
        g.su_stats.host_ms = elapsed();
        return r;
    };
    if (g.ncgroups == 0 || count == 0 || (!kernels && !on_host)) return rebuild(host_values());
    bool device = false;
    if (on_host) {
        const vcrt_sphere* values = host_values();
        if (!values) return VCRT_ERROR_UNKNOWN;
        if (!values_bounded(values, count)) return rebuild(values);
        if (values != g.h_spheres.data()) g.h_spheres.assign(values, values + count);
        const VkResult r = refit_on_host();
        if (r != VK_SUCCESS) return r;
    } else {
        const float* d_values = reinterpret_cast<const float*>(spheres);
        if (!on_device_ptr) {
            if (!values_bounded(spheres, count)) return rebuild(spheres);
            const size_t floats = static_cast<size_t>(count) * 10;
            VCRT_TRY(g.d_su_spheres.reserve(floats));
            VCRT_TRY(hipMemcpyAsync(g.d_su_spheres.data(), spheres, sizeof(float) * floats,
                                    hipMemcpyHostToDevice, g.stream));
            d_values = g.d_su_spheres.data();
            if (spheres != g.h_spheres.data()) g.h_spheres.assign(spheres, spheres + count);
        } else {
            fetched.resize(count);
        }
        bool unbounded = false;
        const VkResult r =
            refit_on_device(d_values, on_device_ptr ? fetched.data() : nullptr, &unbounded);
        if (r != VK_SUCCESS) return r;
        if (unbounded) return rebuild(fetched.data());
        if (on_device_ptr) g.h_spheres = std::move(fetched);
        device = true;
    }
    // the camera-ray lists and camera-relative records of the refitted tables
    if (g.d_prim_info.data() != nullptr) {
        const char* lists = std::getenv("VCRT_CAMERA_LISTS");
        const bool lists_device = !(lists && std::strcmp(lists, "host") == 0) && g.k_cl_prepare &&
                                  g.k_cl_count && g.k_cl_scan && g.k_cl_fill;
        const vcrt_camera_stats last_move = g.cam_stats;  // vcrt_set_camera's record stays
        const VkResult r = lists_device ? build_camera_lists_device() : build_camera_lists_host();
        if (r != VK_SUCCESS) return r;
        g.su_stats.lists_ms = lists_device ? g.cam_stats.lists_ms : 0.0;
        g.cam_stats = last_move;
    }
    if (g.desc.progressive && g.accumulated > 0) {
        // new values restart progressive accumulation at sample 0, as a new scene does
        const VkResult rj = setup_jitter(0);
        if (rj != VK_SUCCESS) return rj;
    }
    g.accumulated = 0;
    g.order_key = 0;  // the cost order is measured again
    VCRT_TRY(reset_sums());
    VCRT_TRY(hipStreamSynchronize(g.stream));
    g.stage.pName = select_kernel().name;
    if (device) {
        float ms = 0.0f;
        VCRT_TRY(hipEventElapsedTime(&ms, g.ev_su[0].get(), g.ev_su[1].get()));
        g.su_stats.refit_ms = ms;
    }
    const uint64_t ng = static_cast<uint64_t>(g.ncgroups), tops = (ng + 63) / 64;
    g.su_stats.on_device = device ? 1 : 0;
    g.su_stats.groups = static_cast<uint64_t>(g.ncbig) + ng;
    g.su_stats.boxes = ng + ng / vcrt::kNodeGroups + tops + (tops & 1);
    g.su_stats.footprint_cells =
        4ull * vcrt::kFootCells + 4ull * (g.d_gf_tab.data() ? g.cgf_n : 0u);
    g.su_stats.host_ms = elapsed();
    return VCRT_SUCCESS;
}

}  // namespace

vcrt_result vcrt_update_spheres(const vcrt_sphere* spheres, int32_t count) {
    return update_spheres(spheres, count, false);
}

vcrt_result vcrt_update_spheres_device(const vcrt_sphere* spheres, int32_t count) {
    return update_spheres(spheres, count, true);
}

vcrt_result vcrt_get_scene_update_stats(vcrt_scene_update_stats* stats) {
    if (!g.begun || !stats) return VCRT_ERROR_INITIALIZATION_FAILED;
    *stats = g.su_stats;
    return VCRT_SUCCESS;
}

int64_t vcrt_scene_table_host(const vcrt_sphere* grouping_of, const vcrt_sphere* values,
                              int32_t count, int32_t table, void* buf, size_t cap) {
    if (count < 0 || (count > 0 && (!grouping_of || !values))) return 0;
    vcrt::CullTables ct;
    // (values that fail the bound have no tables, as a scene that fails it has none)
    if (vcrt::choose_grouping(grouping_of, count, ct) && values_bounded(values, count))
        vcrt::tables_of_grouping(values, count, ct);
    else
        ct = vcrt::CullTables{};
    std::vector<unsigned char> image;
    if (!table_bytes_host(values, count, ct, table, image)) return 0;
    if (buf && cap >= image.size()) std::memcpy(buf, image.data(), image.size());
    return static_cast<int64_t>(image.size());
}

int64_t vcrt_scene_table_read(int32_t table, void* buf, size_t cap) {
    if (!g.begun) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (table == VCRT_TABLE_SCALARS) {
        if (g.ncgroups == 0) return 0;
        const vcrt_scene_scalars s = scalars_struct_state();
        if (buf && cap >= sizeof(s)) std::memcpy(buf, &s, sizeof(s));
        return static_cast<int64_t>(sizeof(s));
    }
    size_t bytes = 0;
    const void* src = table_device(table, &bytes);
    if (!src || bytes == 0) return 0;
    if (buf && cap >= bytes) {
        VCRT_TRY(hipStreamSynchronize(g.stream));
        VCRT_TRY(hipMemcpy(buf, src, bytes, hipMemcpyDeviceToHost));
    }
    return static_cast<int64_t>(bytes);
}

vcrt_result vcrt_selftest_sin(uint32_t first, uint32_t count, uint64_t* mismatches,
                              uint64_t* fallbacks, uint32_t* first_mismatch) {
    if (!g.begun || !mismatches || !fallbacks || !first_mismatch)
        return VCRT_ERROR_INITIALIZATION_FAILED;
    hipFunction_t f = nullptr;
    VCRT_TRY(hipModuleGetFunction(&f, static_cast<hipModule_t>(g.stage.module), "vcrt_check_sin"));
    DeviceBuffer<uint32_t> buf;  // [2] u64 counters + first mismatch; freed on every return
    VCRT_TRY(buf.reserve(6));
    uint32_t init[6] = {0, 0, 0, 0, 0xFFFFFFFFu, 0};
    VCRT_TRY(hipMemcpy(buf.data(), init, sizeof(init), hipMemcpyHostToDevice));
    VCRT_TRY(hipStreamSynchronize(nullptr));  // (the check runs on g.stream)
    vcrt::SinCheckParams sp{reinterpret_cast<unsigned long long*>(buf.data()), buf.data() + 4,
                            first, count, {}};
    for (int j = 0; j < 13; j++) sp.sin_c[j] = vcrt::kSinC[j];
    const VkResult r = launch(f, 8 * 256 * 8, 256, 0, sp);
    if (r != VK_SUCCESS) return r;
    uint32_t out[6] = {0, 0, 0, 0, 0, 0};
    VCRT_TRY(hipMemcpyAsync(out, buf.data(), sizeof(out), hipMemcpyDeviceToHost, g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    std::memcpy(mismatches, &out[0], 8);
    std::memcpy(fallbacks, &out[2], 8);
    *first_mismatch = out[4];
    return VCRT_SUCCESS;
}

vcrt_result vcrt_selftest_unit(const float* triples, uint32_t n, float* out) {
    if (!g.begun || (n && (!triples || !out)) || n > (1u << 28))
        return VCRT_ERROR_INITIALIZATION_FAILED;
    if (!n) return VCRT_SUCCESS;
    hipFunction_t f = nullptr;
    VCRT_TRY(hipModuleGetFunction(&f, static_cast<hipModule_t>(g.stage.module), "vcrt_check_unit"));
    const size_t bytes = sizeof(float) * 3u * n;
    DeviceBuffer<float> buf;  // the triples, then their unit vectors; freed on every return
    VCRT_TRY(buf.reserve(6u * static_cast<size_t>(n)));
    float* d_in = buf.data();
    float* d_out = d_in + 3u * static_cast<size_t>(n);
    hipError_t e = hipMemcpyAsync(d_in, triples, bytes, hipMemcpyHostToDevice, g.stream);
    vcrt::UnitCheckParams up{d_in, d_out, n};
    VkResult r = e == hipSuccess ? launch(f, std::min<uint32_t>((n + 255u) / 256u, 4096u), 256, 0, up)
                                 : to_vk(e);
    if (r == VK_SUCCESS) {
        e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, g.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
        r = to_vk(e);
    } else {
        (void)hipStreamSynchronize(g.stream);
    }
    return r;
}

vcrt_result vcrt_read_framebuffer_srgb8(uint8_t* rgba8, size_t bytes) {
    const FbView v = fb_view();
    if (!g.begun || (!rgba8 && v.elems)) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (bytes < static_cast<size_t>(v.elems) * 4) return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (!v.elems) return VCRT_SUCCESS;
    VCRT_TRY(g.d_srgb.reserve(v.elems));  // the view may have grown (vcrt_comm_init)
    vcrt::EncodeParams ep{v.ptr, g.d_srgb.data(), g.d_srgb_thresholds.data(), v.elems};
    const uint32_t grid = std::min<uint32_t>((v.elems + 255) / 256, 4096);
    VkResult r = launch(g.k_encode, grid, 256, 0, ep);
    if (r != VK_SUCCESS) return r;
    VCRT_TRY(hipMemcpyAsync(rgba8, g.d_srgb.data(), sizeof(uchar4) * v.elems,
                            hipMemcpyDeviceToHost, g.stream));
    VCRT_TRY(hipStreamSynchronize(g.stream));
    return VCRT_SUCCESS;
}

void vcrt_srgb8_thresholds(float thresholds[255]) {
    if (thresholds) srgb_thresholds(thresholds);
}

vcrt_result vcrt_get_stats(vcrt_stats* stats) {
    if (!g.begun || !stats) return VCRT_ERROR_INITIALIZATION_FAILED;
    *stats = g.stats;
    return VCRT_SUCCESS;
}

vcrt_result vcrt_shader_load(const char* filename) {
    if (!g.begun) return VCRT_ERROR_INITIALIZATION_FAILED;
    if (!filename) return VCRT_ERROR_INCOMPATIBLE_SHADER_BINARY;
    (void)hipStreamSynchronize(g.stream);
    const VkResult r = load_code_object(filename);
    if (r == VK_SUCCESS && g.d_geom.data()) g.stage.pName = select_kernel().name;
    // a lens renderer cannot draw with a code object that has no lens kernels
    if (r == VK_SUCCESS && lens_on() && !lens_kernels_bound()) return VCRT_ERROR_FEATURE_NOT_PRESENT;
    return r;
}

int32_t vcrt_scene_builtin(int32_t scene_id, vcrt_sphere* out, int32_t cap) {
    std::vector<vcrt_sphere> s;
    const int r = vcrt::builtin_scene(scene_id, s);
    if (r != VCRT_SUCCESS) return r;
    if (out)
        std::copy_n(s.begin(), std::min<size_t>(s.size(), static_cast<size_t>(std::max(cap, 0))),
                    out);
    return static_cast<int32_t>(s.size());
}

size_t vcrt_scene_generator_text(char* buf, size_t cap) {
    const std::string t = vcrt::scene_generator_text();
    if (buf && cap) {
        const size_t k = std::min(t.size(), cap - 1);
        std::memcpy(buf, t.data(), k);
        buf[k] = '\0';
    }
    return t.size();
}

int32_t vcrt_cull_tables(const vcrt_sphere* spheres, int32_t count, float* geom, float* bound,
                         float* node, float* top, int32_t* index, int32_t* big_groups,
                         float* margin4, int32_t cap_groups) {
    if (count < 0 || (count > 0 && !spheres)) return 0;
    vcrt::CullTables ct;
    if (!vcrt::build_cull_tables(spheres, count, ct)) return 0;
    if (big_groups) *big_groups = ct.nbig;
    if (margin4) std::memcpy(margin4, ct.margin, sizeof(ct.margin));
    if (ct.nbig + ct.ngroups <= cap_groups) {
        if (geom) std::memcpy(geom, ct.geom.data(), sizeof(float) * ct.geom.size());
        if (bound) std::memcpy(bound, ct.bound.data(), sizeof(float) * ct.bound.size());
        if (node) std::memcpy(node, ct.node.data(), sizeof(float) * ct.node.size());
        if (top) std::memcpy(top, ct.top.data(), sizeof(float) * ct.top.size());
        if (index) std::memcpy(index, ct.index.data(), sizeof(int32_t) * ct.index.size());
    }
    return ct.ngroups;
}

int32_t vcrt_cull_footprint(const vcrt_sphere* spheres, int32_t count, uint32_t* tables,
                            float* params8, uint32_t* always) {
    if (count < 0 || (count > 0 && !spheres)) return 0;
    vcrt::CullTables ct;
    if (!vcrt::build_cull_tables(spheres, count, ct) || ct.fp_tab.empty()) return 0;
    if (tables) std::memcpy(tables, ct.fp_tab.data(), sizeof(uint32_t) * ct.fp_tab.size());
    if (params8) {
        const float v[8] = {ct.fp_x[0], ct.fp_x[1], ct.fp_z[0], ct.fp_z[1],
                            ct.fp_y[0], ct.fp_y[1], ct.fp_k2,   0.0f};
        std::memcpy(params8, v, sizeof(v));
    }
    if (always) *always = ct.fp_always;
    return vcrt::kFootprintCells;
}

int32_t vcrt_cull_group_footprint(const vcrt_sphere* spheres, int32_t count, uint32_t* tables,
                                  float* params8, uint32_t* always4, int32_t* eligible) {
    if (eligible) *eligible = 0;
    if (count < 0 || (count > 0 && !spheres)) return 0;
    vcrt::CullTables ct;
    if (!vcrt::build_cull_tables(spheres, count, ct) || ct.gf_cells == 0) return 0;
    if (tables) std::memcpy(tables, ct.gf_tab.data(), sizeof(uint32_t) * ct.gf_tab.size());
    if (params8) {
        const float v[8] = {ct.gf_x[0], ct.gf_x[1], ct.gf_z[0], ct.gf_z[1],
                            ct.fp_y[0], ct.fp_y[1], ct.gf_k2,   0.0f};
        std::memcpy(params8, v, sizeof(v));
    }
    if (always4) std::memcpy(always4, ct.gf_always, sizeof(ct.gf_always));
    if (eligible) *eligible = ct.gf_ok ? 1 : 0;
    return ct.gf_cells;
}

int32_t vcrt_cull_slab(const vcrt_sphere* spheres, int32_t count, float lohi[2]) {
    if (count < 0 || (count > 0 && !spheres)) return 0;
    vcrt::CullTables ct;
    if (!vcrt::build_cull_tables(spheres, count, ct) || !ct.slab) return 0;
    if (lohi) std::memcpy(lohi, ct.slab_lohi, sizeof(ct.slab_lohi));
    return 1;
}

namespace {
// Culling tables and the kernels' camera array for a desc (host only).
vcrt::Camera desc_camera(const vcrt_render_desc& d) {
    const vcrt_camera& c = d.camera;
    return vcrt::make_camera(d.width, d.height,
                             vcrt::mk(c.lookfrom[0], c.lookfrom[1], c.lookfrom[2]),
                             vcrt::mk(c.lookat[0], c.lookat[1], c.lookat[2]),
                             vcrt::mk(c.vup[0], c.vup[1], c.vup[2]), c.vfov,
                             [](double x) { return std::tan(x); });
}

// (a lens desc has no camera-ray lists: its rays do not share an origin)
// The tables are those of `grouping_of`'s grouping filled with `spheres`' values (a refit; the
// scene's own tables when the two are one).
bool host_camera_tables(const vcrt_sphere* grouping_of, const vcrt_sphere* spheres, int32_t count,
                        const vcrt_render_desc* desc_in, vcrt::CullTables& ct, float cam[12]) {
    vcrt_render_desc dv;
    if (!read_desc(desc_in, dv) || !desc_valid(dv) || count < 0 ||
        (count > 0 && (!spheres || !grouping_of)))
        return false;
    if (dv.lens_radius > 0.0f) return false;
    if (!vcrt::choose_grouping(grouping_of, count, ct) || !values_bounded(spheres, count))
        return false;
    vcrt::tables_of_grouping(spheres, count, ct);
    const vcrt::Camera cm = desc_camera(dv);
    const vcrt::f3 v[4] = {cm.pixel00, cm.delta_u, cm.delta_v, cm.center};
    for (int i = 0; i < 4; i++) {
        cam[3 * i + 0] = v[i].x;
        cam[3 * i + 1] = v[i].y;
        cam[3 * i + 2] = v[i].z;
    }
    return true;
}
}  // namespace

int32_t vcrt_primary_lists(const vcrt_sphere* spheres, int32_t count, const vcrt_render_desc* desc,
                           uint32_t* info, int32_t cap_tiles, uint16_t* ids, int32_t cap_ids) {
    return vcrt_refit_primary_lists(spheres, spheres, count, desc, info, cap_tiles, ids, cap_ids);
}

int32_t vcrt_refit_primary_lists(const vcrt_sphere* grouping_of, const vcrt_sphere* spheres,
                                 int32_t count, const vcrt_render_desc* desc, uint32_t* info,
                                 int32_t cap_tiles, uint16_t* ids, int32_t cap_ids) {
    vcrt::CullTables ct;
    float cam[12];
    if (!host_camera_tables(grouping_of, spheres, count, desc, ct, cam)) return -1;
    vcrt::PrimaryLists pl;
    vcrt::build_primary_lists(ct, cam, desc->width, desc->height, desc->rank, desc->world_size,
                              pl);
    if (info && cap_tiles >= static_cast<int32_t>(pl.info.size()))
        std::memcpy(info, pl.info.data(), sizeof(uint32_t) * pl.info.size());
    if (ids && cap_ids >= static_cast<int32_t>(pl.ids.size()))
        std::memcpy(ids, pl.ids.data(), sizeof(uint16_t) * pl.ids.size());
    return static_cast<int32_t>(pl.ids.size());
}

int32_t vcrt_primary_sphere_lists(const vcrt_sphere* spheres, int32_t count,
                                  const vcrt_render_desc* desc, uint32_t* info, int32_t cap_tiles,
                                  float* rec, int32_t cap_floats) {
    return vcrt_refit_primary_sphere_lists(spheres, spheres, count, desc, info, cap_tiles, rec,
                                           cap_floats);
}

int32_t vcrt_refit_primary_sphere_lists(const vcrt_sphere* grouping_of, const vcrt_sphere* spheres,
                                        int32_t count, const vcrt_render_desc* desc,
                                        uint32_t* info, int32_t cap_tiles, float* rec,
                                        int32_t cap_floats) {
    vcrt::CullTables ct;
    float cam[12];
    if (!host_camera_tables(grouping_of, spheres, count, desc, ct, cam)) return -1;
    vcrt::PrimarySphereLists sl;
    vcrt::build_primary_sphere_lists(ct, spheres, cam, desc->width, desc->height, desc->rank,
                                     desc->world_size, sl);
    if (info && cap_tiles >= static_cast<int32_t>(sl.info.size()))
        std::memcpy(info, sl.info.data(), sizeof(uint32_t) * sl.info.size());
    if (rec && cap_floats >= static_cast<int32_t>(sl.rec.size()))
        std::memcpy(rec, sl.rec.data(), sizeof(float) * sl.rec.size());
    return static_cast<int32_t>(sl.rec.size() / 12);
}

int32_t vcrt_lens_offsets(const vcrt_render_desc* desc, uint32_t first, uint32_t count,
                          float* offsets) {
    vcrt_render_desc d;
    if (!read_desc(desc, d) || !desc_valid(d) || (count > 0 && !offsets) ||
        count > static_cast<uint32_t>(INT32_MAX))
        return VCRT_ERROR_INITIALIZATION_FAILED;
    const vcrt::Camera cm = desc_camera(d);
    for (uint32_t k = 0; k < count; k++) {
        // R == 0: the pinhole, +0 (the products of a zero radius would carry the sines' signs)
        const vcrt::f3 o = d.lens_radius > 0.0f
                               ? vcrt::lens_offset(first + k, d.lens_radius, cm.u, cm.v)
                               : vcrt::mk(0.0f, 0.0f, 0.0f);
        float* out = offsets + 3 * static_cast<size_t>(k);
        out[0] = o.x;
        out[1] = o.y;
        out[2] = o.z;
    }
    return static_cast<int32_t>(count);
}

int32_t vcrt_frame_rays(const vcrt_render_desc* desc, const int32_t* xy, int32_t npixels,
                        uint32_t first, uint32_t n, float* origins, float* dirs) {
    vcrt_render_desc d;
    if (!read_desc(desc, d) || !desc_valid(d) || npixels < 0 ||
        (npixels > 0 && (!xy || !origins || !dirs)))
        return VCRT_ERROR_INITIALIZATION_FAILED;
    if (n == 0 || static_cast<uint64_t>(first) + n > (uint64_t{1} << 19))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    for (int32_t p = 0; p < npixels; p++)
        if (xy[2 * p] < 0 || xy[2 * p] >= d.width || xy[2 * p + 1] < 0 || xy[2 * p + 1] >= d.height)
            return VCRT_ERROR_INITIALIZATION_FAILED;
    const vcrt::Camera cm = desc_camera(d);
    // per sample index: the jitter term (tracer.hip viewport_jitter) and the ray's origin
    std::vector<float2> jt(n);
    make_jitter(first, static_cast<int>(n), jt.data());
    std::vector<vcrt::f3> term(n), origin(n);
    for (uint32_t k = 0; k < n; k++) {
        term[k] = vcrt::add(vcrt::scale(jt[k].x, cm.delta_u), vcrt::scale(jt[k].y, cm.delta_v));
        origin[k] = d.lens_radius > 0.0f
                        ? vcrt::add(cm.center,
                                    vcrt::lens_offset(first + k, d.lens_radius, cm.u, cm.v))
                        : cm.center;
    }
    for (int32_t p = 0; p < npixels; p++) {
        // tracer.hip viewport_corner
        const vcrt::f3 corner = vcrt::add(
            vcrt::add(cm.pixel00, vcrt::scale(static_cast<float>(xy[2 * p]), cm.delta_u)),
            vcrt::scale(static_cast<float>(xy[2 * p + 1]), cm.delta_v));
        for (uint32_t k = 0; k < n; k++) {
            const vcrt::f3 dir = vcrt::sub(vcrt::add(corner, term[k]), origin[k]);
            const size_t at = 3 * (static_cast<size_t>(p) * n + k);
            origins[at + 0] = origin[k].x;
            origins[at + 1] = origin[k].y;
            origins[at + 2] = origin[k].z;
            dirs[at + 0] = dir.x;
            dirs[at + 1] = dir.y;
            dirs[at + 2] = dir.z;
        }
    }
    return npixels;
}

int32_t vcrt_ambient_dirs(uint32_t first, uint32_t count, float* out) {
    if (static_cast<uint64_t>(first) + count > (uint64_t{1} << 22))
        return VCRT_ERROR_FORMAT_NOT_SUPPORTED;
    if (count > 0 && !out) return VCRT_ERROR_INITIALIZATION_FAILED;
    for (uint32_t k = 0; k < count; k++) {
        const vcrt::f3 u = vcrt::ambient_dir(first + k);
        out[3 * k + 0] = u.x;
        out[3 * k + 1] = u.y;
        out[3 * k + 2] = u.z;
    }
    return static_cast<int32_t>(count);
}

float vcrt_canonical_sin(float x) { return vcrt::sin_canonical(x); }
float vcrt_canonical_rand(float x, float y) { return vcrt::rand2(x, y); }

const char* vcrt_result_string(vcrt_result r) {
    switch (r) {
        case VCRT_SUCCESS: return "VK_SUCCESS";
        case VCRT_NOT_READY: return "VK_NOT_READY";
        case VCRT_ERROR_OUT_OF_HOST_MEMORY: return "VK_ERROR_OUT_OF_HOST_MEMORY";
        case VCRT_ERROR_OUT_OF_DEVICE_MEMORY: return "VK_ERROR_OUT_OF_DEVICE_MEMORY";
        case VCRT_ERROR_INITIALIZATION_FAILED: return "VK_ERROR_INITIALIZATION_FAILED";
        case VCRT_ERROR_DEVICE_LOST: return "VK_ERROR_DEVICE_LOST";
        case VCRT_ERROR_FEATURE_NOT_PRESENT: return "VK_ERROR_FEATURE_NOT_PRESENT";
        case VCRT_ERROR_FORMAT_NOT_SUPPORTED: return "VK_ERROR_FORMAT_NOT_SUPPORTED";
        case VCRT_ERROR_UNKNOWN: return "VK_ERROR_UNKNOWN";
        case VCRT_ERROR_INCOMPATIBLE_SHADER_BINARY: return "VK_ERROR_INCOMPATIBLE_SHADER_BINARY_EXT";
        default: return "VK_RESULT_UNRECOGNIZED";
    }
}

}  // extern "C"
