/* vcrt.h -- C ABI of the MI355X path tracer (libvcrt.so).
 *
 * This is the drop-in boundary. The reference renders from compile-time constants inside one
 * Vulkan compute dispatch; this ABI carries the same state at run time and replaces:
 *
 *   vcrt_begin            <- VkResult BeginRenderingOperation(void)      include/Renderer.hpp:14
 *                            (storage image Renderer.cpp:433-468, compute pipeline :532-543)
 *   vcrt_draw_next_frame  <- VkResult DrawNextFrame(void)                include/Renderer.hpp:17
 *                            (vkCmdDispatch(W/16,H/16,1) Renderer.cpp:221 + submit :678-686)
 *   vcrt_end              <- VkResult EndRenderingOperation(void)        include/Renderer.hpp:20
 *                            (idempotent teardown, tolerates partial Begin: Renderer.cpp:714-774)
 *   vcrt_shader_load      <- VkResult CreateShaderStageFromFile(...)     include/Shader.hpp:14-15
 *                            (loads the gfx950 code object instead of SPIR-V, Shader.cpp:34-95)
 *   vcrt_set_scene        <- const sphere world[]                        globals.glsl:29-518
 *   vcrt_scene_builtin /
 *   vcrt_scene_generator_text <- SceneGenerator executable stdout        SceneGenerator.cpp:23-56
 *   vcrt_render_desc      <- IMAGE_WIDTH/HEIGHT, SAMPLES_PER_PIXEL, MAX_RECURSION_LEVEL, camera
 *                            globals.glsl:9-24, include/Common.hpp:23-24
 *
 * Added (the reference has no equivalents): read-back of the rgba32f framebuffer, statistics,
 * rank/world tile sharding and the tile re-assembly used after a multi-GPU gather; ray queries
 * on rays the caller supplies (vcrt_trace_rays: radiance and first hit) and occlusion queries
 * (vcrt_occlude_rays: is anything in the way within a per-ray reach); a thin lens for the
 * frames' camera (vcrt_render_desc.lens_radius, vcrt_lens_offsets); a camera that moves between
 * frames without a new vcrt_begin (vcrt_set_camera: the camera-ray lists are rebuilt on the GPU;
 * vcrt_get_camera_stats, vcrt_camera_lists_read); spheres that move between frames without a new
 * vcrt_set_scene (vcrt_update_spheres: the scene's grouping is kept and its tables are refitted
 * on the GPU; vcrt_get_scene_update_stats, vcrt_scene_table_host / _read); the guide buffers of
 * a frame for a denoiser (vcrt_draw_features: first-hit albedo, normal, depth, coverage and
 * sphere id of the frame's own camera rays; vcrt_frame_rays) and its ambient visibility buffer
 * (vcrt_draw_occlusion: the open share of short rays sent from those first hits;
 * vcrt_ambient_dirs); the denoiser those guides are for (vcrt_denoise: an edge-avoiding
 * a-trous filter over a frame and its guide planes; vcrt_denoise_host, vcrt_denoise_scales);
 * temporal accumulation over a reprojection map (vcrt_draw_motion: where each pixel's surface
 * was in the previous frame, vcrt_motion_project; vcrt_reproject: the previous output gathered
 * there and blended with the new frame, vcrt_reproject_host); and the variance-guided link between
 * the two (vcrt_reproject_moments: the accumulation with luminance moments; vcrt_variance: their
 * per-pixel variance; vcrt_denoise_variance: the filter steered by it; their _host forms).
 *
 * Conventions: plain C types and pointers only. Every function returns a VkResult-compatible
 * int32_t (0 = success, negative = error; values from the Vulkan registry). Nothing throws
 * across the ABI. One renderer per process, calls are not reentrant (as in the reference).
 */
#ifndef VCRT_H
#define VCRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t vcrt_result;

/* VkResult values (Vulkan registry), defined locally: there are no Vulkan headers here. */
#define VCRT_SUCCESS 0
#define VCRT_NOT_READY 1
#define VCRT_ERROR_OUT_OF_HOST_MEMORY (-1)
#define VCRT_ERROR_OUT_OF_DEVICE_MEMORY (-2)
#define VCRT_ERROR_INITIALIZATION_FAILED (-3)
#define VCRT_ERROR_DEVICE_LOST (-4)
#define VCRT_ERROR_FEATURE_NOT_PRESENT (-8)
#define VCRT_ERROR_FORMAT_NOT_SUPPORTED (-11)
#define VCRT_ERROR_UNKNOWN (-13)
#define VCRT_ERROR_INCOMPATIBLE_SHADER_BINARY (1000482000) /* VK_..._SHADER_BINARY_EXT */

/* Material ids, textures.glsl:10-12 */
#define VCRT_TEXTURE_LAMBERTIAN 1
#define VCRT_TEXTURE_METAL 2
#define VCRT_TEXTURE_GLASS 3

/* Same field order and size (40 B) as GLSL `struct sphere`, structures.glsl:10-16. */
typedef struct vcrt_sphere {
    float center[3];
    float radius;
    float colour[3];
    float texture[3]; /* x = material id (as float), y = param (ratio / fuzz / eta), z unused */
} vcrt_sphere;

typedef struct vcrt_camera { /* globals.glsl:21-24 */
    float lookfrom[3];
    float lookat[3];
    float vup[3];
    float vfov; /* degrees */
} vcrt_camera;

/* Kernel variants. SMEM: wave-uniform scalar-cache reads of the linear sphere table (measured
 * faster than LDS staging for 485 and 4100 spheres). CULL: spheres grouped
 * spatially in fours, a group is tested only when some ray of the wave may come near it (same
 * results bit for bit; falls back to SMEM below 16 spheres or for unbounded scenes). AUTO =
 * CULL when it applies, else SMEM. */
#define VCRT_KERNEL_AUTO 0
#define VCRT_KERNEL_LDS 1
#define VCRT_KERNEL_SMEM 2
#define VCRT_KERNEL_CULL 3
#define VCRT_KERNEL_CULL_LANE 4 /* CULL with per-lane group tests (LDS or global tables) */
#define VCRT_KERNEL_CULL_FLAT 5 /* CULL_LANE with the exact tests dealt out over the wave */

typedef struct vcrt_render_desc {
    uint32_t struct_size;      /* sizeof(vcrt_render_desc) */
    int32_t width, height;     /* IMAGE_WIDTH, IMAGE_HEIGHT: each <= 65535; a rank's 8x8 tiles
                                * hold <= 2^26 pixels (8192 x 8192 on one GPU), else vcrt_begin
                                * returns VCRT_ERROR_FORMAT_NOT_SUPPORTED */
    int32_t samples_per_pixel; /* SAMPLES_PER_PIXEL, >= 1 */
    int32_t max_depth;         /* MAX_RECURSION_LEVEL, >= 0 */
    vcrt_camera camera;
    int32_t device;        /* HIP device ordinal; -1 = current device */
    int32_t rank;          /* this process's shard of the frame: the 8x8 tiles (tx, ty) with
                              (tx + ty) % world_size == rank, numbered row-major */
    int32_t world_size;    /* number of shards (GPUs) */
    int32_t kernel_variant;
    int32_t blocks_per_cu; /* persistent grid occupancy; 0 = from the occupancy query */
    int32_t accumulate_chunk; /* samples per work item (0 = 64, halved down to 16 while a pixel
                                 has < 16 items, then while the largest rank's share has
                                 < 2^24 - 2^21 items -- unless the desc takes the cost partition:
                                 chunk and tail left to the rules and a kernel variant with a
                                 cost-order build (AUTO, LDS, SMEM, CULL_FLAT), where the second
                                 halving is skipped, the tail is none and the frames run the cost
                                 order; vcrt_work_chunk), rounded up to a multiple of the quantum
                                 below. A scheduling choice only: it does not change the image. */
    int32_t progressive; /* 0: every DrawNextFrame re-renders samples 0..spp-1 (the reference,
                            Linux.cpp:362-366). 1: frame f renders samples f*spp..(f+1)*spp-1 and
                            the framebuffer holds the average of all frames so far (the same
                            image as one render with (f+1)*spp samples and chunk boundaries at
                            every frame; RENDER_ITERATION, Common.hpp:25, was never wired up). */
    const char* code_object_path; /* NULL = vcrt_tracer.hsaco next to libvcrt.so, then embedded */
    int32_t accumulate_tail;      /* the last accumulate_tail samples of every pixel (of every
                                     progressive frame) in chunks of accumulate_tail_chunk, handed
                                     out after all the other work items, so that the items still
                                     running when the queue drains are short. 0 = the rule
                                     (vcrt_work_tail), -1 = none. Part of the chunk partition: it
                                     schedules only; the image depends on the quantum alone. */
    int32_t accumulate_tail_chunk; /* samples per tail item; 0 = the rule. Tail and tail items
                                      are rounded to multiples of the quantum. */
    int32_t accumulate_quantum; /* the accumulation quantum G (a power of two; 0 = the rule,
                                   vcrt_work_quantum: 4, doubled while a pixel would take more
                                   than 512 quanta). A pixel's samples are summed in fp32 in sample
                                   order within each quantum of G consecutive samples (restarting
                                   at every progressive frame); when one quantum covers the pixel
                                   (G >= samples_per_pixel, not progressive) the sum is divided in
                                   fp32, the reference's sequential sum (shader.comp:46-56)
                                   exactly; otherwise every quantum sum is quantized to 2^-s (s per
                                   pixel from its own quantum sums: vcrt_pixel_scale_log2, 32 for
                                   every pixel of the reference scenes) and added exactly. So the
                                   image depends on G only -- not on the
                                   work items, the schedule or the number of GPUs: a sharded frame
                                   equals a one-GPU render bit for bit. Work items hold whole
                                   quanta. At most 512 quanta per pixel (progressive frames
                                   included). */
    float lens_radius; /* thin lens: the radius R of the camera's aperture disk in world units.
                          0 (vcrt_default_desc) = the reference's pinhole, exactly as without the
                          field: the same kernels, camera-ray lists and bits. R > 0: sample index i
                          (absolute: progressive frame f covers f*spp .. (f+1)*spp-1) of every
                          pixel starts at camera centre + offset_i, a point of the disk of radius R
                          in the viewport's plane basis (vcrt_lens_offsets), and aims at the viewport
                          point the pinhole's ray of (x, y, i) passes through:
                            origin_i = center + offset_i
                            dir      = (corner(x, y) + jitter_i) - origin_i
                          each fp32 operation rounded on its own; the pixel is the same
                          accumulation of ray_color(origin_i, dir, max_depth). The viewport lies
                          in the plane through lookat (focal length = |lookfrom - lookat|,
                          shader.comp:21,38), so that plane is in focus: focus by placing lookat on
                          the view axis at the focus distance (there is no separate field).
                          Negative, NaN or infinite: VCRT_ERROR_INITIALIZATION_FAILED.
                          Appended after the first release of this struct: struct_size may be
                          sizeof(vcrt_render_desc) or the size without this field (the field then
                          reads 0). On LP64 targets the field takes the four bytes that padded the
                          struct to its pointer's alignment, so the two sizes are both 112 and a
                          caller built against the older header must have zeroed the whole struct
                          (vcrt_default_desc does). With R > 0 the frame runs the *_lens kernels
                          (vcrt_stats.kernel): AUTO, SMEM and CULL_FLAT; LDS, CULL, CULL_LANE,
                          VCRT_DEBUG_STATS=1 or a code object without the lens kernels give
                          VCRT_ERROR_FEATURE_NOT_PRESENT from vcrt_begin. vcrt_trace_rays and
                          vcrt_occlude_rays take the caller's rays and ignore the lens. */
} vcrt_render_desc;

typedef struct vcrt_stats {
    uint64_t segments;     /* ray segments traced last frame (one full sphere-list scan each) */
    uint64_t sphere_tests; /* segments * nspheres */
    uint64_t samples;      /* local_rows * width * spp */
    double kernel_ms;      /* tracer kernel time, HIP events on the render stream */
    double frame_ms;       /* host wall time of the last vcrt_draw_next_frame */
    double resolve_ms;     /* resolve kernel time (exact chunk sums -> pixels; 0: one chunk) */
    double gather_ms;      /* multi-GPU frame gather + re-interleave (vcrt_comm_init), HIP events */
    int32_t frames;        /* frames drawn since vcrt_begin */
    int32_t grid_blocks, block_threads, kernel_variant;
    int32_t local_tiles;   /* 8x8 tiles this rank renders */
    int32_t nspheres;
    uint32_t lds_bytes;    /* dynamic LDS of the tracer's tables and stacks (without the ring) */
    int32_t accumulate_chunk; /* samples per work item in effect (head) */
    int32_t tables_in_lds;    /* 1 when the culled scan reads its tables from LDS, 2 when only
                                 its boxes (vcrt_trace_cull_flat_boxes) */
    uint64_t accumulated_spp; /* samples per pixel in the framebuffer (progressive: all frames) */
    uint64_t group_tests;  /* groups of four spheres put through the exact test, per wave */
    uint64_t bound_tests;  /* group bounds tested, per wave (CULL variant) */
    char kernel[48];       /* the tracer kernel the last frame launched (its code-object symbol) */
    uint64_t debug[128]; /* diagnostics (VCRT_DEBUG_STATS=1): [0..7] wave-iterations,
                           active-lane sum, hit groups, fetches, last/first wave end time, sum
                           end time, waves; [8..16] wave clock ticks (s_memtime) in the scan,
                           its uniform levels, node / group / candidate passes (CULL_FLAT),
                           candidate passes run, the whole wave, the big list, node pushes,
                           [17..18] shading and sky, block fetch; [19..22] flat passes:
                           entries dealt, live lanes offered, partial passes, passes; [23]
                           the camera fast trace with its shading; [24..31] camera fast
                           trace entries, its lanes, live lanes, listed-group loop trips and
                           lane sum, root loop trips and lane sum; main-scan hit lanes;
                           [32..39] flat scans: wave ticks in the retire, wave-iterations
                           running the fetch loop, block fetches, items started, [36] [37] the
                           entries the LDS-table kernel's group passes and node passes took
                           (vcrt_trace_cull_flat_stats; 0 from the other kernels),
                           wave-iterations running the retire, quanta retired (lanes);
                           [40..127] region counters: wave-level entries into the tracer's
                           counted regions (tracer.hip reg::*, by enum value), summed over
                           the waves */
    int32_t accumulate_tail;       /* tail samples per pixel in effect (0: none) */
    int32_t accumulate_tail_chunk; /* samples per tail item in effect */
    int32_t ring_entries;          /* LDS accumulation ring entries per wave (0: none; the chunk
                                      sums go to global memory directly) */
    int32_t accumulate_quantum;    /* the accumulation quantum G in effect */
    int32_t accumulate_scale_log2; /* the smallest per-pixel quantization scale s of the frame
                                      (vcrt_pixel_scale_log2): 32 unless some pixel's quantum
                                      sums reach 2^12 in magnitude */
    int32_t cost_order;            /* 1: the frame's blocks ran most expensive first (the order
                                      measured by the configuration's first frame; the linear
                                      scans' frames with few items per lane, the cost partition
                                      (accumulate_chunk), or VCRT_WORK_ORDER=cost) */
    int32_t scale_rerenders;       /* renders the last vcrt_draw_next_frame added because a
                                      pixel's quantum sums first reached 2^12 (its scale below 32:
                                      the frame -- progressive: every frame so far -- is rendered
                                      again with each pixel at its own scale) */
} vcrt_stats;

/* Fills *desc with the reference defaults: 1280x720, 1 spp, depth 50, camera
 * (13,2,3)->(0,0,0), vup (0,1,0), vfov 20, rank 0 of 1, stripe 1 (globals.glsl:9-24). */
vcrt_result vcrt_default_desc(vcrt_render_desc* desc);

vcrt_result vcrt_begin(const vcrt_render_desc* desc);
/* The accumulation quantum G that vcrt_begin(desc) uses (the image depends on it alone); host
 * only, no GPU. Negative VkResult for an invalid desc. */
int32_t vcrt_work_quantum(const vcrt_render_desc* desc);
/* Samples per work item of the head that vcrt_begin(desc) uses (a multiple of the quantum);
 * host only, no GPU. Negative VkResult for an invalid desc. */
int32_t vcrt_work_chunk(const vcrt_render_desc* desc);
/* Tail samples per pixel that vcrt_begin(desc) uses (0: none) and, in *tail_chunk, the samples
 * per tail item; host only. The rule: about six head items per lane of the persistent grid,
 * T = 6 * chunk * 327680 / (64 * the largest rank's tiles) rounded to a power of two, in items
 * of max(4, chunk / 8) samples; none when 4 T > samples_per_pixel or chunk >= samples_per_pixel,
 * when the head alone has >= 2 (2^24 - 2^21) items, or for the cost partition (accumulate_chunk).
 * The head ends on a quantum boundary (T is adjusted) and tail items are rounded up to whole
 * quanta. Negative VkResult for an invalid desc. */
int32_t vcrt_work_tail(const vcrt_render_desc* desc, int32_t* tail_chunk);
/* The quantization scale 2^s of a pixel's quantum sums (host only), from E = the largest |S| of
 * its finite quantum sums over every channel (and every progressive frame so far): 32 while
 * E < 2^12 (every pixel of the reference scenes, radiance <= 1 per sample), else the largest s
 * with E * 2^s < 2^44 = 43 - floor(log2 E). Each quantized sum is then an integer below 2^44 and
 * a pixel's (at most 512) of them add exactly in double, whatever the scene's brightness. The
 * renderer measures E while it renders: a frame where some pixel first needs s < 32 is
 * rendered again with every pixel at its own scale (vcrt_stats.scale_rerenders). */
int32_t vcrt_pixel_scale_log2(float max_abs_quantum_sum);
/* Uploads the scene and builds, on the host, its culling tables and the camera-ray lists for
 * this desc's camera and shard (vcrt_cull_tables, vcrt_primary_lists: ~0.1 s for the final
 * scene at 1080p, ~0.4 s for 4100 spheres at 4K). vcrt_begin sets the final scene. */
vcrt_result vcrt_set_scene(const vcrt_sphere* spheres, int32_t count);
vcrt_result vcrt_draw_next_frame(void);
vcrt_result vcrt_end(void);

/* Multi-GPU, one process per GPU (the reference renders on one GPU: Environment.cpp:157-165;
 * "TODO: Cross-GPU sharing", Frontend.cpp:107). Each process calls vcrt_begin with its rank,
 * world_size and device, then vcrt_comm_init with the same id on every rank (rank 0 makes it
 * with vcrt_comm_unique_id and hands it out, e.g. over a TCP store). From then on
 * vcrt_draw_next_frame renders the rank's tiles and gathers every rank's packed tiles to rank 0
 * over RCCL (one grouped send/recv) and re-interleaves them there: on rank 0 it returns with the
 * whole frame, which vcrt_read_framebuffer / vcrt_framebuffer_device then give as [height][width]
 * (the other ranks keep their packed tiles). Collective: every rank must draw every frame.
 * vcrt_end destroys the communicator. */
typedef struct vcrt_comm_id {
    char internal[128]; /* an ncclUniqueId */
} vcrt_comm_id;
vcrt_result vcrt_comm_unique_id(vcrt_comm_id* id);
vcrt_result vcrt_comm_init(const vcrt_comm_id* id);

/* Rank-local framebuffer layout. world_size == 1: the frame, row-major [height][width] (row 0 =
 * top, as the reference's storage image). world_size > 1: packed tiles [tiles][64] with element
 * 8*(y%8) + x%8 of each tile (pixels outside the frame in edge tiles are left untouched). */
vcrt_result vcrt_local_layout(uint32_t* elements, uint32_t* tiles);
/* Copies the rank-local framebuffer (elements * 4 floats, rgba32f) to host memory; count = number
 * of floats available at rgba. */
vcrt_result vcrt_read_framebuffer(float* rgba, size_t count);
/* Device address and size of the framebuffer vcrt_read_framebuffer reads. */
vcrt_result vcrt_framebuffer_device(void** device_ptr, size_t* bytes);
/* Render into caller-owned device memory (>= elements*16 bytes, 16-B aligned); NULL = own.
 * VK_ERROR_FEATURE_NOT_PRESENT after vcrt_comm_init (the gather owns the buffers). */
vcrt_result vcrt_set_framebuffer_device(void* device_ptr, size_t bytes);
/* Rebuild the frame from gathered rank framebuffers: gathered = [world][tiles_per_rank][64]
 * float4 (rank-major, each rank's packed tiles padded to tiles_per_rank), frame = [height][width]
 * float4; both device pointers. Runs on the render stream and returns when done. */
vcrt_result vcrt_assemble_tiles(const void* gathered, void* frame, int32_t width, int32_t height,
                                int32_t world_size, uint32_t tiles_per_rank);
vcrt_result vcrt_get_stats(vcrt_stats* stats);
/* Progressive mode: drop the accumulated frames (sample sequence restarts at 0). */
vcrt_result vcrt_reset_accumulation(void);

/* Moves the camera between frames (added; the reference's camera is compiled in). Requires
 * vcrt_begin; a NULL camera or a call before vcrt_begin returns VCRT_ERROR_INITIALIZATION_FAILED
 * before anything touches the GPU. The camera's values are taken as vcrt_begin takes them (not
 * validated: a degenerate camera renders what it renders there).
 * Every later frame is bit for bit the frame of a fresh renderer -- vcrt_begin with the same
 * description and this camera, then vcrt_set_scene of the current scene -- vcrt_stats.segments and
 * .kernel, the thin lens's frames and a later vcrt_set_scene included. Kept: the device, stream
 * and code object, the scene and its culling tables, the framebuffers (a caller's
 * vcrt_set_framebuffer_device too; the last frame stays in them until the next draw) and the
 * communicator. Rebuilt: the pixel corners, the lens origins, both camera-ray lists and the
 * camera-relative records. Reset: progressive accumulation restarts at sample 0 and the measured
 * cost order is dropped. vcrt_trace_rays and vcrt_occlude_rays do not depend on the camera.
 * The lists are built on the GPU by the camera-list kernels (csrc/camera_lists.hip), the very
 * bytes vcrt_primary_lists / vcrt_primary_sphere_lists give for the new description, in buffers
 * that are kept and only grow. VCRT_CAMERA_LISTS=host in the environment runs the host builders
 * instead, and so does a code object without those kernels (an A/B build of an older tree).
 * Local, not collective: under vcrt_comm_init every rank calls it with the same camera before
 * the next draw. */
vcrt_result vcrt_set_camera(const vcrt_camera* camera);

/* The last vcrt_set_camera (all zero before the first). */
typedef struct vcrt_camera_stats {
    double   host_ms;       /* wall time of the call */
    double   lists_ms;      /* HIP events around the list kernels, the 8-byte read-back of the
                               totals between them included; 0 with the host builders */
    int32_t  on_device;     /* 1: the camera-list kernels built the lists; 0: the host, or the
                               renderer has no lists */
    int32_t  reserved;      /* 0 */
    uint64_t quarters;      /* 4 x local tiles (0: no lists) */
    uint64_t group_ids;     /* entries of the group lists */
    uint64_t pair_records;  /* pair records of the sphere lists */
} vcrt_camera_stats;
vcrt_result vcrt_get_camera_stats(vcrt_camera_stats* stats);

/* Moves the spheres between frames (added): the whole array replaces the current scene's values
 * -- centres, radii, colours and materials -- at the cost of a few small kernels, not of
 * vcrt_set_scene. `count` must equal the current scene's (VCRT_ERROR_FORMAT_NOT_SUPPORTED
 * otherwise, nothing changed); before vcrt_begin, or for NULL with count > 0,
 * VCRT_ERROR_INITIALIZATION_FAILED before anything touches the GPU. vcrt_update_spheres takes a
 * host pointer; vcrt_update_spheres_device a device pointer (40 B per sphere, readable on the
 * renderer's device), waits on nothing but the render stream and returns when done.
 * Every later frame and every later vcrt_trace_rays / vcrt_occlude_rays gives, bit for bit, the
 * result of a fresh renderer -- vcrt_begin with the same description and the current camera,
 * then vcrt_set_scene(spheres, count) -- vcrt_stats.segments included. vcrt_stats.kernel follows
 * the refitted tables and may differ from the fresh renderer's.
 * Kept: the device, stream and code object, the framebuffers, the communicator, every scene
 * buffer and the scene's grouping: the members of the big list and of every hierarchy group
 * (the index words of the group records). Rewritten in place, on the GPU by the kernels of
 * csrc/scene_update.hip: the linear scan table, the per-sphere rows, the group records' geometry,
 * the group, node and chunk boxes in both layouts, the node and group footprint tables, and --
 * through vcrt_set_camera's list kernels -- both camera-ray lists and the camera-relative
 * records. Recomputed on the host from a summary the kernels reduce (one small read-back): the
 * box margins, the shared y slab, the footprint scalars and the kernel selection. Reset:
 * progressive accumulation restarts at sample 0 and the measured cost order is dropped. Once the
 * kept buffers exist the call allocates and frees no device memory.
 * The grouping does not follow the spheres: the boxes are the members' boxes wherever the members
 * go, so the culled scans stay exact, but after large moves the boxes grow and overlap and frames
 * get slower, never wrong. vcrt_set_scene remains the rebuild: call it when the scene has moved
 * far from where it was grouped.
 * When the refit does not apply, the call does what vcrt_set_scene does with the new values (the
 * device variant first copies them to the host) and reports rebuilt = 1: a renderer without
 * culling tables (fewer than 16 spheres, or an unbounded scene), a new centre or radius that
 * fails |v| <= 2^30 (NaN included), or a code object without the refit kernels (an A/B build of
 * an older tree). VCRT_SCENE_UPDATE=host in the environment refits on the host instead
 * (vcrt_scene_table_host's function) and uploads into the kept buffers (A/B runs and tests).
 * Local, not collective, like vcrt_set_camera. */
vcrt_result vcrt_update_spheres(const vcrt_sphere* spheres, int32_t count);
vcrt_result vcrt_update_spheres_device(const vcrt_sphere* spheres, int32_t count);

/* The last vcrt_update_spheres[_device] (all zero before the first). */
typedef struct vcrt_scene_update_stats {
    double   host_ms;          /* wall time of the call */
    double   refit_ms;         /* HIP events around the refit kernels and the summary's read-back;
                                  0 when the host refitted or the scene was rebuilt */
    double   lists_ms;         /* the camera-list kernels (vcrt_camera_stats.lists_ms); 0: none */
    int32_t  on_device;        /* 1: the refit kernels wrote the tables */
    int32_t  rebuilt;          /* 1: the refit did not apply; the call ran vcrt_set_scene */
    uint64_t groups;           /* group records rewritten (big groups included) */
    uint64_t boxes;            /* group, node and chunk boxes rewritten */
    uint64_t footprint_cells;  /* cells of the node and group footprint tables rewritten */
} vcrt_scene_update_stats;
vcrt_result vcrt_get_scene_update_stats(vcrt_scene_update_stats* stats);

/* Diagnostics: one device table of a scene, as bytes in the device's layout. */
#define VCRT_TABLE_LINEAR        0  /* the linear scan table, padding and prefetch group included */
#define VCRT_TABLE_CENTER_RADIUS 1  /* [count][4] */
#define VCRT_TABLE_SHADE         2  /* [count][4] */
#define VCRT_TABLE_MATERIAL      3  /* [count][4] */
#define VCRT_TABLE_GROUPS        4  /* [big + hierarchy groups][20]: geometry, 4 index words */
#define VCRT_TABLE_BOUND         5  /* group-pair boxes, pair-SoA */
#define VCRT_TABLE_BOUND_NF      6  /* the same, near/far layout */
#define VCRT_TABLE_NODE          7
#define VCRT_TABLE_NODE_NF       8  /* padded to whole chunks */
#define VCRT_TABLE_TOP           9
#define VCRT_TABLE_FOOT         10  /* the node footprint tables, packed as the kernel reads them */
#define VCRT_TABLE_GROUP_FOOT   11
#define VCRT_TABLE_SCALARS      12  /* a vcrt_scene_scalars */
typedef struct vcrt_scene_scalars {
    int32_t  nbig, ngroups;
    float    margin[4];
    int32_t  slab_on;
    float    slab[2];
    float    fp_x[2], fp_z[2], fp_y[2], fp_k2;
    uint32_t fp_always;
    uint32_t gf_n;
    float    gf_x[2], gf_z[2], gf_k2;
    uint32_t gf_always[4];
    int32_t  gf_ok;
    int32_t  bounded, radii_safe;
} vcrt_scene_scalars;
/* The bytes of one device table as a refit computes them on the host: the grouping
 * vcrt_set_scene(grouping_of) chooses, filled with the values of `values` (same count; with
 * values == grouping_of exactly what vcrt_set_scene uploads). Returns the size in bytes (writes
 * when cap suffices), 0 when the table does not exist (no culling tables; no group footprint). */
int64_t vcrt_scene_table_host(const vcrt_sphere* grouping_of, const vcrt_sphere* values,
                              int32_t count, int32_t table, void* buf, size_t cap);
/* The same table copied back from the renderer's device buffers, whoever wrote it (a negative
 * VkResult before vcrt_begin). */
int64_t vcrt_scene_table_read(int32_t table, void* buf, size_t cap);

/* vcrt_primary_lists / vcrt_primary_sphere_lists (below) over refitted tables: the grouping of
 * `grouping_of` filled with the values of `spheres`, as vcrt_scene_table_host. */
int32_t vcrt_refit_primary_lists(const vcrt_sphere* grouping_of, const vcrt_sphere* spheres,
                                 int32_t count, const vcrt_render_desc* desc, uint32_t* info,
                                 int32_t cap_tiles, uint16_t* ids, int32_t cap_ids);
int32_t vcrt_refit_primary_sphere_lists(const vcrt_sphere* grouping_of, const vcrt_sphere* spheres,
                                        int32_t count, const vcrt_render_desc* desc,
                                        uint32_t* info, int32_t cap_tiles, float* rec,
                                        int32_t cap_floats);

/* Diagnostic: the camera-ray lists the next frame will use, copied back from the device in the
 * form of the two host functions below (vcrt_primary_lists: group_info, ids;
 * vcrt_primary_sphere_lists: sphere_info, rec), whoever built them: the host at vcrt_begin /
 * vcrt_set_scene, or vcrt_set_camera. Returns the entries of each info (4 x local tiles), 0 when
 * the renderer has no lists (no culling tables, a lens, VCRT_PRIMARY_LISTS=0), or a negative
 * VkResult before vcrt_begin; *num_ids and *num_pairs receive the sizes. Writes the infos when
 * cap_entries, ids when cap_ids and rec when cap_floats (12 per pair) are large enough; any
 * pointer may be NULL. */
int32_t vcrt_camera_lists_read(uint32_t* group_info, uint32_t* sphere_info, int32_t cap_entries,
                               uint16_t* ids, int32_t cap_ids, float* rec, int32_t cap_floats,
                               int32_t* num_ids, int32_t* num_pairs);
/* The rank-local framebuffer encoded as sRGB8 RGBA (alpha linear), as the reference's
 * B8G8R8A8_SRGB swapchain stores it at present time (Frontend.cpp:43; shader.frag:14 copies the
 * texel): channel byte = round-to-nearest of 255 * sRGB(clamp(c, 0, 1)). bytes >= elements*4. */
vcrt_result vcrt_read_framebuffer_srgb8(uint8_t* rgba8, size_t bytes);
/* The 255 ascending linear thresholds behind that encode (byte = #{k : c >= t[k]}). */
void vcrt_srgb8_thresholds(float thresholds[255]);

/* Ray queries: the radiance (ray_color, functions.glsl:65-92) and the first hit of rays the caller
 * supplies, against the scene of the last vcrt_set_scene -- any camera model, picking, probes
 * (the frame's own albedo and normal buffers: vcrt_draw_features). Added (the reference traces
 * its own camera's rays only). */
typedef struct vcrt_ray_hit {   /* 32 B; the path's first segment */
    float    t;          /* accepted root; the reference's `infinity` (globals.glsl:26) when sphere < 0 */
    int32_t  sphere;     /* index into the array given to vcrt_set_scene; -1: sky, or max_depth == 0 */
    uint32_t segments;   /* sphere-list scans this ray's path ran, 0..max_depth */
    uint32_t reserved;   /* 0 */
    float    normal[3];  /* (point - centre) / radius as functions.glsl:33-35 computes it: not flipped,
                            not renormalised; 0 when sphere < 0 */
    float    reserved2;  /* 0 */
} vcrt_ray_hit;

typedef struct vcrt_ray_stats {
    uint64_t segments;     /* sum over the batch */
    uint64_t group_tests;  /* as vcrt_stats: groups of four put through the exact test, per wave */
    uint64_t bound_tests;  /* group/node/chunk boxes tested, per wave (0: the linear scan only) */
    double   kernel_ms;    /* HIP events on the render stream */
    char     kernel[48];   /* code-object symbol that ran */
} vcrt_ray_stats;

/* origins, dirs: [count][3] floats, packed. radiance: [count][4] floats (rgb = ray_color, a = 1).
 * radiance or hits may be NULL (not both); stats may be NULL. Host pointers; staged through device
 * buffers that are kept (and grown) between calls and freed by vcrt_end.
 *
 * For a ray of six finite components and a direction that is not all zero, rgb and segments are
 * ray_color's for (origin, dir, max_depth) bit for bit, and t, sphere and normal those of its
 * first hit_sphere scan (strict <, the earliest index on ties); max_depth == 0 gives radiance 0,
 * 0 segments and sphere -1. Any other ray is traced without a fault: its result is deterministic,
 * otherwise unspecified, and changes no other ray's. Results do not depend on the order of the
 * batch, on how it is split over calls, on the description's rank, world_size or kernel_variant,
 * or on vcrt_comm_init (the call is local, not collective). The framebuffer, the progressive
 * accumulation, vcrt_stats and the cost order are left alone: a frame drawn after a query has the
 * bits it would have had without it. Exactly count entries of each output are written; count == 0
 * succeeds and writes nothing.
 * Errors: VCRT_ERROR_INITIALIZATION_FAILED before vcrt_begin, for NULL inputs with count > 0 and
 * when both outputs are NULL; VCRT_ERROR_FORMAT_NOT_SUPPORTED for max_depth < 0 or count > 2^30;
 * VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object has no vcrt_trace_rays kernel (an
 * A/B build of an older tree). */
vcrt_result vcrt_trace_rays(const float* origins, const float* dirs, uint32_t count,
                            int32_t max_depth, float* radiance, vcrt_ray_hit* hits,
                            vcrt_ray_stats* stats);
/* The same with device pointers (16-B aligned outputs, else VCRT_ERROR_INITIALIZATION_FAILED), on
 * the render stream; returns when done. */
vcrt_result vcrt_trace_rays_device(const float* origins, const float* dirs, uint32_t count,
                                   int32_t max_depth, float* radiance, vcrt_ray_hit* hits,
                                   vcrt_ray_stats* stats);

/* Occlusion queries: is anything in the way within a ray's reach? Shadow rays, ambient occlusion,
 * line of sight, probe visibility. Added.
 * origins, dirs: [count][3] floats, packed; dirs are not normalised and t is in units of dir, as
 * in the reference. tmax: [count] floats, each ray's reach T, or NULL: the reference's `infinity`
 * (1e5, globals.glsl:26) for every ray. occluded: [count] bytes. stats may be NULL.
 *
 * occluded[i] = 1 iff hit_sphere (functions.glsl:14-40) with min_t = 0.001 and max_t = T accepts
 * some sphere of the array given to vcrt_set_scene, every fp32 operation rounded on its own in
 * the reference's order; else 0: one bit per ray, bit for bit. With tmax NULL, occluded[i] ==
 * (the first hit of vcrt_trace_rays has sphere >= 0). T may be any float that is not NaN:
 * T <= 0.001 gives 0; +inf and values above 1e5 are allowed and see hits the first-hit query
 * cannot. This holds for rays of six finite components, a direction that is not all zero and a
 * T that is not NaN; any other ray is traced without a fault and writes 0 or 1, deterministic,
 * otherwise unspecified, changing no other ray's answer. As for vcrt_trace_rays, results do not
 * depend on the order of the batch, on how it is split over calls, on the description's rank,
 * world_size or kernel_variant, or on vcrt_comm_init; the framebuffer, the progressive
 * accumulation, vcrt_stats and the cost order are left alone; exactly count bytes are written;
 * count == 0 succeeds and writes nothing.
 * stats: segments = count (one scan per ray), group_tests and bound_tests as for vcrt_trace_rays
 * (a scan stops once every ray of its wave is occluded), kernel = "vcrt_occlude_rays".
 * Host pointers; staged through device buffers that are kept (and grown) between calls and freed
 * by vcrt_end.
 * Errors: VCRT_ERROR_INITIALIZATION_FAILED before vcrt_begin and for NULL origins, dirs or
 * occluded with count > 0; VCRT_ERROR_FORMAT_NOT_SUPPORTED for count > 2^30;
 * VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object has no vcrt_occlude_rays kernel (an
 * A/B build of an older tree). */
vcrt_result vcrt_occlude_rays(const float* origins, const float* dirs, const float* tmax,
                              uint32_t count, uint8_t* occluded, vcrt_ray_stats* stats);
/* The same with device pointers (no alignment requirement), on the render stream; returns when
 * done. */
vcrt_result vcrt_occlude_rays_device(const float* origins, const float* dirs, const float* tmax,
                                     uint32_t count, uint8_t* occluded, vcrt_ray_stats* stats);

/* Feature buffers: the guide images a denoiser wants, of the frame's own camera rays -- first-hit
 * albedo, normal and depth, a coverage channel and a sphere id for edge stopping and picking --
 * generated on the GPU from the renderer's camera, jitter and lens, averaged per pixel in a fixed
 * order, in the framebuffer's layout. Added.
 *
 * For a local pixel (x, y) and the sample indices i = first .. first + n - 1, ray_i(x, y) is
 * exactly the ray the frame traces for sample index i (absolute, as lens_radius counts them):
 *   pinhole:          origin = camera centre,        dir = (corner(x, y) + jitter_i) - centre
 *   lens_radius > 0:  origin_i = centre + offset_i,  dir = (corner(x, y) + jitter_i) - origin_i
 * (vcrt_lens_offsets; corner = pixel00 + x delta_u + y delta_v and jitter_i = jx delta_u + jy
 * delta_v of shader.comp:43-49), every fp32 operation rounded on its own: vcrt_frame_rays is this
 * definition as code. (t_i, s_i, normal_i) is the first hit_sphere scan of that ray, what
 * vcrt_trace_rays reports in vcrt_ray_hit: strict <, the earliest index on ties, normal = (point -
 * centre) / radius, not flipped, not renormalised. Per sample:
 *   a_i  the albedo: sky (s_i < 0): sky_factor(d.y / length(d)), i.e. ray_color(origin, dir, 1)
 *        of a miss; glass (material id 3): (1, 1, 1); anything else: the sphere's colour as
 *        stored, without texture[1]
 *   n_i  normal_i, or 0 for the sky
 *   z_i  t_i, or 0 for the sky; t is in units of dir: for the pinhole the viewport point is at
 *        t = 1, so z x focal length is planar depth
 *   c_i  1 on a hit, else 0
 * Outputs, each [elements] in the rank-local framebuffer layout (vcrt_local_layout: world 1
 * [height][width]; world > 1 packed tiles [tiles][64], slots outside the frame left untouched; the
 * float4 planes go through vcrt_assemble_tiles as frames do):
 *   albedo        float4: rgb = (sum a_i) / n, a = (sum c_i) / n
 *   normal_depth  float4: xyz = (sum n_i) / n, w = (sum z_i) / n
 *   sphere        int32:  s of sample index `first` (-1: sky)
 * Every sum is an fp32 sum that starts at +0 and adds in sample order, divided once by (float)n
 * with correctly rounded division. One lane owns a pixel and runs its samples in order, so the
 * bits depend on (desc, camera, scene, first, n) only -- not on the schedule, on kernel_variant,
 * or on which scan served a ray (the camera-ray lists where the frame has them, else the scans of
 * vcrt_trace_rays; VCRT_FEATURE_LISTS=0 in the environment turns the list route off: A/B runs and
 * tests). The contract holds wherever the frame's does: a bounded scene and a finite camera;
 * anything else is traced without a fault, deterministic, otherwise unspecified.
 *
 * Any output may be NULL, but not all three; stats may be NULL. The call is local, not collective,
 * runs on the render stream and returns when done. It leaves alone the framebuffer, the
 * progressive accumulation, vcrt_stats, the measured cost order and the frame's jitter and lens
 * tables: it builds the jitter terms and lens origins of its own index range, with the kernel and
 * host functions the frame uses, into buffers of its own that are kept, only grown, and freed by
 * vcrt_end. After vcrt_set_camera, vcrt_update_spheres and vcrt_set_scene it sees the new state.
 * vcrt_draw_features takes host pointers (staged through device buffers kept between calls);
 * vcrt_draw_features_device device pointers, the float4 planes 16-B aligned.
 * Errors: VCRT_ERROR_INITIALIZATION_FAILED, before anything touches the GPU, before vcrt_begin,
 * when all three outputs are NULL and for a misaligned device plane;
 * VCRT_ERROR_FORMAT_NOT_SUPPORTED for n == 0 or first + n > 2^19 (the index bound of
 * vcrt_lens_offsets), checked before the renderer's state, so it reads the same before
 * vcrt_begin; VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object has no
 * vcrt_frame_features kernel (an A/B build of an older tree). */
typedef struct vcrt_feature_stats {
    uint64_t rays;          /* valid local pixels * n */
    uint64_t listed_rays;   /* rays answered from the camera-ray lists */
    uint64_t group_tests;   /* as vcrt_ray_stats */
    uint64_t bound_tests;
    double   kernel_ms;     /* the feature kernel, HIP events on the render stream */
    double   host_ms;       /* wall time of the call */
    char     kernel[48];    /* code-object symbol that ran */
} vcrt_feature_stats;
vcrt_result vcrt_draw_features(uint32_t first, uint32_t n, float* albedo, float* normal_depth,
                               int32_t* sphere, vcrt_feature_stats* stats);
vcrt_result vcrt_draw_features_device(uint32_t first, uint32_t n, float* albedo,
                                      float* normal_depth, int32_t* sphere,
                                      vcrt_feature_stats* stats);
/* The frame's rays of listed pixels, the definition above as code (host only, no GPU): for pixel
 * p = (xy[2 p], xy[2 p + 1]) of the whole frame and sample index first + k, k < n, origins and
 * dirs [(p * n + k) * 3 ..] receive ray_{first + k}(x, y) of desc's camera and lens. Returns
 * npixels, or a negative VkResult: VCRT_ERROR_INITIALIZATION_FAILED for an invalid desc, a
 * negative npixels, a NULL pointer with npixels > 0 or a pixel outside the frame;
 * VCRT_ERROR_FORMAT_NOT_SUPPORTED for n == 0 or first + n > 2^19. */
int32_t vcrt_frame_rays(const vcrt_render_desc* desc, const int32_t* xy, int32_t npixels,
                        uint32_t first, uint32_t n, float* origins /* [npixels][n][3] */,
                        float* dirs /* [npixels][n][3] */);

/* The ambient visibility buffer: for every pixel the share of short any-hit rays, sent from the
 * first hits of the frame's own camera rays over the hemisphere, that nothing stops -- the usual
 * companion of albedo, normal and depth as a denoiser guide, and with albedo the cheap preview
 * shading of an editor (vcrt_set_camera, vcrt_update_spheres). The camera rays, their first hits
 * and the secondary rays are generated on the GPU in one kernel; nothing per ray is uploaded.
 * Added.
 *
 * For a local pixel (x, y) and the sample indices i = first .. first + n - 1, ray_i(x, y) =
 * (o_i, d_i) is vcrt_draw_features' ray (vcrt_frame_rays) and (t_i, s_i, normal_i) its first hit
 * as vcrt_ray_hit reports it. A sample that hits (s_i >= 0) sends m secondary rays, k < m, every
 * fp32 operation rounded on its own, no contraction:
 *   P   = o_i + t_i * d_i                       per component, the product then the sum
 *   dn  = d.x n.x + d.y n.y + d.z n.z           summed left to right
 *   N   = dn > 0 ? -normal_i : normal_i         the normal turned against the ray
 *   u   = u_j, j = i * m + k                    vcrt_ambient_dirs, below
 *   d'  = N + u                                 the reference's Lambertian lobe: normal + unit
 *   open_{i,k} = !occluded(P, d', reach)        vcrt_occlude_rays' predicate: hit_sphere with
 *                                               min_t = 0.001 and max_t = reach, t in units of d'
 * u_j (vcrt_ambient_dirs: host only, no GPU), fj = (float)j:
 *   a = rand(fj, fj + 0.5f), b = rand(fj + 0.5f, fj)      vcrt_canonical_rand
 *   zc = 1 - 2 a, rr = sqrtf(max(0, 1 - zc zc)), phi = 6.2831855f * b
 *   u = (rr sin(phi + 1.5707964f), rr sin(phi), zc)       vcrt_canonical_sin
 * the lens offsets' recipe on a sphere, sqrtf correctly rounded.
 * Output: visibility, float4 [elements] in the rank-local framebuffer layout (it goes through
 * vcrt_assemble_tiles and the image writers as a frame does; slots outside the frame are left
 * untouched). With C the number of samples that hit and U the number of open secondary rays over
 * them, both integers:
 *   rgb = (float)(U + m (n - C)) / (float)(n m)       a sky sample counts as fully open
 *   a   = (float)C / (float)n                          the coverage, vcrt_draw_features' albedo.a
 * one correctly rounded division each. The sums are integer counts, so the bits depend on (desc,
 * camera, scene, first, n, m, reach) only: not on which lane took which ray, on the route that
 * served a first hit (VCRT_FEATURE_LISTS) or on kernel_variant. The contract holds where the
 * frame's does and for d' not all zero and a finite normal; anything else is traced without a
 * fault, deterministic, otherwise unspecified.
 *
 * stats may be NULL. The call is local, not collective, runs on the render stream and returns
 * when done. It leaves alone the framebuffer, the progressive accumulation, vcrt_stats, the
 * measured cost order and the frame's jitter and lens tables (it shares vcrt_draw_features' own
 * tables and keeps a u_j table and a staging plane, only grown, freed by vcrt_end). After
 * vcrt_set_camera, vcrt_update_spheres and vcrt_set_scene it sees the new state.
 * vcrt_draw_occlusion takes a host pointer, vcrt_draw_occlusion_device a device pointer, 16-B
 * aligned.
 * Errors: VCRT_ERROR_FORMAT_NOT_SUPPORTED unless 1 <= m <= 256, n >= 1, first + n <= 2^19,
 * n m <= 4096 and (first + n) m <= 2^22 (every j + 0.5f is then exact), checked before the
 * renderer's state, so it reads the same before vcrt_begin; VCRT_ERROR_INITIALIZATION_FAILED,
 * before anything touches the GPU, for a NULL plane, a NaN reach (any other float is taken:
 * +inf, and reach <= 0.001 leaves every ray open), a misaligned device plane and before
 * vcrt_begin; VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object has no
 * vcrt_frame_occlusion kernel (an A/B build of an older tree). */
typedef struct vcrt_occlusion_buffer_stats {
    uint64_t rays;            /* valid local pixels * n */
    uint64_t hit_rays;        /* of them, the samples that hit a sphere */
    uint64_t secondary_rays;  /* hit_rays * m */
    uint64_t occluded;        /* secondary rays that something stops */
    uint64_t listed_rays;     /* camera rays answered from the camera-ray lists */
    uint64_t group_tests;     /* as vcrt_ray_stats, the camera and the secondary rays together */
    uint64_t bound_tests;
    double   kernel_ms;       /* the kernel, HIP events on the render stream */
    double   host_ms;         /* wall time of the call */
    char     kernel[48];      /* code-object symbol that ran */
} vcrt_occlusion_buffer_stats;
vcrt_result vcrt_draw_occlusion(uint32_t first, uint32_t n, uint32_t m, float reach,
                                float* visibility, vcrt_occlusion_buffer_stats* stats);
vcrt_result vcrt_draw_occlusion_device(uint32_t first, uint32_t n, uint32_t m, float reach,
                                       float* visibility, vcrt_occlusion_buffer_stats* stats);
/* u_j of j = first .. first + count - 1, the definition above as code (host only, no GPU), into
 * out [count][3]. Returns count, or a negative VkResult: VCRT_ERROR_FORMAT_NOT_SUPPORTED for
 * first + count > 2^22, VCRT_ERROR_INITIALIZATION_FAILED for a NULL out with count > 0. */
int32_t vcrt_ambient_dirs(uint32_t first, uint32_t count, float* out /* [count][3] */);

/* The denoiser those guide buffers are for: an edge-avoiding a-trous wavelet filter (Dammertz,
 * Sewtz, Hanika, Lensch 2010) over a frame, albedo-demodulated, steered by vcrt_draw_features'
 * planes. A pure image function of the caller's planes: a one-GPU framebuffer, or rank 0's
 * assembled frame with guides put through vcrt_assemble_tiles. Added.
 *
 * Inputs, each [height][width] float4, row 0 at the top: colour, a frame (its alpha is carried
 * through untouched); albedo and normal_depth exactly as vcrt_draw_features writes them, either
 * may be NULL, which switches off the terms that use it. Output: one float4 plane of that shape.
 *
 * Scales, computed once on the host in fp32 (vcrt_denoise_scales is this as code):
 *   k_X  = 1.0f / (sigma_X * sigma_X)   the product, then a correctly rounded division;
 *          0 when sigma_X == 0
 *   kl_l = k_colour * 4^l                exact: sigma_colour halves every pass
 * A term is ON when its k is not 0 and its plane is there (normal and depth: normal_depth;
 * albedo: albedo; colour: always there). A term that is off is the constant +0 and is not
 * evaluated, so "off" and "k = 0" give the same bits.
 *
 * Pass 0 input, eps = 0x1p-10f: with demodulate != 0 and a non-NULL albedo
 *   s_0.c = colour.c / fmaxf(albedo.c, eps)    per rgb channel, correctly rounded
 * otherwise s_0 = colour.
 * Pass l = 0 .. levels - 1, for pixel p = (x, y), step = 1 << l: the taps q = (x + step dx,
 * y + step dy) for dx, dy in -2 .. 2 are visited with dy outer and dx inner, both ascending; a
 * tap outside the frame is skipped (not clamped, not mirrored). Every fp32 operation is rounded on
 * its own, no contraction:
 *   h   = k5[dx + 2] * k5[dy + 2]          k5 = {1/16, 1/4, 3/8, 1/4, 1/16} (products exact)
 *   dn  = sum over x, y, z    of (n_p - n_q)^2   left to right     (normal_depth.xyz)
 *   rz  = (z_p - z_q) / ((fabsf(z_p) + fabsf(z_q)) + 0x1p-20f)     (normal_depth.w)
 *   da  = sum over r, g, b, a of (a_p - a_q)^2   left to right     (albedo, coverage included)
 *   dl  = sum over r, g, b    of (s_p - s_q)^2   left to right     (this pass's input)
 *   X   = ((dn * k_normal + (rz * rz) * k_depth) + da * k_albedo) + dl * kl_l
 *         (each product an ON term, else +0)
 *   e   = 1.0f - fminf(X, 1.0f)
 *   w   = h * (e * e)
 *   acc.c += w * s_q.c   (rgb),   wsum += w          both start at +0
 *   s_{l+1}(p).c = acc.c / wsum                      correctly rounded
 * The centre tap has X = 0 and w = 9/64, so wsum > 0. The weight is a compact polynomial on
 * purpose: no exp, so every bit is reproducible on the host.
 * Final: out.c = s_levels.c * fmaxf(albedo.c, eps) when pass 0 demodulated, else s_levels.c;
 * out.a = colour.a.
 * One lane owns one output pixel and runs its 25 taps in that order, so the bits depend on the
 * planes and the parameters only -- not on the launch shape, and not on which passes stage
 * their footprint in LDS (VCRT_DENOISE_LDS below). The contract holds for finite planes whose
 * s_0 is finite; anything else is filtered without a fault, deterministic, otherwise unspecified
 * (a tap whose guide terms alone reach 1 has w = 0 and its colour is not read).
 *
 * vcrt_denoise_host is the definition as code (host only, no GPU; csrc/denoise.cpp).
 * vcrt_denoise takes host pointers, staged through device planes that are kept, only grown, and
 * freed by vcrt_end; vcrt_denoise_device device pointers, 16-B aligned, readable on the
 * renderer's device. Both need vcrt_begin for the device, the stream and the code object, run one
 * launch of vcrt_denoise_pass per pass on the render stream -- pass 0 fuses the demodulation, the
 * last pass the re-modulation, the passes between go through two scratch planes kept likewise --
 * and return when done. They leave alone the framebuffer, the accumulation, vcrt_stats and the
 * cost order: a frame drawn after a denoise has the bits it would have had without it. The
 * planes' size need not be the renderer's.
 * VCRT_DENOISE_LDS=N in the environment (read at every call): the first N passes, at most the two
 * of step 1 and 2, stage their workgroup's footprint with its halo of 2 step in LDS; unset = 2,
 * the measured choice (profiles/denoise.json); 0 = every pass reads its taps directly. Same bits.
 * Errors: VCRT_ERROR_FORMAT_NOT_SUPPORTED, checked first, so it reads the same before vcrt_begin:
 * a struct_size that is not sizeof(vcrt_denoise_params), levels outside 1 .. 8, a NaN, negative
 * or infinite sigma, a sigma so small that its k (kl_l of the last pass for the colour) is not
 * finite, width or height outside 1 .. 65535, more than 2^26 pixels.
 * VCRT_ERROR_INITIALIZATION_FAILED, before anything touches the GPU: a NULL colour or out, out
 * equal to an input pointer, a misaligned device plane, and (not vcrt_denoise_host) before
 * vcrt_begin. demodulate or sigma_albedo > 0 with a NULL albedo is not an error: those terms are
 * off. VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object has no vcrt_denoise_pass kernel
 * (an A/B build of an older tree). A NULL params takes vcrt_default_denoise_params. */
typedef struct vcrt_denoise_params {
    uint32_t struct_size;   /* sizeof(vcrt_denoise_params) */
    int32_t  levels;        /* 1..8: passes, pass l = 0..levels-1 has tap spacing 2^l */
    float    sigma_normal;  /* 0 = term off, for each sigma */
    float    sigma_depth;   /* relative depth */
    float    sigma_albedo;
    float    sigma_colour;  /* on the filtered signal itself; halves every pass */
    int32_t  demodulate;    /* 1: filter colour / albedo, multiply back at the end */
} vcrt_denoise_params;
/* The defaults: the sigmas that minimise the error of the denoised 4-spp final scene against its
 * 256-spp frame over a small grid (profiles/denoise_defaults.json). */
vcrt_result vcrt_default_denoise_params(vcrt_denoise_params* params);
/* k4 = {k_normal, k_depth, k_albedo, k_colour} of params (host only); the parameter errors
 * above. */
vcrt_result vcrt_denoise_scales(const vcrt_denoise_params* params, float k4[4]);
typedef struct vcrt_denoise_stats {
    double   kernel_ms;     /* all passes, HIP events on the render stream */
    double   host_ms;       /* wall time of the call */
    double   pass_ms[8];    /* each pass, between the events around it */
    int32_t  passes;        /* launches = levels */
    int32_t  lds_passes;    /* of them, the passes that staged their footprint in LDS */
    char     kernel[48];    /* "vcrt_denoise_pass" */
} vcrt_denoise_stats;
vcrt_result vcrt_denoise_host(const float* colour, const float* albedo, const float* normal_depth,
                              int32_t width, int32_t height, const vcrt_denoise_params* params,
                              float* out);
vcrt_result vcrt_denoise(const float* colour, const float* albedo, const float* normal_depth,
                         int32_t width, int32_t height, const vcrt_denoise_params* params,
                         float* out, vcrt_denoise_stats* stats);
vcrt_result vcrt_denoise_device(const float* colour, const float* albedo,
                                const float* normal_depth, int32_t width, int32_t height,
                                const vcrt_denoise_params* params, float* out,
                                vcrt_denoise_stats* stats);

/* The reprojection map: where was each pixel's surface in the previous frame? vcrt_set_camera and
 * vcrt_update_spheres restart the accumulation; this call and vcrt_reproject below carry the
 * previous output across them. Added.
 *
 * For every valid local pixel (x, y) the call traces the pixel's centre ray, o = camera centre,
 * d = corner(x, y) - centre with corner = pixel00 + x delta_u + y delta_v: no jitter, no lens
 * offset (a jittered ray would shift a static scene's map by up to half a pixel; the map
 * describes the pixel, not a sample; a lens renderer's map is the pinhole's). (t, s, normal) is
 * the ray's first hit exactly as vcrt_ray_hit reports it: hit_sphere's strict <, the earliest
 * index on ties, normal = (point - c) / r, not flipped.
 * The previous camera, once on the host in fp32: cam' = the camera of prev_camera at the
 * renderer's width and height, C' its centre, and
 *   e = pixel00' - C'    nw = cross(delta_u', delta_v')    num = dot(e, nw)
 *   nu = delta_u' / dot(delta_u', delta_u')    nv = delta_v' / dot(delta_v', delta_v')
 * Per pixel, every fp32 operation rounded on its own, no contraction, divisions correctly
 * rounded, dot products summed left to right (c', r': sphere s's previous centre and radius):
 *   Q    = s >= 0 ? c' + r' * normal    per component: the product, then the sum
 *                 : C' + d              the sky is a direction: no parallax
 *   q    = Q - C'    den = dot(q, nw)    lam = num / den
 *   ok   = lam > 0 && lam <= FLT_MAX    (false for a NaN)
 *   h    = lam * q - e    px = dot(h, nu)    py = dot(h, nv)    z' = den / num
 *   key  = (float)(s + 2)               the sky: 1
 *   motion  = ok ? (px, py, z', key) : (0, 0, 0, 0)
 *   surface = (key, s >= 0 ? t : 0, 0, 0)
 * (px, py) are whole-frame pixel coordinates, pixel centres at integers (pixel00 is the centre of
 * pixel (0, 0)); z' is the depth the previous camera would have reported for the point, in t's
 * units (the viewport plane is at 1). vcrt_motion_project is the projection as code.
 * Identity is exact: when prev_camera is NULL or has the current vcrt_camera's bits, and the
 * pixel is sky or sphere s's previous centre and radius have the current bits,
 *   motion = ((float)x, (float)y, s >= 0 ? t : 1.0f, key)
 * so a static view of a static scene accumulates exactly.
 *
 * prev_spheres NULL: the current values; else count must be the scene's, and only the centres
 * and radii are read. vcrt_draw_motion takes host pointers (the previous centres and radii go
 * into a device table, the planes through staging planes; both kept, only grown, freed by
 * vcrt_end); vcrt_draw_motion_device device pointers: prev_spheres the 40-byte records, 4-B
 * aligned, the planes 16-B aligned. Either plane may be NULL, not both. Both planes are float4
 * [elements] in the rank-local framebuffer's layout (vcrt_local_layout); slots outside the frame
 * are left untouched; gathered planes go through vcrt_assemble_tiles as frames do. One launch of
 * vcrt_frame_motion, one wave per local 8x8 tile; a pinhole renderer with camera-ray lists takes
 * them (VCRT_FEATURE_LISTS=0: never; same bits). The framebuffer, the accumulation, vcrt_stats,
 * the cost order and the frame's jitter and lens tables are left alone.
 * Errors: VCRT_ERROR_INITIALIZATION_FAILED, before anything touches the GPU: before vcrt_begin,
 * both planes NULL, a misaligned device pointer. VCRT_ERROR_FORMAT_NOT_SUPPORTED: prev_spheres
 * with a count that is not the scene's, a scene of 2^24 - 2 spheres or more (the key would not
 * be exact). VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object has no vcrt_frame_motion
 * kernel (an A/B build of an older tree). */
typedef struct vcrt_motion_stats {
    uint64_t rays;         /* valid local pixels */
    uint64_t hit_rays;     /* of them, centre rays that hit a sphere */
    uint64_t projected;    /* pixels whose point projected (ok), identity included */
    uint64_t identity;     /* pixels served by the identity rule */
    uint64_t listed_rays;  /* rays answered from the camera-ray lists */
    uint64_t group_tests;  /* as vcrt_feature_stats, per wave */
    uint64_t bound_tests;
    double   kernel_ms;    /* HIP events on the render stream */
    double   host_ms;      /* wall time of the call */
    char     kernel[48];   /* "vcrt_frame_motion" */
} vcrt_motion_stats;
vcrt_result vcrt_draw_motion(const vcrt_camera* prev_camera, const vcrt_sphere* prev_spheres,
                             int32_t count, float* motion, float* surface,
                             vcrt_motion_stats* stats);
vcrt_result vcrt_draw_motion_device(const vcrt_camera* prev_camera,
                                    const vcrt_sphere* prev_spheres, int32_t count, float* motion,
                                    float* surface, vcrt_motion_stats* stats);
/* The projection above as code (host only, no GPU): (px, py, z') of each of `count` world points
 * through the camera prev_camera (NULL: desc's) at desc's width and height, into out [count][3];
 * a NaN triple where the point does not project. VCRT_ERROR_INITIALIZATION_FAILED for an invalid
 * desc, a negative count or a NULL array with count > 0. */
vcrt_result vcrt_motion_project(const vcrt_render_desc* desc, const vcrt_camera* prev_camera,
                                const float* points /* [count][3] */, int32_t count,
                                float* out /* [count][3] */);

/* Temporal accumulation: the previous call's output, gathered at the position each pixel's
 * surface had in the previous frame, blended with the new frame. The denoiser above is spatial
 * only; this is the link that lets samples outlive a camera move or a scene update. A pure image
 * function of the caller's planes, like vcrt_denoise: a one-GPU framebuffer, or rank 0's
 * assembled frame with the other planes put through vcrt_assemble_tiles. Added.
 *
 * Planes, each [height][width], row 0 at the top. float4: colour, the new frame; motion, this
 * frame's reprojection map as vcrt_draw_motion writes it, (px, py, z, key) -- the pixel's surface
 * lay at (px, py) of the previous frame at depth z, and key names the surface (1: the sky,
 * s + 2: sphere s; 0: nothing to reproject); history_colour, the previous call's out;
 * history_surface, the previous frame's surface plane (key, depth, -, -), the last two words
 * not read; out. float: history_length, the previous call's out_length; out_length.
 *
 * Per pixel p with m = motion[p], W = (float)width, H = (float)height, every fp32 operation
 * rounded on its own, no contraction, divisions correctly rounded:
 *   if !(m.w >= 1 && m.x > -1 && m.x < W && m.y > -1 && m.y < H):   (a NaN fails)
 *       out = colour[p], out_length = 1
 *   fx = floorf(m.x), fy = floorf(m.y), ax = m.x - fx, ay = m.y - fy, ix = (int)fx, iy = (int)fy
 *   the taps q = (ix + dx, iy + dy) in the order (dx, dy) = (0,0), (1,0), (0,1), (1,1):
 *     b = (dx ? ax : 1 - ax) * (dy ? ay : 1 - ay)
 *     skipped, nothing of q read, when b == 0 or q lies outside the frame; rejected unless
 *       history_surface[q].x == m.w                      the same sphere, or sky on sky
 *       history_length[q] >= 1
 *       m.w == 1 || depth_tolerance == 0 ||              zq = history_surface[q].y
 *         fabsf(m.z - zq) / ((fabsf(m.z) + fabsf(zq)) + 0x1p-20f) <= depth_tolerance
 *     accepted: acc.c += b * history_colour[q].c (rgb), lsum += b * history_length[q],
 *               wsum += b                                all from +0
 *   if wsum > 0:
 *       hcol.c = acc.c / wsum    L = lsum / wsum    N = fminf(L + 1, max_history)
 *       a = fmaxf(alpha, 1 / N)
 *       out.c = hcol.c + a * (colour.c - hcol.c)    out.a = colour.a    out_length = N
 *   else: out = colour[p], out_length = 1
 * While N stays below max_history and 1 / N above alpha this is the running mean of the samples
 * seen at the surface point; from there on an exponential average. A sequence starts from a
 * history_length plane of zeros (every tap rejected: out = colour, out_length = 1).
 * The contract holds for finite planes; any other input is processed without a fault,
 * deterministically, and is otherwise unspecified. No plane is read outside the frame, whatever
 * motion holds: NaN, infinities, huge values.
 *
 * vcrt_reproject_host is the definition as code (host only, no GPU; csrc/reproject.cpp).
 * vcrt_reproject takes host pointers, staged through device planes that are kept, only grown, and
 * freed by vcrt_end; vcrt_reproject_device device pointers, the float4 planes 16-B and the float
 * planes 4-B aligned, readable on the renderer's device. Both need vcrt_begin for the device, the
 * stream and the code object, run one launch of vcrt_reproject_pass on the render stream -- one
 * lane per pixel -- and return when done. They leave alone the framebuffer, the accumulation,
 * vcrt_stats and the cost order. The planes' size need not be the renderer's.
 * Errors: VCRT_ERROR_FORMAT_NOT_SUPPORTED, checked first, so it reads the same before vcrt_begin:
 * a struct_size that is not sizeof(vcrt_reproject_params), a NaN parameter, alpha outside (0, 1],
 * max_history outside 1 .. 65535, a negative depth_tolerance, width or height outside
 * 1 .. 65535, more than 2^26 pixels. VCRT_ERROR_INITIALIZATION_FAILED, before anything touches
 * the GPU: a NULL plane, out or out_length equal to an input pointer or to each other, a
 * misaligned device plane, and (not vcrt_reproject_host) before vcrt_begin.
 * VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object has no vcrt_reproject_pass kernel
 * (an A/B build of an older tree). A NULL params takes vcrt_default_reproject_params. */
typedef struct vcrt_reproject_params {
    uint32_t struct_size;      /* sizeof(vcrt_reproject_params) */
    float    alpha;            /* 0 < alpha <= 1: the least weight of the new frame */
    float    max_history;      /* 1 .. 65535: cap of the history length */
    float    depth_tolerance;  /* >= 0, relative; 0 = depth test off */
} vcrt_reproject_params;
/* The defaults: the alpha and depth_tolerance that minimise the error of eight accumulated 4-spp
 * frames of an orbit of the final scene against the last view's 256-spp frame over a small grid
 * (profiles/reproject_defaults.json); max_history 32. */
vcrt_result vcrt_default_reproject_params(vcrt_reproject_params* params);
typedef struct vcrt_reproject_stats {
    double   kernel_ms;        /* the launch, HIP events on the render stream */
    double   host_ms;          /* wall time of the call */
    uint64_t accepted_pixels;  /* pixels with wsum > 0: blended with history */
    char     kernel[48];       /* "vcrt_reproject_pass" */
} vcrt_reproject_stats;
vcrt_result vcrt_reproject_host(const float* colour, const float* motion,
                                const float* history_colour, const float* history_surface,
                                const float* history_length, int32_t width, int32_t height,
                                const vcrt_reproject_params* params, float* out,
                                float* out_length);
vcrt_result vcrt_reproject(const float* colour, const float* motion, const float* history_colour,
                           const float* history_surface, const float* history_length,
                           int32_t width, int32_t height, const vcrt_reproject_params* params,
                           float* out, float* out_length, vcrt_reproject_stats* stats);
vcrt_result vcrt_reproject_device(const float* colour, const float* motion,
                                  const float* history_colour, const float* history_surface,
                                  const float* history_length, int32_t width, int32_t height,
                                  const vcrt_reproject_params* params, float* out,
                                  float* out_length, vcrt_reproject_stats* stats);

/* Variance-guided denoising (Schied et al. 2017, SVGF): the link between the two calls above. The
 * accumulation carries the first and second moments of the demodulated luminance along
 * (vcrt_reproject_moments), they become a per-pixel variance, estimated spatially where the
 * history is short (vcrt_variance), and that variance sets the denoiser's colour threshold per
 * pixel and is filtered with the signal (vcrt_denoise_variance). vcrt_reproject and vcrt_denoise
 * are unchanged. Pure image functions of the caller's planes, each [height][width], row 0 at the
 * top, with the three forms of the calls above. Added.
 * Everywhere: every fp32 operation rounded on its own, no contraction, divisions correctly
 * rounded, sums from +0 in the stated order, one lane per output pixel, eps = 0x1p-10f and
 *   lum(v) = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z
 *
 * vcrt_reproject_moments: vcrt_reproject's five input planes and two output planes, whose bits
 * are exactly vcrt_reproject's for the same planes and alpha, max_history, depth_tolerance; and
 * albedo (float4, may be NULL), history_moments (float4, the previous call's out_moments) and
 * out_moments (float4). Per pixel p, c = colour[p]:
 *   s.c = albedo ? c.c / fmaxf(albedo[p].c, eps) : c.c    (rgb: the signal the denoiser filters)
 *   Y = lum(s)    Y2 = Y * Y
 *   the four taps are visited, skipped, rejected and accepted exactly as in vcrt_reproject; an
 *   accepted tap q adds, after vcrt_reproject's five sums,
 *     m1 += b * history_moments[q].x    m2 += b * history_moments[q].y
 *   (a skipped or rejected tap's moments are not read)
 *   if wsum > 0:  rn = 1 / N    (vcrt_reproject's a is fmaxf(alpha, rn))
 *       h1 = m1 / wsum    h2 = m2 / wsum    am = fmaxf(alpha_moments, rn)
 *       M1 = h1 + am * (Y - h1)    M2 = h2 + am * (Y2 - h2)
 *   else: M1 = Y, M2 = Y2                                  (N = 1)
 *   out_moments = (M1, M2, fmaxf(M2 - M1 * M1, 0), N)
 * A sequence starts from history planes of zeros, as vcrt_reproject's does. No plane is read
 * outside the frame, whatever motion holds. One launch of vcrt_reproject_moments_pass.
 * Errors: vcrt_reproject's, with alpha_moments outside (0, 1] a FORMAT error, a NULL
 * history_moments or out_moments, and an output plane equal to any other plane,
 * INITIALIZATION_FAILED. A NULL params takes vcrt_default_reproject_moments_params.
 *
 * vcrt_variance: moments, the out_moments plane above; surface, this frame's surface plane from
 * vcrt_draw_motion (only .x, the key, is read); variance, float [height][width]: the variance of
 * the accumulated, demodulated luminance. Per pixel p = (x, y), N = fmaxf(moments[p].w, 1):
 *   if moments[p].w >= min_history:  v = moments[p].z
 *   else: the taps q = (x + dx, y + dy) for dx, dy in -3 .. 3, dy outer and dx inner, both
 *     ascending; a tap counts when it is inside the frame and surface[q].x == surface[p].x; the
 *     centre always counts. For every counting tap, in that order,
 *       S1 += moments[q].x    S2 += moments[q].y    n += 1    (n a float, exact)
 *     a1 = S1 / n    a2 = S2 / n
 *     v = fmaxf(a2 - a1 * a1, 0) * (min_history / N)        SVGF's boost of young pixels
 *   variance[p] = v * fmaxf(alpha, 1 / N)
 * alpha is the vcrt_reproject alpha the sequence runs with: the factor is the newest frame's
 * weight in the accumulated colour. That is the variance of the mean exactly while the
 * accumulation is the running mean (weight 1 / N each); once the average is exponential the
 * variance of the mean tends to alpha / (2 - alpha) of a sample's, so the factor alpha is an
 * upper estimate. One launch of vcrt_variance_pass_lds, whose workgroup stages its 32 x 8 pixels
 * with their halo of 3 in LDS; VCRT_VARIANCE_LDS=0 in the environment (read at every call) takes
 * vcrt_variance_pass, which reads the taps directly: the same bits, 2 to 3.5 times the time
 * wherever a seventh of the pixels or more is young (profiles/variance.json).
 * Errors: FORMAT_NOT_SUPPORTED for a wrong struct_size, min_history outside 1 .. 65535, alpha
 * outside (0, 1], a NaN, the shape limits above; INITIALIZATION_FAILED for a NULL plane, variance
 * equal to an input, a misaligned device plane (moments, surface 16 B, variance 4 B), and (not
 * _host) before vcrt_begin. A NULL params takes vcrt_default_variance_params.
 *
 * vcrt_denoise_variance: vcrt_denoise with one more input, variance (float [height][width]), and
 * one more output, out_variance (float [height][width], may be NULL). The variance rides in the
 * fourth channel of the signal: s_0.w = fmaxf(variance[p], 0), s_0.rgb as vcrt_denoise's. Per
 * pass l and pixel p = (x, y), differing from vcrt_denoise in this only:
 *   the colour term is ON when sigma_colour != 0; then, before the 25 taps,
 *     the taps q = (x + dx, y + dy) for dx, dy in -1 .. 1 (spacing 1 at every pass), dy outer
 *     and dx inner, both ascending, taps outside the frame skipped, k3 = {1/4, 1/2, 1/4}:
 *       h3 = k3[dx + 1] * k3[dy + 1]    gsum += h3 * s_l(q).w    gw += h3
 *     g  = gsum / gw
 *     kv = 1.0f / ((sigma_colour * sigma_colour) * g + 0x1p-20f)   sigma_colour does not halve:
 *                                                                 the variance shrinks instead
 *   per tap: dy = lum(s_l(p)) - lum(s_l(q))    tl = (dy * dy) * kv    in the place of dl * kl_l
 *   X, e, w, acc.c and wsum as vcrt_denoise's; after wsum += w:  vacc += (w * w) * s_l(q).w
 *   s_{l+1}(p).rgb = acc / wsum    s_{l+1}(p).w = vacc / (wsum * wsum)
 * Final: out as vcrt_denoise's (re-modulated, out.a = colour.a); out_variance[p] = s_levels(p).w.
 * A tap whose guide terms alone reach 1 has w = 0 and adds +0 to every sum; its signal is not
 * read. One launch per pass of vcrt_denoise_var_pass or, for the first VCRT_DENOISE_LDS passes,
 * vcrt_denoise_var_pass_lds (the staged halo of 2 step holds the 3 x 3 taps; same bits).
 * Errors: vcrt_denoise's for its parameters and planes; a NULL variance, variance equal to out,
 * out_variance equal to any other plane, a misaligned device plane (the float planes 4 B):
 * INITIALIZATION_FAILED. A NULL params takes vcrt_default_denoise_variance_params.
 *
 * The host forms stage through device planes that are kept, only grown, and freed by vcrt_end.
 * All leave alone the framebuffer, the accumulation, vcrt_stats and the cost order.
 * VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object lacks the call's kernels. */
typedef struct vcrt_reproject_moments_params {
    uint32_t struct_size;      /* sizeof(vcrt_reproject_moments_params) */
    float    alpha;            /* as vcrt_reproject_params */
    float    max_history;
    float    depth_tolerance;
    float    alpha_moments;    /* 0 < alpha_moments <= 1: the least weight of the new moments */
} vcrt_reproject_moments_params;
typedef struct vcrt_variance_params {
    uint32_t struct_size;      /* sizeof(vcrt_variance_params) */
    float    min_history;      /* 1 .. 65535: below it the variance is estimated spatially */
    float    alpha;            /* 0 < alpha <= 1: the sequence's vcrt_reproject alpha */
} vcrt_variance_params;
typedef struct vcrt_variance_stats {
    double   kernel_ms;        /* the launch, HIP events on the render stream */
    double   host_ms;          /* wall time of the call */
    uint64_t spatial_pixels;   /* pixels below min_history: estimated from their neighbours */
    char     kernel[48];       /* "vcrt_variance_pass_lds" or "vcrt_variance_pass" */
} vcrt_variance_stats;
/* The defaults of the three calls: tools/variance_defaults.py's choice
 * (profiles/variance_defaults.json). vcrt_default_denoise_variance_params is
 * vcrt_default_denoise_params with the chain's sigma_colour. */
vcrt_result vcrt_default_reproject_moments_params(vcrt_reproject_moments_params* params);
vcrt_result vcrt_default_variance_params(vcrt_variance_params* params);
vcrt_result vcrt_default_denoise_variance_params(vcrt_denoise_params* params);
vcrt_result vcrt_reproject_moments_host(const float* colour, const float* motion,
                                        const float* history_colour, const float* history_surface,
                                        const float* history_length, const float* albedo,
                                        const float* history_moments, int32_t width,
                                        int32_t height,
                                        const vcrt_reproject_moments_params* params, float* out,
                                        float* out_length, float* out_moments);
/* stats: vcrt_reproject_stats, kernel "vcrt_reproject_moments_pass" */
vcrt_result vcrt_reproject_moments(const float* colour, const float* motion,
                                   const float* history_colour, const float* history_surface,
                                   const float* history_length, const float* albedo,
                                   const float* history_moments, int32_t width, int32_t height,
                                   const vcrt_reproject_moments_params* params, float* out,
                                   float* out_length, float* out_moments,
                                   vcrt_reproject_stats* stats);
vcrt_result vcrt_reproject_moments_device(const float* colour, const float* motion,
                                          const float* history_colour,
                                          const float* history_surface,
                                          const float* history_length, const float* albedo,
                                          const float* history_moments, int32_t width,
                                          int32_t height,
                                          const vcrt_reproject_moments_params* params, float* out,
                                          float* out_length, float* out_moments,
                                          vcrt_reproject_stats* stats);
vcrt_result vcrt_variance_host(const float* moments, const float* surface, int32_t width,
                               int32_t height, const vcrt_variance_params* params,
                               float* variance);
vcrt_result vcrt_variance(const float* moments, const float* surface, int32_t width,
                          int32_t height, const vcrt_variance_params* params, float* variance,
                          vcrt_variance_stats* stats);
vcrt_result vcrt_variance_device(const float* moments, const float* surface, int32_t width,
                                 int32_t height, const vcrt_variance_params* params,
                                 float* variance, vcrt_variance_stats* stats);
vcrt_result vcrt_denoise_variance_host(const float* colour, const float* albedo,
                                       const float* normal_depth, const float* variance,
                                       int32_t width, int32_t height,
                                       const vcrt_denoise_params* params, float* out,
                                       float* out_variance);
/* stats: vcrt_denoise_stats, kernel "vcrt_denoise_var_pass" */
vcrt_result vcrt_denoise_variance(const float* colour, const float* albedo,
                                  const float* normal_depth, const float* variance, int32_t width,
                                  int32_t height, const vcrt_denoise_params* params, float* out,
                                  float* out_variance, vcrt_denoise_stats* stats);
vcrt_result vcrt_denoise_variance_device(const float* colour, const float* albedo,
                                         const float* normal_depth, const float* variance,
                                         int32_t width, int32_t height,
                                         const vcrt_denoise_params* params, float* out,
                                         float* out_variance, vcrt_denoise_stats* stats);

/* Adaptive sampling: per-pixel sample counts traced on the GPU. vcrt_draw_samples traces, for
 * every local pixel, the number of further samples of the frame's own rays that a count plane
 * names, and sums their radiance in a fixed order; vcrt_sample_counts turns a variance plane
 * (vcrt_variance) into such a count plane. Nothing is uploaded per ray. Added.
 *
 * counts (uint16), sums (float4) and mean (float4, may be NULL) are [elements] planes in the
 * rank-local framebuffer layout (vcrt_local_layout: world 1 [height][width]; world > 1 packed tiles
 * [tiles][64]); slots outside the frame are neither read nor written. For a valid local pixel p,
 *   n_p = min(counts[p], max_count)
 * and its samples are the indices i = first .. first + n_p - 1: ray_i(x, y) is vcrt_frame_rays'
 * ray of that index (the definition above vcrt_draw_features, pinhole or lens), and
 *   r_i = ray_color(ray_i, desc.max_depth)
 * bit for bit what vcrt_trace_rays returns for that ray. The order of summation is fixed with
 * the quantum Q = 4 (vcrt_work_quantum's base): quantum k of pixel p covers the sample offsets
 * 4 k .. min(4 k + 3, n_p - 1);
 *   S_k = the fp32 sum of the quantum's r_i, from +0, in index order
 *   S_p = the fp32 sum of the S_k, from +0, in ascending k
 * every operation rounded on its own, no contraction. So the bits depend on (desc, camera, scene,
 * first, max_count, counts) only -- not on which lane or wave traced which quantum, on the route
 * that served a first hit (the camera-ray lists where the frame has them, else the scans of
 * vcrt_trace_rays; VCRT_FEATURE_LISTS=0 turns the list route off, as for vcrt_draw_features), or
 * on kernel_variant.
 *   accumulate == 0:  sums[p] = (S_p, (float)n_p), which is (0, 0, 0, 0) when n_p == 0
 *   accumulate != 0:  for n_p > 0, sums[p].rgb = old.rgb + S_p (one fp32 add per channel) and
 *                     sums[p].a = old.a + (float)n_p; for n_p == 0 the slot is not written
 * so a zeroed plane carried through several rounds holds (radiance sum, sample count) per pixel;
 * the caller gives each round a `first` at or past the previous round's first + max_count (the
 * indices need not be contiguous, only distinct). When mean is non-NULL,
 *   mean[p] = (sums[p].rgb / sums[p].a, 1) after the update, the divisions correctly rounded;
 *   mean[p] = (0, 0, 0, 1) where sums[p].a == 0
 * Relation to the frame: with uniform counts 4, first 0 and a non-progressive desc of
 * samples_per_pixel 4 and accumulate_quantum 4, mean.rgb equals the framebuffer's rgb bit for bit
 * (both are the sequential sum divided once).
 *
 * Three kernels run on the render stream: vcrt_sample_scan (the exclusive prefix of
 * ceil(n_p / 4), the item table, the totals; one 32-byte read-back sizes the scratch, 16 B per
 * item, kept and only grown), vcrt_trace_samples (a persistent grid whose waves claim items for
 * their idle lanes with one atomic; a lane runs its item's up to four paths one after another, so
 * a pixel's quanta spread over lanes and waves) and vcrt_sample_resolve (one lane per pixel).
 * The call is local, not collective, and returns when done. It leaves alone the framebuffer, the
 * progressive accumulation, vcrt_stats, the measured cost order and the frame's jitter and lens
 * tables: the jitter terms and lens origins of [first, first + max_count) are built with the
 * kernel and host functions the frame uses into vcrt_draw_features' tables. After
 * vcrt_set_camera, vcrt_update_spheres and vcrt_set_scene it sees the new state.
 * vcrt_draw_samples takes host pointers (staged through device planes kept between calls; sums
 * is uploaded first when accumulate != 0 or the planes are packed tiles); vcrt_draw_samples_device
 * device pointers, the float4 planes 16-B aligned, counts 2-B aligned.
 * Errors: VCRT_ERROR_FORMAT_NOT_SUPPORTED for max_count == 0, max_count > 256 or first +
 * max_count > 2^19, checked before the renderer's state, so they read the same before vcrt_begin,
 * and when the scan finds more than 2^28 quanta (nothing is written then);
 * VCRT_ERROR_INITIALIZATION_FAILED, before anything touches the GPU, before vcrt_begin, for a
 * NULL counts or sums, for mean == sums and for a misaligned device plane;
 * VCRT_ERROR_FEATURE_NOT_PRESENT when the loaded code object lacks the three kernels (an A/B
 * build of an older tree). */
typedef struct vcrt_sample_stats {
    uint64_t pixels;       /* valid local pixels with n_p > 0 */
    uint64_t samples;      /* sum of n_p over the valid local pixels */
    uint64_t items;        /* work items (quanta) traced */
    uint64_t segments;     /* ray segments traced */
    uint64_t listed_rays;  /* camera rays answered from the camera-ray lists (0 if the route is not used) */
    uint64_t group_tests, bound_tests;   /* as vcrt_ray_stats */
    double   scan_ms, kernel_ms, resolve_ms, host_ms;  /* HIP events on the render stream; wall */
    char     kernel[48];   /* the tracing kernel's symbol */
} vcrt_sample_stats;
vcrt_result vcrt_draw_samples(uint32_t first, uint32_t max_count, const uint16_t* counts,
                              int32_t accumulate, float* sums, float* mean,
                              vcrt_sample_stats* stats);
vcrt_result vcrt_draw_samples_device(uint32_t first, uint32_t max_count, const uint16_t* counts,
                                     int32_t accumulate, float* sums, float* mean,
                                     vcrt_sample_stats* stats);
/* vcrt_sample_counts: a count plane from a variance plane, element-wise; variance is a float
 * plane and counts a uint16 plane of `elements` entries each (any layout: the same one).
 *   k = 1.0f / (target * target)      the product, then one correctly rounded division (host)
 *   v = fmaxf(variance[e], 0)         (a NaN gives 0)
 *   t = v * k
 *   c = t >= (float)max_count ? max_count : (uint32_t)ceilf(t)
 *   counts[e] = max(c, min_count)
 * target is the standard deviation to reach: a pixel whose mean has variance v needs about
 * v / target^2 times the samples it has. stats->total is the sum of the counts, so a caller can
 * rescale target to a budget. The kernel (vcrt_sample_counts_pass) computes the host function's
 * bits. Errors: FORMAT_NOT_SUPPORTED for a wrong struct_size, a target that is not positive and
 * finite or whose k is not (NaN included), min_count > max_count, max_count > 256, elements == 0
 * or > 2^31; INITIALIZATION_FAILED for a NULL params or plane, counts equal to variance, a
 * misaligned device plane (variance 4 B, counts 2 B), and (not _host) before vcrt_begin;
 * FEATURE_NOT_PRESENT when the loaded code object lacks the kernel. */
typedef struct vcrt_sample_count_params {
    uint32_t struct_size;  /* sizeof(vcrt_sample_count_params) */
    float    target;       /* > 0: the standard deviation to reach */
    uint32_t min_count, max_count;   /* min_count <= max_count <= 256 */
} vcrt_sample_count_params;
typedef struct vcrt_sample_count_stats {
    uint64_t total;        /* the sum of the counts written */
    double   kernel_ms;    /* the launch, HIP events on the render stream (0: _host) */
    double   host_ms;      /* wall time of the call (0: _host) */
    char     kernel[48];   /* "vcrt_sample_counts_pass" (empty: _host) */
} vcrt_sample_count_stats;
vcrt_result vcrt_sample_counts_host(const float* variance, uint32_t elements,
                                    const vcrt_sample_count_params* params, uint16_t* counts,
                                    vcrt_sample_count_stats* stats);
vcrt_result vcrt_sample_counts(const float* variance, uint32_t elements,
                               const vcrt_sample_count_params* params, uint16_t* counts,
                               vcrt_sample_count_stats* stats);
vcrt_result vcrt_sample_counts_device(const float* variance, uint32_t elements,
                                      const vcrt_sample_count_params* params, uint16_t* counts,
                                      vcrt_sample_count_stats* stats);

/* Loads (or reloads) the tracer code object from a file; the analogue of
 * CreateShaderStageFromFile. Returns VCRT_ERROR_INCOMPATIBLE_SHADER_BINARY when the file
 * cannot be read or is not a gfx950 code object. Requires vcrt_begin. A lens renderer
 * (lens_radius > 0) gets VCRT_ERROR_FEATURE_NOT_PRESENT for a code object without the *_lens
 * kernels (an A/B build of an older tree), and so do its draws until another one is loaded. */
vcrt_result vcrt_shader_load(const char* filename);

/* Built-in scenes. */
#define VCRT_SCENE_FINAL 0       /* SceneGenerator (481) + big three + ground = 485 spheres */
#define VCRT_SCENE_THREE 1       /* big three + ground (globals.glsl:513-517) = 4 spheres   */
#define VCRT_SCENE_RED 2         /* red Lambertian (0,1,0) r=1 + ground = 2 spheres         */
#define VCRT_SCENE_STRESS4096 3  /* 4096 generated (grid [-33,33)^2) + big three + ground   */
/* Writes up to cap spheres; returns the scene's sphere count, or a negative VkResult. */
int32_t vcrt_scene_builtin(int32_t scene_id, vcrt_sphere* out, int32_t cap);
/* SceneGenerator stdout, byte for byte. Returns the length (excluding NUL); writes up to cap-1
 * bytes plus NUL when buf != NULL. */
size_t vcrt_scene_generator_text(char* buf, size_t cap);

/* The culled scans' grouped tables for a sphere list (host only, no GPU). The big spheres
 * (radius > 8x the median and 5% of the centres' extent) form a short list of groups tested
 * for every ray (*big_groups of them, written first to geom/index); the rest form the
 * hierarchy. Tables: groups of four in pair-SoA form (16 floats each), hierarchy group-pair
 * boxes (16 floats per two groups: lox0 lox1 loy0 loy1 loz0 loz1 hix0 hix1 hiy0 hiy1 hiz0 hiz1
 * K0 K1 0 0 -- the members' extent rounded outwards and K = 8.1u / r_min of the members; a ray
 * rules box i out when its line misses the box grown by its margin, see csrc/tracer.hip
 * box_gap), node-pair boxes (same form; node i covers hierarchy groups 8i..8i+7), top-level
 * boxes (same form; entry i covers hierarchy groups 64i..64i+63, count ceil(G/64) rounded up to
 * even), member indices (4 per group, -1 = padding) and margin4 = {max |centre|, r_max^2, max
 * |box coordinate|, 0} over the hierarchy (rounded up). Returns the hierarchy group count G, a
 * multiple of 16 (0 = culling does not apply: < 16 spheres or unbounded scene), and writes the
 * tables when cap_groups >= *big_groups + G (any pointer may be NULL). */
int32_t vcrt_cull_tables(const vcrt_sphere* spheres, int32_t count, float* geom, float* bound,
                         float* node, float* top, int32_t* index, int32_t* big_groups,
                         float* margin4, int32_t cap_groups);

/* The shared y slab of those tables (host only, no GPU): 1 when every group, node and chunk box
 * that has members carries the same finite lo.y and hi.y, bit for bit -- written to lohi when it
 * is not NULL -- so that the flat culled scans evaluate the two y planes once per ray instead of
 * once per box (csrc/tracer.hip, fact (3a)); 0 otherwise, when culling does not apply, or with
 * VCRT_SLAB=0 in the environment (the three-axis test everywhere: A/B runs and tests). */
int32_t vcrt_cull_slab(const vcrt_sphere* spheres, int32_t count, float lohi[2]);

/* The footprint tables of those tables' node level (host only, no GPU; csrc/cluster.hpp
 * CullTables::fp_tab, csrc/tracer.hip fact (5)), as the LDS-table flat scan gets them: tables =
 * [4][N] node bit masks (x: lo.x <= cell, hi.x >= cell; then z), params8 = {x scale, x offset,
 * z scale, z offset, y lo, y hi, 2 Kmax, 0} and *always = the nodes every ray keeps. Returns N,
 * the cells per table (0: culling does not apply); any pointer may be NULL. They do not depend
 * on VCRT_SLAB. */
int32_t vcrt_cull_footprint(const vcrt_sphere* spheres, int32_t count, uint32_t* tables,
                            float* params8, uint32_t* always);

/* The group-level footprint tables of the LDS-table flat scan (host only, no GPU): tables =
 * [4][N][4] uint32, 128-bit group masks (low word first; bit = hierarchy group index) by cell of
 * x (lo <= cell, hi >= cell) and of z, params8 = {x scale, x offset, z scale, z offset, y lo,
 * y hi, 2 Kmax, 0}, always4 = the groups every ray keeps. Returns N, the cells per table, chosen
 * so that the tables fill the LDS bytes of the group boxes and node tables they replace (0: no
 * tables: culling does not apply, more than 128 hierarchy groups or a degenerate extent).
 * *eligible = 1 when a frame of this scene takes its groups from them in place of the node level:
 * every group box with members has one y extent, bit for bit (whatever VCRT_SLAB says), and
 * VCRT_GROUP_FOOT is not 0; a renderer further needs its camera-ray lists (VCRT_PRIMARY_LISTS;
 * a lens renderer, lens_radius > 0, has none).
 * Any pointer may be NULL. */
int32_t vcrt_cull_group_footprint(const vcrt_sphere* spheres, int32_t count, uint32_t* tables,
                                  float* params8, uint32_t* always4, int32_t* eligible);

/* The flat culled scan's camera-ray lists for a scene and render description (host only, no
 * GPU; csrc/primary.cpp): for each 4x4-pixel quarter (qx, qy) of each local tile lt of
 * desc->rank (in the kernels' local-tile order), info[4 lt + 2 qy + qx] = offset << 4 | count
 * of its hierarchy groups in ids (count <= 8), or 15 when it has no list. Returns the number of
 * ids (-1: no culling tables, an invalid desc, or lens_radius > 0: lens rays share no origin), and writes info / ids when cap_tiles (entries
 * of info) / cap_ids are large enough (pointers may be NULL). */
int32_t vcrt_primary_lists(const vcrt_sphere* spheres, int32_t count, const vcrt_render_desc* desc,
                           uint32_t* info, int32_t cap_tiles, uint16_t* ids, int32_t cap_ids);

/* The camera fast trace's per-sphere lists (host only, no GPU; csrc/primary.cpp): for each 4x4
 * quarter as above, info = first pair << 4 | spheres (<= 14), or 15 when it has no list, and the
 * pair records, 12 floats each: (ocx0,ocx1,ocy0,ocy1) (ocz0,ocz1,cc0,cc1) (index0, index1 as
 * int bits, 0, 0), camera-relative as the kernel's exact test computes them (oc = camera centre -
 * centre, cc = |oc|^2 - r^2 in fp32; an odd list pads with oc = 0, cc = 3e38, index -1). Returns
 * the number of pair records (-1: no culling tables, an invalid desc, or lens_radius > 0: lens rays share no origin), and writes info / rec
 * when cap_tiles (entries) / cap_floats are large enough (pointers may be NULL). */
int32_t vcrt_primary_sphere_lists(const vcrt_sphere* spheres, int32_t count,
                                  const vcrt_render_desc* desc, uint32_t* info, int32_t cap_tiles,
                                  float* rec, int32_t cap_floats);

/* The thin lens's per-sample origin offsets for a render description (host only, no GPU):
 * offsets[3 k .. 3 k + 2] = offset_i for sample index i = first + k, k < count, with R =
 * desc->lens_radius, fi = (float)i and (camera_u, camera_v) shader.comp:28-29's unit basis
 *   a   = rand(fi, fi + 0.5f)            b   = rand(fi + 0.5f, fi)        vcrt_canonical_rand
 *   rho = R * sqrtf(a)                   phi = 6.2831855f * b             0x40C90FDB
 *   lx  = rho * sin(phi + 1.5707964f)    ly  = rho * sin(phi)             vcrt_canonical_sin
 *   offset_i = lx * camera_u + ly * camera_v                              (0x3FC90FDB)
 * every fp32 operation rounded on its own; all +0 when R == 0. i and i + 0.5 are exact for every
 * index a renderer admits (< 2^19). Returns count, or a negative VkResult for an invalid desc or
 * a NULL offsets with count > 0. */
int32_t vcrt_lens_offsets(const vcrt_render_desc* desc, uint32_t first, uint32_t count,
                          float* offsets /* [count][3] */);

/* Device self-test of the kernel's fast sin path (tracer.hip vcrt_check_sin): for the fp32
 * inputs whose bit patterns are first .. first + count - 1, counts those where the device's
 * sin_fast differs from the canonical sin (must be 0) and those where it fell back to the
 * canonical evaluation, and returns the smallest differing pattern (0xFFFFFFFF if none).
 * Diagnostic addition (the reference has no such call). Requires vcrt_begin. */
vcrt_result vcrt_selftest_sin(uint32_t first, uint32_t count, uint64_t* mismatches,
                              uint64_t* fallbacks, uint32_t* first_mismatch);

/* Device self-test of the scatter's unit vector (tracer.hip unit_of, kernel vcrt_check_unit):
 * out[i] = the device's normalize of triples[i] (three rand() values, none negative), which must
 * equal triples[i] / sqrt(dot) with the correctly rounded fp32 sqrt and divisions bit for bit,
 * inside the helper's one-reciprocal range and outside it. n <= 2^28. Diagnostic addition (the
 * reference has no such call). Requires vcrt_begin. */
vcrt_result vcrt_selftest_unit(const float* triples /* [n][3] */, uint32_t n,
                               float* out /* [n][3] */);

/* Canonical math as used by the kernel (host evaluation), for tests and tools. */
float vcrt_canonical_sin(float x);
float vcrt_canonical_rand(float x, float y);

const char* vcrt_result_string(vcrt_result r);

#ifdef __cplusplus
}
#endif
#endif
