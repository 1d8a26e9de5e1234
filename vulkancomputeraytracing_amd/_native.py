"""ctypes view of the C ABI in include/vcrt.h (libvcrt.so, built in-tree by ``make``).

There is no fallback: if the library is missing the import of the renderer fails loudly.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libvcrt.so")
CODE_OBJECT_PATH = os.path.join(LIB_DIR, "vcrt_tracer.hsaco")
BIN_DIR = os.path.join(HERE, "bin")

# VkResult values (vcrt.h)
VK_SUCCESS = 0
VK_NOT_READY = 1
VK_ERROR_OUT_OF_HOST_MEMORY = -1
VK_ERROR_OUT_OF_DEVICE_MEMORY = -2
VK_ERROR_INITIALIZATION_FAILED = -3
VK_ERROR_DEVICE_LOST = -4
VK_ERROR_FEATURE_NOT_PRESENT = -8
VK_ERROR_FORMAT_NOT_SUPPORTED = -11
VK_ERROR_UNKNOWN = -13
VK_ERROR_INCOMPATIBLE_SHADER_BINARY_EXT = 1000482000

TEXTURE_LAMBERTIAN = 1
TEXTURE_METAL = 2
TEXTURE_GLASS = 3

KERNEL_AUTO = 0
KERNEL_LDS = 1
KERNEL_SMEM = 2
KERNEL_CULL = 3
KERNEL_CULL_LANE = 4
KERNEL_CULL_FLAT = 5

SCENE_FINAL = 0
SCENE_THREE = 1
SCENE_RED = 2
SCENE_STRESS4096 = 3


class vcrt_sphere(ctypes.Structure):
    _fields_ = [
        ("center", ctypes.c_float * 3),
        ("radius", ctypes.c_float),
        ("colour", ctypes.c_float * 3),
        ("texture", ctypes.c_float * 3),
    ]


class vcrt_camera(ctypes.Structure):
    _fields_ = [
        ("lookfrom", ctypes.c_float * 3),
        ("lookat", ctypes.c_float * 3),
        ("vup", ctypes.c_float * 3),
        ("vfov", ctypes.c_float),
    ]


class vcrt_render_desc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("samples_per_pixel", ctypes.c_int32),
        ("max_depth", ctypes.c_int32),
        ("camera", vcrt_camera),
        ("device", ctypes.c_int32),
        ("rank", ctypes.c_int32),
        ("world_size", ctypes.c_int32),
        ("kernel_variant", ctypes.c_int32),
        ("blocks_per_cu", ctypes.c_int32),
        ("accumulate_chunk", ctypes.c_int32),
        ("progressive", ctypes.c_int32),
        ("code_object_path", ctypes.c_char_p),
        ("accumulate_tail", ctypes.c_int32),
        ("accumulate_tail_chunk", ctypes.c_int32),
        ("accumulate_quantum", ctypes.c_int32),
        ("lens_radius", ctypes.c_float),
    ]


class vcrt_stats(ctypes.Structure):
    _fields_ = [
        ("segments", ctypes.c_uint64),
        ("sphere_tests", ctypes.c_uint64),
        ("samples", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("frame_ms", ctypes.c_double),
        ("resolve_ms", ctypes.c_double),
        ("gather_ms", ctypes.c_double),
        ("frames", ctypes.c_int32),
        ("grid_blocks", ctypes.c_int32),
        ("block_threads", ctypes.c_int32),
        ("kernel_variant", ctypes.c_int32),
        ("local_tiles", ctypes.c_int32),
        ("nspheres", ctypes.c_int32),
        ("lds_bytes", ctypes.c_uint32),
        ("accumulate_chunk", ctypes.c_int32),
        ("tables_in_lds", ctypes.c_int32),
        ("accumulated_spp", ctypes.c_uint64),
        ("group_tests", ctypes.c_uint64),
        ("bound_tests", ctypes.c_uint64),
        ("kernel", ctypes.c_char * 48),
        ("debug", ctypes.c_uint64 * 128),
        ("accumulate_tail", ctypes.c_int32),
        ("accumulate_tail_chunk", ctypes.c_int32),
        ("ring_entries", ctypes.c_int32),
        ("accumulate_quantum", ctypes.c_int32),
        ("accumulate_scale_log2", ctypes.c_int32),
        ("cost_order", ctypes.c_int32),
        ("scale_rerenders", ctypes.c_int32),
    ]


class vcrt_ray_hit(ctypes.Structure):
    _fields_ = [
        ("t", ctypes.c_float),
        ("sphere", ctypes.c_int32),
        ("segments", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("normal", ctypes.c_float * 3),
        ("reserved2", ctypes.c_float),
    ]


class vcrt_ray_stats(ctypes.Structure):
    _fields_ = [
        ("segments", ctypes.c_uint64),
        ("group_tests", ctypes.c_uint64),
        ("bound_tests", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_feature_stats(ctypes.Structure):
    _fields_ = [
        ("rays", ctypes.c_uint64),
        ("listed_rays", ctypes.c_uint64),
        ("group_tests", ctypes.c_uint64),
        ("bound_tests", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_occlusion_buffer_stats(ctypes.Structure):
    _fields_ = [
        ("rays", ctypes.c_uint64),
        ("hit_rays", ctypes.c_uint64),
        ("secondary_rays", ctypes.c_uint64),
        ("occluded", ctypes.c_uint64),
        ("listed_rays", ctypes.c_uint64),
        ("group_tests", ctypes.c_uint64),
        ("bound_tests", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_denoise_params(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("levels", ctypes.c_int32),
        ("sigma_normal", ctypes.c_float),
        ("sigma_depth", ctypes.c_float),
        ("sigma_albedo", ctypes.c_float),
        ("sigma_colour", ctypes.c_float),
        ("demodulate", ctypes.c_int32),
    ]


class vcrt_denoise_stats(ctypes.Structure):
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("pass_ms", ctypes.c_double * 8),
        ("passes", ctypes.c_int32),
        ("lds_passes", ctypes.c_int32),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_motion_stats(ctypes.Structure):
    _fields_ = [
        ("rays", ctypes.c_uint64),
        ("hit_rays", ctypes.c_uint64),
        ("projected", ctypes.c_uint64),
        ("identity", ctypes.c_uint64),
        ("listed_rays", ctypes.c_uint64),
        ("group_tests", ctypes.c_uint64),
        ("bound_tests", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_reproject_params(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("alpha", ctypes.c_float),
        ("max_history", ctypes.c_float),
        ("depth_tolerance", ctypes.c_float),
    ]


class vcrt_reproject_stats(ctypes.Structure):
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("accepted_pixels", ctypes.c_uint64),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_reproject_moments_params(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("alpha", ctypes.c_float),
        ("max_history", ctypes.c_float),
        ("depth_tolerance", ctypes.c_float),
        ("alpha_moments", ctypes.c_float),
    ]


class vcrt_variance_params(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("min_history", ctypes.c_float),
        ("alpha", ctypes.c_float),
    ]


class vcrt_variance_stats(ctypes.Structure):
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("spatial_pixels", ctypes.c_uint64),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_sample_stats(ctypes.Structure):
    _fields_ = [
        ("pixels", ctypes.c_uint64),
        ("samples", ctypes.c_uint64),
        ("items", ctypes.c_uint64),
        ("segments", ctypes.c_uint64),
        ("listed_rays", ctypes.c_uint64),
        ("group_tests", ctypes.c_uint64),
        ("bound_tests", ctypes.c_uint64),
        ("scan_ms", ctypes.c_double),
        ("kernel_ms", ctypes.c_double),
        ("resolve_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_sample_count_params(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("target", ctypes.c_float),
        ("min_count", ctypes.c_uint32),
        ("max_count", ctypes.c_uint32),
    ]


class vcrt_sample_count_stats(ctypes.Structure):
    _fields_ = [
        ("total", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("kernel", ctypes.c_char * 48),
    ]


class vcrt_camera_stats(ctypes.Structure):
    _fields_ = [
        ("host_ms", ctypes.c_double),
        ("lists_ms", ctypes.c_double),
        ("on_device", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("quarters", ctypes.c_uint64),
        ("group_ids", ctypes.c_uint64),
        ("pair_records", ctypes.c_uint64),
    ]


class vcrt_scene_update_stats(ctypes.Structure):
    _fields_ = [
        ("host_ms", ctypes.c_double),
        ("refit_ms", ctypes.c_double),
        ("lists_ms", ctypes.c_double),
        ("on_device", ctypes.c_int32),
        ("rebuilt", ctypes.c_int32),
        ("groups", ctypes.c_uint64),
        ("boxes", ctypes.c_uint64),
        ("footprint_cells", ctypes.c_uint64),
    ]


class vcrt_scene_scalars(ctypes.Structure):
    _fields_ = [
        ("nbig", ctypes.c_int32),
        ("ngroups", ctypes.c_int32),
        ("margin", ctypes.c_float * 4),
        ("slab_on", ctypes.c_int32),
        ("slab", ctypes.c_float * 2),
        ("fp_x", ctypes.c_float * 2),
        ("fp_z", ctypes.c_float * 2),
        ("fp_y", ctypes.c_float * 2),
        ("fp_k2", ctypes.c_float),
        ("fp_always", ctypes.c_uint32),
        ("gf_n", ctypes.c_uint32),
        ("gf_x", ctypes.c_float * 2),
        ("gf_z", ctypes.c_float * 2),
        ("gf_k2", ctypes.c_float),
        ("gf_always", ctypes.c_uint32 * 4),
        ("gf_ok", ctypes.c_int32),
        ("bounded", ctypes.c_int32),
        ("radii_safe", ctypes.c_int32),
    ]


# VCRT_TABLE_* (vcrt.h): name -> (id, numpy dtype of the table's words)
SCENE_TABLES = {
    "linear": (0, "float32"),
    "center_radius": (1, "float32"),
    "shade": (2, "float32"),
    "material": (3, "float32"),
    "groups": (4, "float32"),
    "bound": (5, "float32"),
    "bound_nf": (6, "float32"),
    "node": (7, "float32"),
    "node_nf": (8, "float32"),
    "top": (9, "float32"),
    "foot": (10, "uint32"),
    "group_foot": (11, "uint32"),
    "scalars": (12, "uint8"),
}


class vcrt_comm_id(ctypes.Structure):
    _fields_ = [("internal", ctypes.c_char * 128)]  # an ncclUniqueId


# name -> (restype, argtypes); every symbol include/vcrt.h declares.
SIGNATURES = {
    "vcrt_default_desc": (ctypes.c_int32, [ctypes.POINTER(vcrt_render_desc)]),
    "vcrt_begin": (ctypes.c_int32, [ctypes.POINTER(vcrt_render_desc)]),
    "vcrt_work_quantum": (ctypes.c_int32, [ctypes.POINTER(vcrt_render_desc)]),
    "vcrt_work_chunk": (ctypes.c_int32, [ctypes.POINTER(vcrt_render_desc)]),
    "vcrt_work_tail": (ctypes.c_int32, [ctypes.POINTER(vcrt_render_desc),
                                        ctypes.POINTER(ctypes.c_int32)]),
    "vcrt_pixel_scale_log2": (ctypes.c_int32, [ctypes.c_float]),
    "vcrt_set_scene": (ctypes.c_int32, [ctypes.POINTER(vcrt_sphere), ctypes.c_int32]),
    "vcrt_draw_next_frame": (ctypes.c_int32, []),
    "vcrt_end": (ctypes.c_int32, []),
    "vcrt_comm_unique_id": (ctypes.c_int32, [ctypes.POINTER(vcrt_comm_id)]),
    "vcrt_comm_init": (ctypes.c_int32, [ctypes.POINTER(vcrt_comm_id)]),
    "vcrt_local_layout": (ctypes.c_int32, [ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint32)]),
    "vcrt_read_framebuffer": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_size_t]),
    "vcrt_framebuffer_device": (
        ctypes.c_int32, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]),
    "vcrt_set_framebuffer_device": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_size_t]),
    "vcrt_assemble_tiles": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p] +
                            [ctypes.c_int32] * 3 + [ctypes.c_uint32]),
    "vcrt_get_stats": (ctypes.c_int32, [ctypes.POINTER(vcrt_stats)]),
    "vcrt_reset_accumulation": (ctypes.c_int32, []),
    "vcrt_set_camera": (ctypes.c_int32, [ctypes.POINTER(vcrt_camera)]),
    "vcrt_get_camera_stats": (ctypes.c_int32, [ctypes.POINTER(vcrt_camera_stats)]),
    "vcrt_camera_lists_read": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(ctypes.c_int32)]),
    "vcrt_update_spheres": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32]),
    "vcrt_update_spheres_device": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32]),
    "vcrt_get_scene_update_stats": (ctypes.c_int32, [ctypes.POINTER(vcrt_scene_update_stats)]),
    "vcrt_scene_table_host": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                               ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t]),
    "vcrt_scene_table_read": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t]),
    "vcrt_read_framebuffer_srgb8": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_size_t]),
    "vcrt_selftest_sin": (ctypes.c_int32, [ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint32)]),
    "vcrt_selftest_unit": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "vcrt_srgb8_thresholds": (None, [ctypes.c_void_p]),
    "vcrt_trace_rays": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                         ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.POINTER(vcrt_ray_stats)]),
    "vcrt_trace_rays_device": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.POINTER(vcrt_ray_stats)]),
    "vcrt_occlude_rays": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_uint32, ctypes.c_void_p,
                                           ctypes.POINTER(vcrt_ray_stats)]),
    "vcrt_occlude_rays_device": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_uint32,
                                                  ctypes.c_void_p,
                                                  ctypes.POINTER(vcrt_ray_stats)]),
    "vcrt_draw_features": (ctypes.c_int32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(vcrt_feature_stats)]),
    "vcrt_draw_features_device": (ctypes.c_int32, [ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p,
                                                   ctypes.POINTER(vcrt_feature_stats)]),
    "vcrt_frame_rays": (ctypes.c_int32, [ctypes.POINTER(vcrt_render_desc), ctypes.c_void_p,
                                         ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "vcrt_draw_occlusion": (ctypes.c_int32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_float, ctypes.c_void_p,
                                             ctypes.POINTER(vcrt_occlusion_buffer_stats)]),
    "vcrt_draw_occlusion_device": (ctypes.c_int32, [ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.c_uint32, ctypes.c_float,
                                                    ctypes.c_void_p,
                                                    ctypes.POINTER(vcrt_occlusion_buffer_stats)]),
    "vcrt_ambient_dirs": (ctypes.c_int32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]),
    "vcrt_default_denoise_params": (ctypes.c_int32, [ctypes.POINTER(vcrt_denoise_params)]),
    "vcrt_denoise_scales": (ctypes.c_int32, [ctypes.POINTER(vcrt_denoise_params),
                                             ctypes.c_void_p]),
    "vcrt_denoise_host": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int32, ctypes.c_int32,
                                           ctypes.POINTER(vcrt_denoise_params), ctypes.c_void_p]),
    "vcrt_denoise": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int32, ctypes.c_int32,
                                      ctypes.POINTER(vcrt_denoise_params), ctypes.c_void_p,
                                      ctypes.POINTER(vcrt_denoise_stats)]),
    "vcrt_denoise_device": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int32, ctypes.c_int32,
                                             ctypes.POINTER(vcrt_denoise_params), ctypes.c_void_p,
                                             ctypes.POINTER(vcrt_denoise_stats)]),
    "vcrt_draw_motion": (ctypes.c_int32, [ctypes.POINTER(vcrt_camera), ctypes.c_void_p,
                                          ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.POINTER(vcrt_motion_stats)]),
    "vcrt_draw_motion_device": (ctypes.c_int32, [ctypes.POINTER(vcrt_camera), ctypes.c_void_p,
                                                 ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.POINTER(vcrt_motion_stats)]),
    "vcrt_motion_project": (ctypes.c_int32, [ctypes.POINTER(vcrt_render_desc),
                                             ctypes.POINTER(vcrt_camera), ctypes.c_void_p,
                                             ctypes.c_int32, ctypes.c_void_p]),
    "vcrt_default_reproject_params": (ctypes.c_int32, [ctypes.POINTER(vcrt_reproject_params)]),
    "vcrt_reproject_host": (ctypes.c_int32, [ctypes.c_void_p] * 5 + [ctypes.c_int32] * 2 +
                            [ctypes.POINTER(vcrt_reproject_params), ctypes.c_void_p,
                             ctypes.c_void_p]),
    "vcrt_reproject": (ctypes.c_int32, [ctypes.c_void_p] * 5 + [ctypes.c_int32] * 2 +
                       [ctypes.POINTER(vcrt_reproject_params), ctypes.c_void_p, ctypes.c_void_p,
                        ctypes.POINTER(vcrt_reproject_stats)]),
    "vcrt_reproject_device": (ctypes.c_int32, [ctypes.c_void_p] * 5 + [ctypes.c_int32] * 2 +
                              [ctypes.POINTER(vcrt_reproject_params), ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.POINTER(vcrt_reproject_stats)]),
    "vcrt_default_reproject_moments_params": (ctypes.c_int32,
                                              [ctypes.POINTER(vcrt_reproject_moments_params)]),
    "vcrt_default_variance_params": (ctypes.c_int32, [ctypes.POINTER(vcrt_variance_params)]),
    "vcrt_default_denoise_variance_params": (ctypes.c_int32,
                                             [ctypes.POINTER(vcrt_denoise_params)]),
    "vcrt_reproject_moments_host": (ctypes.c_int32, [ctypes.c_void_p] * 7 + [ctypes.c_int32] * 2 +
                                    [ctypes.POINTER(vcrt_reproject_moments_params)] +
                                    [ctypes.c_void_p] * 3),
    "vcrt_reproject_moments": (ctypes.c_int32, [ctypes.c_void_p] * 7 + [ctypes.c_int32] * 2 +
                               [ctypes.POINTER(vcrt_reproject_moments_params)] +
                               [ctypes.c_void_p] * 3 + [ctypes.POINTER(vcrt_reproject_stats)]),
    "vcrt_reproject_moments_device": (ctypes.c_int32,
                                      [ctypes.c_void_p] * 7 + [ctypes.c_int32] * 2 +
                                      [ctypes.POINTER(vcrt_reproject_moments_params)] +
                                      [ctypes.c_void_p] * 3 +
                                      [ctypes.POINTER(vcrt_reproject_stats)]),
    "vcrt_variance_host": (ctypes.c_int32, [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 2 +
                           [ctypes.POINTER(vcrt_variance_params), ctypes.c_void_p]),
    "vcrt_variance": (ctypes.c_int32, [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 2 +
                      [ctypes.POINTER(vcrt_variance_params), ctypes.c_void_p,
                       ctypes.POINTER(vcrt_variance_stats)]),
    "vcrt_variance_device": (ctypes.c_int32, [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 2 +
                             [ctypes.POINTER(vcrt_variance_params), ctypes.c_void_p,
                              ctypes.POINTER(vcrt_variance_stats)]),
    "vcrt_denoise_variance_host": (ctypes.c_int32, [ctypes.c_void_p] * 4 + [ctypes.c_int32] * 2 +
                                   [ctypes.POINTER(vcrt_denoise_params), ctypes.c_void_p,
                                    ctypes.c_void_p]),
    "vcrt_denoise_variance": (ctypes.c_int32, [ctypes.c_void_p] * 4 + [ctypes.c_int32] * 2 +
                              [ctypes.POINTER(vcrt_denoise_params), ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.POINTER(vcrt_denoise_stats)]),
    "vcrt_denoise_variance_device": (ctypes.c_int32,
                                     [ctypes.c_void_p] * 4 + [ctypes.c_int32] * 2 +
                                     [ctypes.POINTER(vcrt_denoise_params), ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(vcrt_denoise_stats)]),
    "vcrt_draw_samples": (ctypes.c_int32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                           ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(vcrt_sample_stats)]),
    "vcrt_draw_samples_device": (ctypes.c_int32, [ctypes.c_uint32, ctypes.c_uint32,
                                                  ctypes.c_void_p, ctypes.c_int32,
                                                  ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.POINTER(vcrt_sample_stats)]),
    "vcrt_sample_counts_host": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32,
                                                 ctypes.POINTER(vcrt_sample_count_params),
                                                 ctypes.c_void_p,
                                                 ctypes.POINTER(vcrt_sample_count_stats)]),
    "vcrt_sample_counts": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.POINTER(vcrt_sample_count_params),
                                            ctypes.c_void_p,
                                            ctypes.POINTER(vcrt_sample_count_stats)]),
    "vcrt_sample_counts_device": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32,
                                                   ctypes.POINTER(vcrt_sample_count_params),
                                                   ctypes.c_void_p,
                                                   ctypes.POINTER(vcrt_sample_count_stats)]),
    "vcrt_shader_load": (ctypes.c_int32, [ctypes.c_char_p]),
    "vcrt_scene_builtin": (ctypes.c_int32,
                           [ctypes.c_int32, ctypes.POINTER(vcrt_sphere), ctypes.c_int32]),
    "vcrt_scene_generator_text": (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]),
    "vcrt_cull_tables": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                                          ctypes.c_void_p, ctypes.c_int32]),
    "vcrt_cull_slab": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "vcrt_cull_footprint": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "vcrt_cull_group_footprint": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_void_p]),
    "vcrt_primary_lists": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32,
                                            ctypes.POINTER(vcrt_render_desc), ctypes.c_void_p,
                                            ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]),
    "vcrt_primary_sphere_lists": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32,
                                                   ctypes.POINTER(vcrt_render_desc),
                                                   ctypes.c_void_p, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.c_int32]),
    "vcrt_refit_primary_lists": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                  ctypes.POINTER(vcrt_render_desc),
                                                  ctypes.c_void_p, ctypes.c_int32,
                                                  ctypes.c_void_p, ctypes.c_int32]),
    "vcrt_refit_primary_sphere_lists": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p,
                                                         ctypes.c_int32,
                                                         ctypes.POINTER(vcrt_render_desc),
                                                         ctypes.c_void_p, ctypes.c_int32,
                                                         ctypes.c_void_p, ctypes.c_int32]),
    "vcrt_lens_offsets": (ctypes.c_int32, [ctypes.POINTER(vcrt_render_desc), ctypes.c_uint32,
                                           ctypes.c_uint32, ctypes.c_void_p]),
    "vcrt_canonical_sin": (ctypes.c_float, [ctypes.c_float]),
    "vcrt_canonical_rand": (ctypes.c_float, [ctypes.c_float, ctypes.c_float]),
    "vcrt_result_string": (ctypes.c_char_p, [ctypes.c_int32]),
}

_lib = None


def _share_torch_hip_runtime() -> None:
    """One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (SONAME
    libamdhip64.so.7, the same as /opt/rocm's). If it is loaded first, libvcrt.so's
    DT_NEEDED libamdhip64.so.7 binds to it and torch tensors, streams and RCCL share one runtime
    with the tracer; loaded the other way round the process would hold two HIP/HSA runtimes."""
    try:
        import torch  # noqa: F401
    except ImportError:
        return
    # the same for RCCL (SONAME librccl.so.1 in both): libvcrt's gather and torch's
    # process group then use one RCCL
    for name in ("libamdhip64.so", "librccl.so"):
        torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib", name)
        if os.path.exists(torch_lib):
            ctypes.CDLL(torch_lib, mode=ctypes.RTLD_GLOBAL)


def lib() -> ctypes.CDLL:
    """Load libvcrt.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C {HERE}` "
                "(or __graft_entry__.build()); there is no CPU fallback")
        if os.environ.get("VCRT_SYSTEM_HIP", "0") != "1":
            _share_torch_hip_runtime()
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def result_string(code: int) -> str:
    return lib().vcrt_result_string(code).decode()


class VcrtError(RuntimeError):
    def __init__(self, where: str, code: int):
        super().__init__(f"{where} failed: {result_string(code)} ({code})")
        self.code = code


def check_count(where: str, value: int) -> int:
    """A count-or-VkResult return: negative values are errors."""
    if value < 0:
        raise VcrtError(where, value)
    return value


def check(where: str, code: int) -> int:
    if code != VK_SUCCESS:
        raise VcrtError(where, code)
    return code
