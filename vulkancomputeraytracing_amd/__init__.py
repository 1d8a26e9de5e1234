"""MI355X-native drop-in for the fhh200000/VulkanComputeRayTracing hot path.

The per-pixel ray-gen -> sphere-list intersect -> scatter -> multi-bounce accumulate path of
shaders/shader.comp runs as hand-written HIP kernels for gfx950 (csrc/tracer.hip) behind the
C ABI of include/vcrt.h (lib/libvcrt.so). This package is the Python mirror of the reference's
host API (Renderer Begin/Draw/End, Shader loading, SceneGenerator) over that ABI.
"""
from . import _native
from ._native import (VK_SUCCESS, VK_ERROR_INITIALIZATION_FAILED, VcrtError, KERNEL_AUTO,
                      KERNEL_LDS, KERNEL_SMEM, KERNEL_CULL, KERNEL_CULL_LANE, KERNEL_CULL_FLAT,
                      TEXTURE_GLASS, TEXTURE_LAMBERTIAN, TEXTURE_METAL)
from .renderer import (BeginRenderingOperation, DrawNextFrame, EndRenderingOperation, RAY_HIT_DTYPE,
                       Renderer, RenderDesc, SetRenderDescription, SetRenderScene, frame_rays, lens_offsets,
                       ambient_dirs, render, denoise_host, denoise_scales, default_denoise_params,
                       reproject_host, motion_project, default_reproject_params, tile_pixel_map,
                       tile_slots, tiles_for_rank, reproject_moments_host, variance_host,
                       denoise_variance_host, default_reproject_moments_params,
                       default_variance_params, default_denoise_variance_params,
                       sample_counts_host)
from .scene import SPHERE_DTYPE, builtin_scene, make_spheres, scene_generator_text

__all__ = [
    "BeginRenderingOperation", "DrawNextFrame", "EndRenderingOperation", "Renderer",
    "RenderDesc", "SetRenderDescription", "SetRenderScene", "render", "tiles_for_rank",
    "tile_slots", "tile_pixel_map", "RAY_HIT_DTYPE", "lens_offsets", "frame_rays", "ambient_dirs",
    "denoise_host", "denoise_scales", "default_denoise_params",
    "reproject_host", "motion_project", "default_reproject_params",
    "reproject_moments_host", "variance_host", "denoise_variance_host",
    "default_reproject_moments_params", "default_variance_params",
    "default_denoise_variance_params", "sample_counts_host",
    "SPHERE_DTYPE", "builtin_scene", "make_spheres", "scene_generator_text", "VcrtError",
    "VK_SUCCESS", "VK_ERROR_INITIALIZATION_FAILED", "KERNEL_AUTO", "KERNEL_LDS", "KERNEL_SMEM",
    "KERNEL_CULL", "KERNEL_CULL_LANE", "KERNEL_CULL_FLAT", "TEXTURE_GLASS", "TEXTURE_LAMBERTIAN", "TEXTURE_METAL", "_native",
]
