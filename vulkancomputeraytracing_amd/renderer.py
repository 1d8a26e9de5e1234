"""Python mirror of the reference's Renderer lifecycle (include/Renderer.hpp:14-20).

``BeginRenderingOperation`` / ``DrawNextFrame`` / ``EndRenderingOperation`` keep the reference's
names and VkResult return convention (0 = VK_SUCCESS, negative = error). ``RenderDesc`` carries
what the reference fixed at compile time (globals.glsl:9-24). ``Renderer`` is the same lifecycle
as a context manager that raises on error. Everything goes through libvcrt.so (the C ABI of
include/vcrt.h); the compute runs in the gfx950 kernels of vcrt_tracer.hsaco.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from .scene import SPHERE_DTYPE, builtin_scene


@dataclass
class RenderDesc:
    width: int = 1280               # IMAGE_WIDTH  (globals.glsl:16)
    height: int = 720               # IMAGE_HEIGHT (globals.glsl:17)
    samples_per_pixel: int = 1      # SAMPLES_PER_PIXEL (globals.glsl:9-13)
    max_depth: int = 50             # MAX_RECURSION_LEVEL (globals.glsl:14)
    lookfrom: tuple = (13.0, 2.0, 3.0)   # globals.glsl:21-24
    lookat: tuple = (0.0, 0.0, 0.0)
    vup: tuple = (0.0, 1.0, 0.0)
    vfov: float = 20.0
    device: int = -1
    rank: int = 0
    world_size: int = 1             # shards: rank owns the 8x8 tiles with (tx + ty) % world == rank
    kernel_variant: int = N.KERNEL_AUTO
    blocks_per_cu: int = 0
    accumulate_chunk: int = 0       # samples per work item: 0 = from the frame (work_chunk)
    progressive: bool = False       # frame f continues the sample sequence; average of all frames
    code_object_path: str | None = None
    accumulate_tail: int = 0        # tail samples per pixel: 0 = the rule (work_tail), -1 = none
    accumulate_tail_chunk: int = 0  # samples per tail item; 0 = the rule
    accumulate_quantum: int = 0     # accumulation quantum G (the image depends on it alone):
                                    # 0 = the rule (work_quantum); >= spp: sequential order
    lens_radius: float = 0.0        # thin lens: aperture radius in world units (0 = the pinhole);
                                    # the plane through lookat is in focus (vcrt.h)
    _path_keepalive: bytes | None = field(default=None, repr=False)

    def to_c(self) -> N.vcrt_render_desc:
        d = N.vcrt_render_desc()
        N.lib().vcrt_default_desc(ctypes.byref(d))
        d.width, d.height = self.width, self.height
        d.samples_per_pixel, d.max_depth = self.samples_per_pixel, self.max_depth
        d.camera.lookfrom[:] = [float(v) for v in self.lookfrom]
        d.camera.lookat[:] = [float(v) for v in self.lookat]
        d.camera.vup[:] = [float(v) for v in self.vup]
        d.camera.vfov = float(self.vfov)
        d.device = self.device
        d.rank, d.world_size = self.rank, self.world_size
        d.kernel_variant = self.kernel_variant
        d.blocks_per_cu = self.blocks_per_cu
        d.accumulate_chunk = self.accumulate_chunk
        d.progressive = 1 if self.progressive else 0
        d.accumulate_tail = self.accumulate_tail
        d.accumulate_tail_chunk = self.accumulate_tail_chunk
        d.accumulate_quantum = self.accumulate_quantum
        d.lens_radius = float(self.lens_radius)
        if self.code_object_path:
            self._path_keepalive = self.code_object_path.encode()
            d.code_object_path = self._path_keepalive
        return d

    def with_camera(self, lookfrom=None, lookat=None, vup=None, vfov=None) -> "RenderDesc":
        """A copy of this description with the given camera fields; omitted ones keep their
        value."""
        import dataclasses
        changes = {}
        for name, v in (("lookfrom", lookfrom), ("lookat", lookat), ("vup", vup)):
            if v is not None:
                v = tuple(float(x) for x in v)
                if len(v) != 3:
                    raise ValueError(f"{name}: three components expected")
                changes[name] = v
        if vfov is not None:
            changes["vfov"] = float(vfov)
        return dataclasses.replace(self, **changes)


def work_quantum(desc: RenderDesc) -> int:
    """The accumulation quantum G the renderer uses for `desc`, from the C ABI
    (vcrt_work_quantum: host only, no GPU): the oracle's `quantum` for the same image."""
    return N.check_count("vcrt_work_quantum",
                         N.lib().vcrt_work_quantum(ctypes.byref(desc.to_c())))


def work_chunk(desc: RenderDesc) -> int:
    """Samples per work item of the head the renderer uses for `desc`, from the C ABI
    (vcrt_work_chunk: host only, no GPU). A scheduling choice: the image depends on the
    quantum (work_quantum) only."""
    return N.check_count("vcrt_work_chunk", N.lib().vcrt_work_chunk(ctypes.byref(desc.to_c())))


def work_tail(desc: RenderDesc) -> tuple[int, int]:
    """(tail samples per pixel, samples per tail item) the renderer uses for `desc`, from the
    C ABI (vcrt_work_tail: host only, no GPU); (0, 0) when there is no tail."""
    kt = ctypes.c_int32(0)
    t = N.check_count("vcrt_work_tail", N.lib().vcrt_work_tail(ctypes.byref(desc.to_c()),
                                                                ctypes.byref(kt)))
    return (t, kt.value) if t > 0 else (0, 0)


def lens_offsets(desc: RenderDesc, first: int, count: int) -> np.ndarray:
    """float32 [count, 3]: the thin lens's origin offsets of sample indices first .. first+count-1
    for `desc` (vcrt_lens_offsets: host only, no GPU); all +0 for the pinhole (lens_radius 0)."""
    out = np.zeros((int(count), 3), np.float32)
    N.check_count("vcrt_lens_offsets",
                  N.lib().vcrt_lens_offsets(ctypes.byref(desc.to_c()), int(first), int(count),
                                            out.ctypes.data_as(ctypes.c_void_p)))
    return out


MAX_SAMPLE_INDEX = 1 << 19  # sample indices a renderer admits (vcrt.h vcrt_lens_offsets)


def _check_sample_range(first, n) -> tuple[int, int]:
    """(first, n) of a range of sample indices, validated before any native call."""
    try:
        first, n = int(first), int(n)
    except (TypeError, ValueError) as e:
        raise ValueError(f"first, samples: integers expected ({e})") from None
    if first < 0:
        raise ValueError("first must be >= 0")
    if n < 1:
        raise ValueError("at least one sample")
    if first + n > MAX_SAMPLE_INDEX:
        raise ValueError("first + samples must not exceed 2^19")
    return first, n


def frame_rays(desc: RenderDesc, xy, first: int, n: int) -> tuple[np.ndarray, np.ndarray]:
    """The rays a frame of `desc` traces for the pixels xy [npixels, 2] (x, y) and the sample
    indices first .. first + n - 1 (vcrt_frame_rays: host only, no GPU), the definition behind
    Renderer.draw_features: (origins, dirs), float32 [npixels, n, 3] each."""
    first, n = _check_sample_range(first, n)
    try:
        xy = np.ascontiguousarray(xy, dtype=np.int32)
    except (TypeError, ValueError) as e:
        raise ValueError(f"xy: not convertible to an int32 array ({e})") from None
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError(f"xy: shape [npixels, 2] expected, got {tuple(xy.shape)}")
    if len(xy) and (xy.min() < 0 or xy[:, 0].max() >= desc.width or xy[:, 1].max() >= desc.height):
        raise ValueError("xy: a pixel outside the frame")
    origins = np.zeros((len(xy), n, 3), np.float32)
    dirs = np.zeros((len(xy), n, 3), np.float32)
    N.check_count("vcrt_frame_rays", N.lib().vcrt_frame_rays(
        ctypes.byref(desc.to_c()), xy.ctypes.data, len(xy), first, n, origins.ctypes.data,
        dirs.ctypes.data))
    return origins, dirs


MAX_AMBIENT_RAYS = 4096      # samples * rays of one draw_occlusion (vcrt.h vcrt_draw_occlusion)
MAX_AMBIENT_INDEX = 1 << 22  # ambient directions a renderer admits (vcrt.h vcrt_ambient_dirs)


def ambient_dirs(first: int, count: int) -> np.ndarray:
    """float32 [count, 3]: the unit vectors u_j of j = first .. first + count - 1 that
    Renderer.draw_occlusion adds to a hit's normal (vcrt_ambient_dirs: host only, no GPU)."""
    try:
        first, count = int(first), int(count)
    except (TypeError, ValueError) as e:
        raise ValueError(f"first, count: integers expected ({e})") from None
    if first < 0 or count < 0:
        raise ValueError("first and count must be >= 0")
    if first + count > MAX_AMBIENT_INDEX:
        raise ValueError("first + count must not exceed 2^22")
    out = np.zeros((count, 3), np.float32)
    N.check_count("vcrt_ambient_dirs", N.lib().vcrt_ambient_dirs(first, count, out.ctypes.data))
    return out


DENOISE_FIELDS = ("levels", "sigma_normal", "sigma_depth", "sigma_albedo", "sigma_colour",
                  "demodulate")
_DENOISE_INTEGER_FIELDS = ("levels", "demodulate")


def default_denoise_params() -> dict:
    """vcrt_default_denoise_params as a dict: levels, the four sigmas and demodulate."""
    p = N.vcrt_denoise_params()
    N.check("vcrt_default_denoise_params", N.lib().vcrt_default_denoise_params(ctypes.byref(p)))
    return {f: getattr(p, f) for f in DENOISE_FIELDS}


def _denoise_params(given: dict) -> N.vcrt_denoise_params:
    return _float_params("denoise", N.vcrt_denoise_params, "vcrt_default_denoise_params",
                         DENOISE_FIELDS, given, integer=_DENOISE_INTEGER_FIELDS)


def denoise_scales(**params) -> np.ndarray:
    """float32 [4]: k_normal, k_depth, k_albedo, k_colour = 1 / sigma^2 (0 for sigma 0) of the
    denoiser's parameters (vcrt_denoise_scales: host only, no GPU)."""
    k = np.zeros(4, np.float32)
    p = _denoise_params(params)
    N.check("vcrt_denoise_scales", N.lib().vcrt_denoise_scales(ctypes.byref(p), k.ctypes.data))
    return k


def denoise_host(colour, albedo=None, normal_depth=None, **params) -> np.ndarray:
    """The denoiser's definition on the host (vcrt_denoise_host: no GPU): the edge-avoiding
    a-trous filter of vcrt.h over numpy planes [height, width, 4]; Renderer.denoise computes the
    same bits on the GPU. params: levels, sigma_normal, sigma_depth, sigma_albedo, sigma_colour,
    demodulate (omitted: default_denoise_params)."""
    if _is_torch(colour):
        raise ValueError("denoise_host takes numpy planes")
    colour, albedo, normal_depth = _check_image_planes(
        dict(colour=colour, albedo=albedo, normal_depth=normal_depth),
        optional=("albedo", "normal_depth")).values()
    p = _denoise_params(params)
    out = np.empty_like(colour)
    N.check("vcrt_denoise_host", N.lib().vcrt_denoise_host(
        colour.ctypes.data, None if albedo is None else albedo.ctypes.data,
        None if normal_depth is None else normal_depth.ctypes.data,
        colour.shape[1], colour.shape[0], ctypes.byref(p), out.ctypes.data))
    return out


REPROJECT_FIELDS = ("alpha", "max_history", "depth_tolerance")


def default_reproject_params() -> dict:
    """vcrt_default_reproject_params as a dict: alpha, max_history, depth_tolerance."""
    p = N.vcrt_reproject_params()
    N.check("vcrt_default_reproject_params",
            N.lib().vcrt_default_reproject_params(ctypes.byref(p)))
    return {f: getattr(p, f) for f in REPROJECT_FIELDS}


def _reproject_params(given: dict) -> N.vcrt_reproject_params:
    return _float_params("reproject", N.vcrt_reproject_params, "vcrt_default_reproject_params",
                         REPROJECT_FIELDS, given)


REPROJECT_PLANES = ("colour", "motion", "history_colour", "history_surface", "history_length")


def reproject_host(colour, motion, history_colour, history_surface, history_length, **params):
    """Temporal accumulation's definition on the host (vcrt_reproject_host: no GPU) over numpy
    planes [height, width, 4] and history_length [height, width]: (out, out_length);
    Renderer.reproject computes the same bits on the GPU. params: alpha, max_history,
    depth_tolerance (omitted: default_reproject_params)."""
    if _is_torch(colour):
        raise ValueError("reproject_host takes numpy planes")
    pl = _check_image_planes(dict(colour=colour, motion=motion, history_colour=history_colour,
                                  history_surface=history_surface,
                                  history_length=history_length), scalar=("history_length",))
    p = _reproject_params(params)
    c = pl["colour"]
    out, length = np.empty_like(c), np.empty(c.shape[:2], np.float32)
    N.check("vcrt_reproject_host", N.lib().vcrt_reproject_host(
        *(pl[n].ctypes.data for n in REPROJECT_PLANES), c.shape[1], c.shape[0], ctypes.byref(p),
        out.ctypes.data, length.ctypes.data))
    return out, length


REPROJECT_MOMENTS_FIELDS = REPROJECT_FIELDS + ("alpha_moments",)
VARIANCE_FIELDS = ("min_history", "alpha")


def _float_params(call: str, struct, default_fn: str, fields, given: dict, integer=()):
    """The C parameter block `struct`: the defaults with the fields `given` names (None: the
    default), floats but for the names in `integer`."""
    unknown = set(given) - set(fields)
    if unknown:
        raise TypeError(f"{call}: unexpected parameters {sorted(unknown)}")
    p = struct()
    N.check(default_fn, getattr(N.lib(), default_fn)(ctypes.byref(p)))
    for name, v in given.items():
        if v is None:
            continue
        try:
            setattr(p, name, int(v) if name in integer else float(v))
        except (TypeError, ValueError, OverflowError) as e:
            raise ValueError(f"{call}: {name}: a number expected ({e})") from None
    return p


def _reproject_moments_params(given: dict) -> N.vcrt_reproject_moments_params:
    return _float_params("reproject_moments", N.vcrt_reproject_moments_params,
                         "vcrt_default_reproject_moments_params", REPROJECT_MOMENTS_FIELDS, given)


def _variance_params(given: dict) -> N.vcrt_variance_params:
    return _float_params("variance", N.vcrt_variance_params, "vcrt_default_variance_params",
                         VARIANCE_FIELDS, given)


def _denoise_variance_params(given: dict) -> N.vcrt_denoise_params:
    return _float_params("denoise_variance", N.vcrt_denoise_params,
                         "vcrt_default_denoise_variance_params", DENOISE_FIELDS, given,
                         integer=_DENOISE_INTEGER_FIELDS)


def default_reproject_moments_params() -> dict:
    """vcrt_default_reproject_moments_params as a dict: reproject's fields and alpha_moments."""
    p = _reproject_moments_params({})
    return {f: getattr(p, f) for f in REPROJECT_MOMENTS_FIELDS}


def default_variance_params() -> dict:
    """vcrt_default_variance_params as a dict: min_history, alpha."""
    p = _variance_params({})
    return {f: getattr(p, f) for f in VARIANCE_FIELDS}


def default_denoise_variance_params() -> dict:
    """vcrt_default_denoise_variance_params as a dict: denoise's fields."""
    p = _denoise_variance_params({})
    return {f: getattr(p, f) for f in DENOISE_FIELDS}


def _check_image_planes(planes: dict, scalar=(), optional=()) -> dict:
    """Planes of one image call, validated before any native call: numpy float32 C-contiguous
    (converted) or torch float32 contiguous tensors on one CUDA device (as they are). The first
    plane is [height, width, 4] and sets the shape; the names in `scalar` are [height, width], the
    others [height, width, 4]; the names in `optional` may be None. Raises ValueError."""
    first_name = next(iter(planes))
    first = planes[first_name]
    if first is None:
        raise ValueError(f"{first_name}: a plane expected")
    torch_in = _is_torch(first)
    out = {}
    shape = None
    for name, a in planes.items():
        if a is None:
            if name not in optional:
                raise ValueError(f"{name}: a plane expected")
            out[name] = None
            continue
        if _is_torch(a) != torch_in:
            raise ValueError("the planes must all be numpy arrays or all torch tensors")
        if torch_in:
            import torch
            if a.dtype != torch.float32 or not a.is_cuda or not a.is_contiguous():
                raise ValueError(f"{name}: a contiguous float32 CUDA tensor expected")
            if a.device != first.device:
                raise ValueError(f"{name}: torch tensors must be on one CUDA device")
        else:
            try:
                a = np.ascontiguousarray(a, dtype=np.float32)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{name}: not convertible to a float32 array ({e})") from None
        if shape is None:
            if a.ndim != 3 or a.shape[2] != 4:
                raise ValueError(f"{name}: shape [height, width, 4] expected, "
                                 f"got {tuple(a.shape)}")
            shape = tuple(a.shape)
        elif name in scalar:
            if tuple(a.shape) != shape[:2]:
                raise ValueError(f"{name}: shape [height, width] of the {first_name} plane "
                                 f"expected, got {tuple(a.shape)}")
        elif tuple(a.shape) != shape:
            raise ValueError(f"{name}: shape [height, width, 4] of the {first_name} plane "
                             f"expected, got {tuple(a.shape)}")
        out[name] = a
    return out


MOMENTS_PLANES = ("colour", "motion", "history_colour", "history_surface", "history_length",
                  "albedo", "history_moments")


def _ptr(a):
    """The address of a checked plane (None: NULL)."""
    if a is None:
        return None
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


def _stats_dict(st, keys=None, unnamed: str = "") -> dict:
    """A stats struct as a dict: `keys` in their order (None: the struct's fields in theirs), then
    "kernel" (`unnamed` when the call launched nothing and left the name empty)."""
    if keys is None:
        keys = [f for f, _ in st._fields_ if f != "kernel"]
    return {**{k: getattr(st, k) for k in keys}, "kernel": st.kernel.decode() or unnamed}


def reproject_moments_host(colour, motion, history_colour, history_surface, history_length,
                           history_moments, albedo=None, **params):
    """Temporal accumulation with luminance moments, the definition on the host
    (vcrt_reproject_moments_host: no GPU) over numpy planes: (out, out_length, out_moments);
    Renderer.reproject_moments computes the same bits on the GPU. params: alpha, max_history,
    depth_tolerance, alpha_moments (omitted: default_reproject_moments_params)."""
    if _is_torch(colour):
        raise ValueError("reproject_moments_host takes numpy planes")
    pl = _check_image_planes(dict(colour=colour, motion=motion, history_colour=history_colour,
                                  history_surface=history_surface,
                                  history_length=history_length, albedo=albedo,
                                  history_moments=history_moments),
                             scalar=("history_length",), optional=("albedo",))
    p = _reproject_moments_params(params)
    c = pl["colour"]
    out, length = np.empty_like(c), np.empty(c.shape[:2], np.float32)
    moments = np.empty_like(c)
    N.check("vcrt_reproject_moments_host", N.lib().vcrt_reproject_moments_host(
        *(_ptr(pl[n]) for n in MOMENTS_PLANES), c.shape[1], c.shape[0], ctypes.byref(p),
        out.ctypes.data, length.ctypes.data, moments.ctypes.data))
    return out, length, moments


def variance_host(moments, surface, **params) -> np.ndarray:
    """The per-pixel variance of the accumulated luminance, the definition on the host
    (vcrt_variance_host: no GPU) over numpy planes [height, width, 4]: float32 [height, width];
    Renderer.variance computes the same bits on the GPU. params: min_history, alpha (omitted:
    default_variance_params)."""
    if _is_torch(moments):
        raise ValueError("variance_host takes numpy planes")
    pl = _check_image_planes(dict(moments=moments, surface=surface))
    p = _variance_params(params)
    m = pl["moments"]
    out = np.empty(m.shape[:2], np.float32)
    N.check("vcrt_variance_host", N.lib().vcrt_variance_host(
        m.ctypes.data, pl["surface"].ctypes.data, m.shape[1], m.shape[0], ctypes.byref(p),
        out.ctypes.data))
    return out


SAMPLE_MAX_COUNT = 256  # vcrt_draw_samples' and vcrt_sample_counts' largest max_count


def _sample_count_params(target, min_count, max_count) -> N.vcrt_sample_count_params:
    """vcrt_sample_counts' parameters, validated before any native call."""
    try:
        target, min_count, max_count = float(target), int(min_count), int(max_count)
    except (TypeError, ValueError) as e:
        raise ValueError(f"target, min_count, max_count: numbers expected ({e})") from None
    if not (target > 0.0 and np.isfinite(target)):
        raise ValueError("target must be positive and finite")
    if not 0 <= min_count <= max_count <= SAMPLE_MAX_COUNT:
        raise ValueError(f"0 <= min_count <= max_count <= {SAMPLE_MAX_COUNT} expected")
    p = N.vcrt_sample_count_params()
    p.struct_size = ctypes.sizeof(N.vcrt_sample_count_params)
    p.target, p.min_count, p.max_count = target, min_count, max_count
    return p


def _check_count_elements(n: int) -> None:
    if not 1 <= n <= 1 << 31:
        raise ValueError("variance: 1 .. 2^31 elements expected")


def _variance_plane(variance) -> np.ndarray:
    try:
        variance = np.ascontiguousarray(variance, dtype=np.float32)
    except (TypeError, ValueError) as e:
        raise ValueError(f"variance: not convertible to a float32 array ({e})") from None
    _check_count_elements(variance.size)
    return variance


def sample_counts_host(variance, target: float, min_count: int = 0, max_count: int = 64,
                       stats: bool = False):
    """The count plane of Renderer.draw_samples from a variance plane, the definition on the
    host (vcrt_sample_counts_host: no GPU): counts[e] = max(c, min_count) with t = max(variance[e],
    0) * (1 / target^2) and c = max_count if t >= max_count else ceil(t), uint16 in variance's
    shape; Renderer.sample_counts computes the same bits on the GPU. With stats=True the result
    is (counts, total)."""
    if _is_torch(variance):
        raise ValueError("sample_counts_host takes a numpy plane")
    p = _sample_count_params(target, min_count, max_count)
    variance = _variance_plane(variance)
    out = np.empty(variance.shape, np.uint16)
    st = N.vcrt_sample_count_stats()
    N.check("vcrt_sample_counts_host", N.lib().vcrt_sample_counts_host(
        variance.ctypes.data, variance.size, ctypes.byref(p), out.ctypes.data, ctypes.byref(st)))
    return (out, st.total) if stats else out


def denoise_variance_host(colour, variance, albedo=None, normal_depth=None, **params):
    """The variance-steered denoiser's definition on the host (vcrt_denoise_variance_host: no
    GPU) over numpy planes: (out [height, width, 4], out_variance [height, width]);
    Renderer.denoise_variance computes the same bits on the GPU. params: denoise's (omitted:
    default_denoise_variance_params)."""
    if _is_torch(colour):
        raise ValueError("denoise_variance_host takes numpy planes")
    pl = _check_image_planes(dict(colour=colour, albedo=albedo, normal_depth=normal_depth,
                                  variance=variance), scalar=("variance",),
                             optional=("albedo", "normal_depth"))
    p = _denoise_variance_params(params)
    c = pl["colour"]
    out, out_var = np.empty_like(c), np.empty(c.shape[:2], np.float32)
    N.check("vcrt_denoise_variance_host", N.lib().vcrt_denoise_variance_host(
        c.ctypes.data, _ptr(pl["albedo"]), _ptr(pl["normal_depth"]), pl["variance"].ctypes.data,
        c.shape[1], c.shape[0], ctypes.byref(p), out.ctypes.data, out_var.ctypes.data))
    return out, out_var


def _camera_c(desc: RenderDesc, camera) -> N.vcrt_camera:
    """A vcrt_camera from `camera`: a RenderDesc, or a dict of the camera fields that differ from
    desc's (lookfrom, lookat, vup, vfov)."""
    if isinstance(camera, RenderDesc):
        return camera.to_c().camera
    if not isinstance(camera, dict) or set(camera) - {"lookfrom", "lookat", "vup", "vfov"}:
        raise ValueError("camera: a RenderDesc or a dict of lookfrom, lookat, vup, vfov expected")
    return desc.with_camera(**camera).to_c().camera


def motion_project(desc: RenderDesc, points, prev_camera=None) -> np.ndarray:
    """float32 [n, 3]: (px, py, z') of the world points [n, 3] through the camera prev_camera
    (None: desc's; a RenderDesc or a dict of camera fields) at desc's size -- the projection of
    Renderer.draw_motion (vcrt_motion_project: host only, no GPU). A NaN triple where a point
    does not project."""
    try:
        pts = np.ascontiguousarray(points, dtype=np.float32)
    except (TypeError, ValueError) as e:
        raise ValueError(f"points: not convertible to a float32 array ({e})") from None
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points: shape [n, 3] expected, got {tuple(pts.shape)}")
    out = np.empty_like(pts)
    cam = None if prev_camera is None else ctypes.byref(_camera_c(desc, prev_camera))
    N.check("vcrt_motion_project", N.lib().vcrt_motion_project(
        ctypes.byref(desc.to_c()), cam, pts.ctypes.data, len(pts), out.ctypes.data))
    return out


def pixel_scale_log2(max_abs_quantum_sum: float) -> int:
    """s of a pixel's quantization scale 2^s from its largest |quantum sum| (vcrt_pixel_scale_log2:
    host only, no GPU): 32 below 2^12, else the largest s with max * 2^s < 2^44. The oracle
    restates the same rule (oracle_pixel_scale_log2)."""
    return N.lib().vcrt_pixel_scale_log2(float(max_abs_quantum_sum))


def tiles_for_rank(width: int, height: int, world: int, rank: int) -> list[int]:
    """Row-major 8x8 tile indices (ty * tiles_x + tx) rank `rank` renders, in its local order:
    the tiles with (tx + ty) % world == rank (csrc/vcrt_math.h tile_of)."""
    tx_n, ty_n = (width + 7) // 8, (height + 7) // 8
    return [ty * tx_n + tx for ty in range(ty_n) for tx in range(tx_n)
            if (tx + ty) % world == rank]


def tile_slots(width: int, height: int, world: int = 1, rank: int = 0) -> int:
    """64 work slots per owned tile (edge tiles included whole)."""
    return 64 * len(tiles_for_rank(width, height, world, rank))


def tile_pixel_map(width: int, height: int, world: int) -> np.ndarray:
    """For every frame pixel [y, x]: (rank, element index in that rank's packed tile buffer).
    The host statement of the index map the vcrt_assemble kernel applies (owner_of)."""
    tx_n, ty_n = (width + 7) // 8, (height + 7) // 8
    rank_of = np.zeros((ty_n, tx_n), np.int64)
    local_of = np.zeros((ty_n, tx_n), np.int64)
    for r in range(world):
        for lt, t in enumerate(tiles_for_rank(width, height, world, r)):
            rank_of[t // tx_n, t % tx_n] = r
            local_of[t // tx_n, t % tx_n] = lt
    y, x = np.mgrid[0:height, 0:width]
    return np.stack([rank_of[y // 8, x // 8],
                     local_of[y // 8, x // 8] * 64 + (y % 8) * 8 + x % 8], axis=-1)


# ---- ray queries --------------------------------------------------------------------------

# vcrt_ray_hit (include/vcrt.h), 32 bytes: the first segment of a queried ray's path
RAY_HIT_DTYPE = np.dtype([
    ("t", np.float32),
    ("sphere", np.int32),
    ("segments", np.uint32),
    ("reserved", np.uint32),
    ("normal", np.float32, (3,)),
    ("reserved2", np.float32),
])


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _check_rays(origins, dirs):
    """The two ray arrays of Renderer.trace_rays, validated before any native call: numpy
    float32 C-contiguous [n, 3] (converted), or torch float32 contiguous [n, 3] on one CUDA
    device (as they are). Raises ValueError."""
    if _is_torch(origins) != _is_torch(dirs):
        raise ValueError("origins and dirs must both be numpy arrays or both torch tensors")
    if _is_torch(origins):
        import torch
        for name, a in (("origins", origins), ("dirs", dirs)):
            if a.dtype != torch.float32:
                raise ValueError(f"{name}: torch tensors must be float32, not {a.dtype}")
            if not a.is_cuda or a.device != origins.device:
                raise ValueError(f"{name}: torch tensors must be on one CUDA device")
            if not a.is_contiguous():
                raise ValueError(f"{name}: torch tensors must be contiguous")
    else:
        try:
            origins = np.ascontiguousarray(origins, dtype=np.float32)
            dirs = np.ascontiguousarray(dirs, dtype=np.float32)
        except (TypeError, ValueError) as e:
            raise ValueError(f"origins, dirs: not convertible to float32 arrays ({e})") from None
    for name, a in (("origins", origins), ("dirs", dirs)):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name}: shape [n, 3] expected, got {tuple(a.shape)}")
    if origins.shape[0] != dirs.shape[0]:
        raise ValueError(f"origins has {origins.shape[0]} rays, dirs {dirs.shape[0]}")
    if origins.shape[0] > 1 << 30:
        raise ValueError("at most 2^30 rays per call")
    return origins, dirs


def _check_reach(tmax, n: int, origins):
    """Renderer.occluded's tmax for n rays held like `origins` (validated by _check_rays): None,
    or float32 [n] where the rays are -- numpy C-contiguous, or a torch tensor on their device. A
    scalar is broadcast (on the host, then copied: no torch kernel runs). Raises ValueError."""
    if tmax is None:
        return None
    rays_torch = _is_torch(origins)
    if _is_torch(tmax):
        import torch
        if not rays_torch:
            raise ValueError("tmax: a torch tensor with numpy rays")
        if tmax.dtype != torch.float32:
            raise ValueError(f"tmax: torch tensors must be float32, not {tmax.dtype}")
        if tmax.device != origins.device:
            raise ValueError("tmax: must be on the rays' device")
        if not tmax.is_contiguous():
            raise ValueError("tmax: torch tensors must be contiguous")
        if tmax.ndim != 1 or tmax.shape[0] != n:
            raise ValueError(f"tmax: shape [{n}] expected, got {tuple(tmax.shape)}")
        return tmax
    try:
        t = np.asarray(tmax, dtype=np.float32)
    except (TypeError, ValueError) as e:
        raise ValueError(f"tmax: not convertible to float32 ({e})") from None
    if t.ndim == 0:
        t = np.full(n, t, dtype=np.float32)
    elif rays_torch:
        raise ValueError("tmax: a scalar or a torch tensor with torch rays")
    if t.ndim != 1 or t.shape[0] != n:
        raise ValueError(f"tmax: shape [{n}] expected, got {tuple(t.shape)}")
    t = np.ascontiguousarray(t)
    if rays_torch:
        import torch
        return torch.from_numpy(t).to(origins.device)
    return t


# ---- reference-named lifecycle (VkResult codes, no exceptions) ----------------------------

_desc = RenderDesc()
_scene: np.ndarray | None = None


def SetRenderDescription(desc: RenderDesc) -> int:
    global _desc
    _desc = desc
    return N.VK_SUCCESS


def SetRenderScene(spheres) -> int:
    global _scene
    _scene = None if spheres is None else np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    return N.VK_SUCCESS


# The C ABI holds one renderer per process (vcrt.h): a vcrt_begin ends the one before it. The
# Renderer object that owns the current state; an older one is stale and its calls raise
# instead of acting on its successor's state (or ending it on close).
_live = None


def _retire_live() -> None:
    global _live
    if _live is not None:
        _live._open = False
        _live = None


def BeginRenderingOperation() -> int:
    _retire_live()
    lib = N.lib()
    d = _desc.to_c()
    r = lib.vcrt_begin(ctypes.byref(d))
    if r == N.VK_SUCCESS and _scene is not None:
        r = lib.vcrt_set_scene(_scene.ctypes.data_as(ctypes.POINTER(N.vcrt_sphere)), len(_scene))
        if r != N.VK_SUCCESS:
            lib.vcrt_end()
    return r


def DrawNextFrame() -> int:
    return N.lib().vcrt_draw_next_frame()


def EndRenderingOperation() -> int:
    _retire_live()
    return N.lib().vcrt_end()


# ---- the same lifecycle as an object --------------------------------------------------------

class Renderer:
    """Begin on construction / __enter__, End on close / __exit__; raises VcrtError."""

    def __init__(self, desc: RenderDesc | None = None, scene=None):
        self.desc = desc or RenderDesc()
        self._lib = N.lib()
        self._frame_stats = N.vcrt_stats()  # frame_times()' reused struct
        self._c_desc = self.desc.to_c()
        _retire_live()  # vcrt_begin ends the previous renderer's state
        N.check("vcrt_begin", self._lib.vcrt_begin(ctypes.byref(self._c_desc)))
        global _live
        _live = self
        self._open = True
        if scene is not None:
            self.set_scene(scene)

    def _L(self):
        """The library, for the renderer that owns the C ABI's state; a stale one raises."""
        if not getattr(self, "_open", False) or _live is not self:
            raise N.VcrtError("Renderer (closed, or replaced by a later one)",
                              N.VK_ERROR_INITIALIZATION_FAILED)
        return self._lib

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        global _live
        if getattr(self, "_open", False) and _live is self:
            self._lib.vcrt_end()
            _live = None
        self._open = False

    def set_scene(self, scene) -> None:
        arr = builtin_scene(scene) if isinstance(scene, (str, int)) else scene
        arr = np.ascontiguousarray(arr, dtype=SPHERE_DTYPE)
        self._scene = arr
        N.check("vcrt_set_scene", self._L().vcrt_set_scene(
            arr.ctypes.data_as(ctypes.POINTER(N.vcrt_sphere)), len(arr)))

    def draw_next_frame(self) -> None:
        N.check("vcrt_draw_next_frame", self._L().vcrt_draw_next_frame())

    def comm_init(self, comm_id: bytes) -> None:
        """Join the multi-GPU frame gather (vcrt_comm_init, RCCL inside libvcrt): every rank
        passes the same id (comm_unique_id() of rank 0). Afterwards draw_next_frame on rank 0
        returns the whole frame, which read_framebuffer gives as [height, width, 4]."""
        raw = bytes(comm_id)
        if len(raw) != ctypes.sizeof(N.vcrt_comm_id):
            raise ValueError("a comm id is 128 bytes (vcrt_comm_unique_id)")
        cid = N.vcrt_comm_id()
        ctypes.memmove(ctypes.addressof(cid), raw, len(raw))  # c_char arrays stop at NUL
        N.check("vcrt_comm_init", self._L().vcrt_comm_init(ctypes.byref(cid)))
        self._gathering = True

    def local_layout(self) -> tuple[int, int]:
        """(float4 elements, tiles) of the rank-local framebuffer."""
        e, t = ctypes.c_uint32(), ctypes.c_uint32()
        N.check("vcrt_local_layout", self._L().vcrt_local_layout(ctypes.byref(e), ctypes.byref(t)))
        return e.value, t.value

    def _frame_shape(self) -> tuple[int, ...]:
        elems, tiles = self.local_layout()
        if elems == self.desc.width * self.desc.height and (
                self.desc.world_size == 1 or getattr(self, "_gathering", False)):
            return (self.desc.height, self.desc.width, 4)
        return (tiles, 64, 4)

    def read_framebuffer(self) -> np.ndarray:
        """Framebuffer, float32 rgba: the frame [height, width, 4] (top row first) at world 1 and
        on rank 0 after comm_init; otherwise the rank's packed tiles [tiles, 64, 4] (element
        8*(y%8) + x%8)."""
        shape = self._frame_shape()
        out = np.empty(shape, dtype=np.float32)
        N.check("vcrt_read_framebuffer", self._L().vcrt_read_framebuffer(
            out.ctypes.data_as(ctypes.c_void_p), out.size))
        return out

    def read_framebuffer_srgb8(self) -> np.ndarray:
        """The rank-local framebuffer as sRGB8 RGBA (what the reference's B8G8R8A8_SRGB
        swapchain shows), uint8 with the read_framebuffer shape."""
        shape = self._frame_shape()
        out = np.empty(shape, dtype=np.uint8)
        N.check("vcrt_read_framebuffer_srgb8", self._L().vcrt_read_framebuffer_srgb8(
            out.ctypes.data_as(ctypes.c_void_p), out.size))
        return out

    def reset_accumulation(self) -> None:
        N.check("vcrt_reset_accumulation", self._L().vcrt_reset_accumulation())

    def set_camera(self, lookfrom=None, lookat=None, vup=None, vfov=None) -> None:
        """Move the camera between frames (vcrt_set_camera); omitted fields keep their value and
        `self.desc` follows. Later frames are bit for bit those of a fresh Renderer with the new
        description; the scene, its tables, the framebuffers and the device state are kept, the
        camera-ray lists are rebuilt on the GPU and progressive accumulation restarts."""
        new = self.desc.with_camera(lookfrom, lookat, vup, vfov)
        cam = new.to_c().camera
        N.check("vcrt_set_camera", self._L().vcrt_set_camera(ctypes.byref(cam)))
        self.desc = new
        self._c_desc.camera = cam

    def camera_stats(self) -> dict:
        """The last set_camera (vcrt_get_camera_stats): host_ms, lists_ms, on_device, quarters,
        group_ids, pair_records."""
        s = N.vcrt_camera_stats()
        N.check("vcrt_get_camera_stats", self._L().vcrt_get_camera_stats(ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in N.vcrt_camera_stats._fields_
                if name != "reserved"}

    def camera_lists(self) -> dict:
        """The camera-ray lists the next frame will use, read back from the device
        (vcrt_camera_lists_read) in the form of scene.primary_lists / primary_sphere_lists:
        group_info, sphere_info uint32 [4 x local tiles], ids uint16, rec float32 [pairs, 12].
        All empty when the renderer has no lists (no culling tables, a lens)."""
        lib = self._L()
        nids, npairs = ctypes.c_int32(0), ctypes.c_int32(0)
        n = N.check_count("vcrt_camera_lists_read", lib.vcrt_camera_lists_read(
            None, None, 0, None, 0, None, 0, ctypes.byref(nids), ctypes.byref(npairs)))
        ginfo, sinfo = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        ids = np.zeros(nids.value, np.uint16)
        rec = np.zeros((npairs.value, 12), np.float32)
        if n:
            N.check_count("vcrt_camera_lists_read", lib.vcrt_camera_lists_read(
                ginfo.ctypes.data_as(ctypes.c_void_p), sinfo.ctypes.data_as(ctypes.c_void_p), n,
                ids.ctypes.data_as(ctypes.c_void_p), len(ids),
                rec.ctypes.data_as(ctypes.c_void_p), rec.size, None, None))
        return {"group_info": ginfo, "ids": ids, "sphere_info": sinfo, "rec": rec}

    def update_spheres(self, spheres) -> None:
        """Replace the values of the current scene's spheres between frames
        (vcrt_update_spheres): the count stays, the scene's grouping is kept and every table is
        refitted on the GPU. Later frames and ray queries are bit for bit those of a fresh
        Renderer with the new scene; after large moves they get slower, never wrong (set_scene
        regroups). A numpy [n, 10] float32 array, or whatever set_scene accepts, goes through the
        host call; a contiguous torch float32 [n, 10] tensor on the renderer's device goes
        through the device call on its data_ptr(), after the caller's current stream is
        synchronised. Progressive accumulation restarts."""
        lib = self._L()
        if _is_torch(spheres):
            import torch
            t = spheres
            if t.dtype != torch.float32 or t.ndim != 2 or t.shape[1] != 10:
                raise ValueError("spheres: a torch tensor must be float32 [n, 10]")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("spheres: a torch tensor must be contiguous and on a CUDA device")
            if self.desc.device >= 0 and t.device.index != self.desc.device:
                raise ValueError(f"spheres on {t.device}, the renderer on device {self.desc.device}")
            torch.cuda.current_stream(t.device).synchronize()
            N.check("vcrt_update_spheres_device",
                    lib.vcrt_update_spheres_device(t.data_ptr(), int(t.shape[0])))
            self._scene = None  # the values live on the device
            return
        arr = builtin_scene(spheres) if isinstance(spheres, (str, int)) else spheres
        arr = np.asarray(arr)
        if arr.dtype != SPHERE_DTYPE:
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            if arr.ndim != 2 or arr.shape[1] != 10:
                raise ValueError(f"spheres: shape [n, 10] expected, got {arr.shape}")
            arr = arr.view(SPHERE_DTYPE).reshape(-1)
        arr = np.ascontiguousarray(arr)
        N.check("vcrt_update_spheres", lib.vcrt_update_spheres(arr.ctypes.data, len(arr)))
        self._scene = arr

    def scene_update_stats(self) -> dict:
        """The last update_spheres (vcrt_get_scene_update_stats): host_ms, refit_ms, lists_ms,
        on_device, rebuilt, groups, boxes, footprint_cells."""
        s = N.vcrt_scene_update_stats()
        N.check("vcrt_get_scene_update_stats",
                self._L().vcrt_get_scene_update_stats(ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in N.vcrt_scene_update_stats._fields_}

    def scene_table(self, name: str):
        """One of the scene's device tables read back (vcrt_scene_table_read), whoever wrote it:
        a flat numpy array of the table's words (`_native.SCENE_TABLES`), a dict for "scalars",
        None when the renderer has no such table."""
        from .scene import table_from_bytes
        tid, _ = N.SCENE_TABLES[name]
        lib = self._L()
        n = N.check_count("vcrt_scene_table_read", lib.vcrt_scene_table_read(tid, None, 0))
        if n == 0:
            return None
        buf = np.zeros(n, np.uint8)
        N.check_count("vcrt_scene_table_read", lib.vcrt_scene_table_read(tid, buf.ctypes.data, n))
        return table_from_bytes(name, buf)

    def framebuffer_device(self) -> tuple[int, int]:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        N.check("vcrt_framebuffer_device",
                self._L().vcrt_framebuffer_device(ctypes.byref(p), ctypes.byref(n)))
        return p.value or 0, n.value

    def set_framebuffer_device(self, ptr: int | None, nbytes: int = 0) -> None:
        N.check("vcrt_set_framebuffer_device",
                self._L().vcrt_set_framebuffer_device(ctypes.c_void_p(ptr or None), nbytes))

    def assemble_tiles(self, gathered_ptr: int, frame_ptr: int, tiles_per_rank: int) -> None:
        d = self.desc
        N.check("vcrt_assemble_tiles", self._L().vcrt_assemble_tiles(
            ctypes.c_void_p(gathered_ptr), ctypes.c_void_p(frame_ptr), d.width, d.height,
            d.world_size, tiles_per_rank))

    def _local_lead(self) -> tuple[int, ...]:
        """The leading shape of the rank-local framebuffer's planes: [height, width] at world 1,
        else the packed tiles [tiles, 64]."""
        elems, tiles = self.local_layout()
        return ((self.desc.height, self.desc.width) if self.desc.world_size == 1
                else (tiles, 64))

    def _torch_device(self):
        import torch
        return torch.device("cuda", self.desc.device if self.desc.device >= 0
                            else torch.cuda.current_device())

    def _frame_planes(self, device: bool, channels) -> list:
        """Zero-filled output planes of a frame pass in the rank-local leading shape, one per
        entry of `channels`: c > 0 a float32 [..., c] plane, 0 an int32 [...] one, None none.
        numpy, or with device=True torch tensors on the renderer's device, the caller's current
        stream synchronised behind them: the device call may follow."""
        lead = self._local_lead()
        if not device:
            return [None if c is None else
                    np.zeros(lead + ((c,) if c else ()), np.float32 if c else np.int32)
                    for c in channels]
        import torch
        dev = self._torch_device()
        planes = [None if c is None else
                  torch.zeros(lead + ((c,) if c else ()), device=dev,
                              dtype=torch.float32 if c else torch.int32) for c in channels]
        torch.cuda.current_stream(dev).synchronize()
        return planes

    def trace_rays(self, origins, dirs, max_depth: int | None = None, hits: bool = False,
                   stats: bool = False):
        """Radiance and first hit of caller-supplied rays against the current scene
        (vcrt_trace_rays): any camera model, picking, probes (the frame's own albedo and normal
        buffers: draw_features).

        numpy inputs [n, 3] (anything np.ascontiguousarray(..., float32) takes) go through the
        host call and return the radiance as float32 [n, 4] (rgb = ray_color, alpha 1) and, with
        hits=True, a RAY_HIT_DTYPE array [n]. torch float32 tensors [n, 3] on the renderer's device
        go through the device call on their data_ptr(), after the caller's current stream is
        synchronised, and return a torch float32 [n, 4] and, with hits=True, an int32 [n, 8]
        tensor of the records' raw words: column 1 is the sphere index and column 2 the segment
        count; columns 0 (t) and 4..6 (normal) hold float bits, read them as
        h[:, [0, 4, 5, 6]].view(torch.float32); columns 3 and 7 are 0.

        max_depth=None takes the description's depth. Returns the radiance alone, or a tuple
        (radiance[, hits][, stats dict]) in that order. Shape and dtype errors raise ValueError
        before any native call. The framebuffer and the frame statistics are left alone."""
        origins, dirs = _check_rays(origins, dirs)
        depth = self.desc.max_depth if max_depth is None else int(max_depth)
        if depth < 0:
            raise ValueError("max_depth must be >= 0")
        n = int(origins.shape[0])
        st = N.vcrt_ray_stats()
        if _is_torch(origins):
            import torch
            dev = origins.device
            if self.desc.device >= 0 and dev.index != self.desc.device:
                raise ValueError(f"rays on {dev}, the renderer on device {self.desc.device}")
            lib = self._L()
            rad = torch.empty((n, 4), dtype=torch.float32, device=dev)
            rec = torch.empty((n, 8), dtype=torch.int32, device=dev) if hits else None
            if n:
                torch.cuda.current_stream(dev).synchronize()
                N.check("vcrt_trace_rays_device", lib.vcrt_trace_rays_device(
                    origins.data_ptr(), dirs.data_ptr(), n, depth, rad.data_ptr(),
                    rec.data_ptr() if hits else None, ctypes.byref(st)))
        else:
            lib = self._L()
            rad = np.empty((n, 4), dtype=np.float32)
            rec = np.empty(n, dtype=RAY_HIT_DTYPE) if hits else None
            if n:
                N.check("vcrt_trace_rays", lib.vcrt_trace_rays(
                    origins.ctypes.data, dirs.ctypes.data, n, depth, rad.ctypes.data,
                    rec.ctypes.data if hits else None, ctypes.byref(st)))
        out = [rad]
        if hits:
            out.append(rec)
        if stats:
            out.append(_stats_dict(st, ("segments", "group_tests", "bound_tests", "kernel_ms"),
                                   "vcrt_trace_rays"))
        return out[0] if len(out) == 1 else tuple(out)

    def draw_features(self, samples: int | None = None, first: int = 0, albedo: bool = True,
                      normal: bool = True, sphere: bool = True, stats: bool = False,
                      device: bool = False) -> dict:
        """The guide buffers of the frame's own camera rays for a denoiser (vcrt_draw_features):
        per pixel, over the sample indices first .. first + samples - 1 (samples=None: the
        description's spp), "albedo" float32 [..., 4] (rgb the mean first-hit albedo, the sky's
        colour on a miss, a the coverage), "normal_depth" float32 [..., 4] (xyz the mean first-hit
        normal, w the mean t) and "sphere" int32 [...] (the sphere of sample index `first`, -1 the
        sky), for the planes asked for (`normal` selects normal_depth). The leading shape is the
        rank-local framebuffer's: [height, width] at world 1, else the packed tiles [tiles, 64]
        (slots outside the frame read 0).

        The arrays are numpy through the host call; with device=True they are torch tensors on
        the renderer's device, filled through the device call after the caller's current stream
        is synchronised (no host round trip). With stats=True the dict also holds "stats": rays,
        listed_rays, group_tests, bound_tests, kernel_ms, host_ms, kernel. Argument errors raise
        ValueError before any native call. The framebuffer, the accumulation and the frame
        statistics are left alone."""
        first, n = _check_sample_range(first, self.desc.samples_per_pixel if samples is None
                                       else samples)
        if not (albedo or normal or sphere):
            raise ValueError("at least one of albedo, normal, sphere")
        lib = self._L()
        st = N.vcrt_feature_stats()
        planes = self._frame_planes(device, (4 if albedo else None, 4 if normal else None,
                                             0 if sphere else None))
        name = "vcrt_draw_features_device" if device else "vcrt_draw_features"
        N.check(name, getattr(lib, name)(first, n, *map(_ptr, planes), ctypes.byref(st)))
        out = {k: p for k, p in zip(("albedo", "normal_depth", "sphere"), planes)
               if p is not None}
        if stats:
            out["stats"] = _stats_dict(st, ("rays", "listed_rays", "group_tests", "bound_tests",
                                            "kernel_ms", "host_ms"))
        return out

    def draw_occlusion(self, samples: int | None = None, first: int = 0, rays: int = 8,
                       reach: float | None = None, stats: bool = False, device: bool = False):
        """The ambient visibility buffer of the frame's own camera rays (vcrt_draw_occlusion):
        float32 [..., 4] in the rank-local framebuffer's shape ([height, width, 4] at world 1, else
        the packed tiles [tiles, 64, 4], slots outside the frame 0). Over the sample indices
        first .. first + samples - 1 (samples=None: the description's spp), every sample that hits
        sends `rays` any-hit rays of reach `reach` (None: the reference's infinity, 1e5; +inf is
        allowed; <= 0.001 leaves every ray open) from the hit point along normal + unit vector
        (ambient_dirs); rgb is the share of open rays, a sky sample counting as fully open, and a
        the share of samples that hit -- draw_features' coverage. Albedo x visibility is a
        readable preview frame.

        numpy through the host call; with device=True a torch tensor on the renderer's device,
        filled through the device call after the caller's current stream is synchronised. With
        stats=True the result is (plane, stats dict): rays, hit_rays, secondary_rays, occluded,
        listed_rays, group_tests, bound_tests, kernel_ms, host_ms, kernel. Argument errors raise
        ValueError before any native call. The framebuffer, the accumulation and the frame
        statistics are left alone."""
        first, n = _check_sample_range(first, self.desc.samples_per_pixel if samples is None
                                       else samples)
        try:
            m = int(rays)
            reach = 1e5 if reach is None else float(reach)
        except (TypeError, ValueError) as e:
            raise ValueError(f"rays: an integer, reach: a float expected ({e})") from None
        if not 1 <= m <= 256:
            raise ValueError("rays must be 1 .. 256")
        if n * m > MAX_AMBIENT_RAYS:
            raise ValueError("samples * rays must not exceed 4096")
        if (first + n) * m > MAX_AMBIENT_INDEX:
            raise ValueError("(first + samples) * rays must not exceed 2^22")
        if reach != reach:
            raise ValueError("reach must not be NaN")
        lib = self._L()
        st = N.vcrt_occlusion_buffer_stats()
        out, = self._frame_planes(device, (4,))
        name = "vcrt_draw_occlusion_device" if device else "vcrt_draw_occlusion"
        N.check(name, getattr(lib, name)(first, n, m, reach, _ptr(out), ctypes.byref(st)))
        return (out, _stats_dict(st)) if stats else out

    def denoise(self, frame=None, guides=None, *, levels=None, sigma_normal=None,
                sigma_depth=None, sigma_albedo=None, sigma_colour=None, demodulate=None,
                stats: bool = False, device: bool = False):
        """The frame through the denoiser (vcrt_denoise): the edge-avoiding a-trous filter of
        vcrt.h, albedo-demodulated, steered by draw_features' planes -- on the GPU the bits
        denoise_host computes.

        frame: a plane [height, width, 4]; None takes the renderer's own framebuffer. guides: a
        dict with "albedo" and "normal_depth" as draw_features returns them (either may be
        missing or None: its terms are off); None calls draw_features(samples=spp). Both defaults
        need the whole frame on this renderer, so they work at world size 1 only: a shard puts
        its gathered frame and guide planes through assemble_tiles and passes them in. params:
        the keyword parameters (None: default_denoise_params').

        numpy planes go through the host call and give a numpy plane. torch tensors on the
        renderer's device go through the device call on their data_ptr(), after the caller's
        current stream is synchronised, and give a torch tensor: no host round trip. device=True
        makes the defaults torch tensors (the framebuffer is filtered where it lies). With
        stats=True the result is (plane, stats dict): kernel_ms, host_ms, pass_ms, passes,
        lds_passes, kernel. Shape and dtype errors raise ValueError before any native call. The
        framebuffer, the accumulation and the frame statistics are left alone."""
        lib = self._L()
        p = _denoise_params(dict(levels=levels, sigma_normal=sigma_normal, sigma_depth=sigma_depth,
                                 sigma_albedo=sigma_albedo, sigma_colour=sigma_colour,
                                 demodulate=demodulate))
        if (frame is None or guides is None) and self.desc.world_size != 1:
            raise ValueError(
                "denoise: at world size > 1 a rank holds packed tiles; gather the frame and the "
                "guide planes, rebuild them with assemble_tiles and pass frame= and guides=")
        given = [frame] + [v for v in (guides or {}).values()]
        if any(v is not None and _is_torch(v) for v in given):
            device = True
        if guides is None:
            guides = self.draw_features(sphere=False, device=device)
        own = None  # the renderer's framebuffer on the device: filtered where it lies
        if frame is None and device:
            import torch
            own, _ = self.framebuffer_device()
            frame = torch.empty((self.desc.height, self.desc.width, 4), dtype=torch.float32,
                                device=torch.device(
                                    "cuda", self.desc.device if self.desc.device >= 0
                                    else torch.cuda.current_device()))  # receives the result
        elif frame is None:
            frame = self.read_framebuffer()
        colour, albedo, nd = _check_image_planes(
            dict(colour=frame, albedo=guides.get("albedo"),
                 normal_depth=guides.get("normal_depth")),
            optional=("albedo", "normal_depth")).values()
        st = N.vcrt_denoise_stats()
        h, w = int(colour.shape[0]), int(colour.shape[1])
        if _is_torch(colour):
            import torch
            if self.desc.device >= 0 and colour.device.index != self.desc.device:
                raise ValueError(f"planes on {colour.device}, the renderer on device "
                                 f"{self.desc.device}")
            out = colour if own else torch.empty_like(colour)
            torch.cuda.current_stream(colour.device).synchronize()
            N.check("vcrt_denoise_device", lib.vcrt_denoise_device(
                own or colour.data_ptr(), None if albedo is None else albedo.data_ptr(),
                None if nd is None else nd.data_ptr(), w, h, ctypes.byref(p), out.data_ptr(),
                ctypes.byref(st)))
        else:
            out = np.empty_like(colour)
            N.check("vcrt_denoise", lib.vcrt_denoise(
                colour.ctypes.data, None if albedo is None else albedo.ctypes.data,
                None if nd is None else nd.ctypes.data, w, h, ctypes.byref(p), out.ctypes.data,
                ctypes.byref(st)))
        if stats:
            return out, {"kernel_ms": st.kernel_ms, "host_ms": st.host_ms,
                         "pass_ms": list(st.pass_ms)[:st.passes], "passes": st.passes,
                         "lds_passes": st.lds_passes, "kernel": st.kernel.decode()}
        return out

    def draw_motion(self, prev_camera=None, prev_spheres=None, device: bool = False,
                    stats: bool = False) -> dict:
        """The reprojection map of the frame's pixels (vcrt_draw_motion): {"motion", "surface"},
        float32 [..., 4] each in the rank-local framebuffer's shape ([height, width, 4] at world
        1, else the packed tiles [tiles, 64, 4], slots outside the frame 0). motion = (px, py, z',
        key): where the surface the pixel's centre ray hits lay in the previous frame -- seen by
        prev_camera (None: the current camera; a RenderDesc or a dict of the camera fields that
        differed) with the spheres at prev_spheres (None: the current values; whatever
        update_spheres accepts, of the scene's count) -- in whole-frame pixel coordinates, the
        depth it had there and the surface's key (1 the sky, s + 2 sphere s; all zeros: the point
        does not project). surface = (key, t, 0, 0) of this frame: the next frame's
        history_surface for reproject.

        numpy through the host call; with device=True torch tensors on the renderer's device,
        filled through the device call after the caller's current stream is synchronised (a torch
        prev_spheres [n, 10] is read where it lies and implies device=True). With stats=True the
        dict also holds "stats": rays, hit_rays, projected, identity, listed_rays, group_tests,
        bound_tests, kernel_ms, host_ms, kernel. The framebuffer, the accumulation and the frame
        statistics are left alone."""
        lib = self._L()
        cam = None if prev_camera is None else ctypes.byref(_camera_c(self.desc, prev_camera))
        st = N.vcrt_motion_stats()
        prev_ptr, count = None, 0
        if prev_spheres is not None and _is_torch(prev_spheres):
            import torch
            t = prev_spheres
            if t.dtype != torch.float32 or t.ndim != 2 or t.shape[1] != 10:
                raise ValueError("prev_spheres: a torch tensor must be float32 [n, 10]")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("prev_spheres: a torch tensor must be contiguous and on a CUDA "
                                 "device")
            if self.desc.device >= 0 and t.device.index != self.desc.device:
                raise ValueError(f"prev_spheres on {t.device}, the renderer on device "
                                 f"{self.desc.device}")
            device = True
            prev_ptr, count = t.data_ptr(), int(t.shape[0])
        elif prev_spheres is not None:
            arr = (builtin_scene(prev_spheres) if isinstance(prev_spheres, (str, int))
                   else prev_spheres)
            arr = np.asarray(arr)
            if arr.dtype != SPHERE_DTYPE:
                arr = np.ascontiguousarray(arr, dtype=np.float32)
                if arr.ndim != 2 or arr.shape[1] != 10:
                    raise ValueError(f"prev_spheres: shape [n, 10] expected, got {arr.shape}")
                arr = arr.view(SPHERE_DTYPE).reshape(-1)
            arr = np.ascontiguousarray(arr)
            count = len(arr)
            prev_ptr = arr.ctypes.data
            if device:  # host values: to the device
                import torch
                staged = torch.from_numpy(arr.view(np.float32).reshape(-1, 10).copy()).to(
                    self._torch_device())
                prev_ptr = staged.data_ptr()
        motion, surface = self._frame_planes(device, (4, 4))
        name = "vcrt_draw_motion_device" if device else "vcrt_draw_motion"
        N.check(name, getattr(lib, name)(cam, prev_ptr, count, _ptr(motion), _ptr(surface),
                                         ctypes.byref(st)))
        out = {"motion": motion, "surface": surface}
        if stats:
            out["stats"] = _stats_dict(st)
        return out

    def reproject(self, frame, motion, history=None, *, surface=None, alpha=None,
                  max_history=None, depth_tolerance=None, stats: bool = False):
        """Temporal accumulation (vcrt_reproject): `frame` blended with the previous output
        gathered at each pixel's previous position -- on the GPU the bits reproject_host
        computes. Returns (out, history'): history' = {"colour": out, "surface": surface,
        "length": out_length} is what the next call takes as `history`.

        frame: the new frame [height, width, 4]; motion: draw_motion's "motion" plane of this
        frame, whole ([height, width, 4]: at world size > 1 the gathered planes put through
        assemble_tiles); surface: this frame's "surface" plane, carried into history' for the
        next call (None: history' holds None there and the caller fills it in). history=None
        starts a sequence: out = frame, every length 1. params: alpha, max_history,
        depth_tolerance (None: default_reproject_params').

        numpy planes go through the host call and give numpy planes; torch tensors on the
        renderer's device go through the device call on their data_ptr(), after the caller's
        current stream is synchronised, and give torch tensors. With stats=True the result is
        (out, history', stats dict): kernel_ms, host_ms, accepted_pixels, kernel. Shape and dtype
        errors raise ValueError before any native call. The framebuffer, the accumulation and the
        frame statistics are left alone."""
        lib = self._L()
        p = _reproject_params(dict(alpha=alpha, max_history=max_history,
                                   depth_tolerance=depth_tolerance))
        st = N.vcrt_reproject_stats()
        if history is None:
            if frame is None or (not _is_torch(frame) and np.ndim(frame) != 3):
                raise ValueError("frame: a plane [height, width, 4] expected")
            if _is_torch(frame):
                import torch
                out = frame.clone()
                length = torch.ones(frame.shape[:2], dtype=torch.float32, device=frame.device)
            else:
                out = np.array(frame, dtype=np.float32)
                length = np.ones(out.shape[:2], np.float32)
            hist = {"colour": out, "surface": surface, "length": length}
            if stats:
                return out, hist, {"kernel_ms": 0.0, "host_ms": 0.0, "accepted_pixels": 0,
                                   "kernel": ""}
            return out, hist
        if not isinstance(history, dict) or set(history) < {"colour", "surface", "length"}:
            raise ValueError('history: a dict with "colour", "surface" and "length" expected')
        pl = _check_image_planes(dict(colour=frame, motion=motion,
                                      history_colour=history["colour"],
                                      history_surface=history["surface"],
                                      history_length=history["length"]),
                                 scalar=("history_length",))
        c = pl["colour"]
        h, w = int(c.shape[0]), int(c.shape[1])
        if _is_torch(c):
            import torch
            if self.desc.device >= 0 and c.device.index != self.desc.device:
                raise ValueError(f"planes on {c.device}, the renderer on device "
                                 f"{self.desc.device}")
            out = torch.empty_like(c)
            length = torch.empty((h, w), dtype=torch.float32, device=c.device)
            torch.cuda.current_stream(c.device).synchronize()
            N.check("vcrt_reproject_device", lib.vcrt_reproject_device(
                *(pl[n].data_ptr() for n in REPROJECT_PLANES), w, h, ctypes.byref(p),
                out.data_ptr(), length.data_ptr(), ctypes.byref(st)))
        else:
            out, length = np.empty_like(c), np.empty((h, w), np.float32)
            N.check("vcrt_reproject", lib.vcrt_reproject(
                *(pl[n].ctypes.data for n in REPROJECT_PLANES), w, h, ctypes.byref(p),
                out.ctypes.data, length.ctypes.data, ctypes.byref(st)))
        hist = {"colour": out, "surface": surface, "length": length}
        if stats:
            return out, hist, {"kernel_ms": st.kernel_ms, "host_ms": st.host_ms,
                               "accepted_pixels": st.accepted_pixels,
                               "kernel": st.kernel.decode()}
        return out, hist

    def _same_device(self, plane):
        if self.desc.device >= 0 and plane.device.index != self.desc.device:
            raise ValueError(f"planes on {plane.device}, the renderer on device "
                             f"{self.desc.device}")

    def draw_samples(self, counts, first: int = 0, max_count: int | None = None, sums=None,
                     mean: bool = True, stats: bool = False, *, accumulate: bool | None = None):
        """Adaptive sampling (vcrt_draw_samples): for every local pixel p, n_p = min(counts[p],
        max_count) further samples of the frame's own rays, the sample indices first .. first +
        n_p - 1, traced on the GPU and summed in vcrt.h's fixed order (quanta of four).

        counts is an integer plane in the rank-local framebuffer's leading shape ([height, width]
        at world 1, else the packed tiles [tiles, 64]): a numpy array (converted to uint16) or a
        torch uint16 / int16 tensor on the renderer's device, which goes in without a host trip
        after the caller's current stream is synchronised. max_count=None is 256, the most the
        call accepts. sums=None starts a fresh plane; a given float32 [..., 4] plane (numpy, or
        a tensor like counts) is updated in place: added to, or overwritten with
        accumulate=False. A round that adds to a plane takes a `first` past the earlier rounds'
        first + max_count. Returns a dict: "sums" (rgb the radiance sum, a the sample count),
        "mean" when asked for (rgb / a, alpha 1; zeros where a pixel has no sample yet) and, with
        stats=True, "stats": pixels, samples, items, segments, listed_rays, group_tests,
        bound_tests, scan_ms, kernel_ms, resolve_ms, host_ms, kernel. Argument errors raise
        ValueError before any native call. The framebuffer, the accumulation and the frame
        statistics are left alone."""
        max_count = SAMPLE_MAX_COUNT if max_count is None else max_count
        first, max_count = _check_sample_range(first, max_count)
        if max_count > SAMPLE_MAX_COUNT:
            raise ValueError(f"max_count must not exceed {SAMPLE_MAX_COUNT}")
        lib = self._L()
        lead = self._local_lead()
        on_device = _is_torch(counts)
        if sums is not None and _is_torch(sums) != on_device:
            raise ValueError("counts and sums must both be numpy arrays or both torch tensors")
        if accumulate is None:
            accumulate = sums is not None
        if accumulate and sums is None:
            raise ValueError("accumulate: a sums plane expected")
        st = N.vcrt_sample_stats()
        if on_device:
            import torch
            if counts.dtype not in (torch.uint16, torch.int16) or not counts.is_cuda \
                    or not counts.is_contiguous():
                raise ValueError("counts: a contiguous uint16 (or int16) CUDA tensor expected")
            self._same_device(counts)
            if tuple(counts.shape) != lead:
                raise ValueError(f"counts: shape {lead} expected, got {tuple(counts.shape)}")
            if sums is None:
                sums = torch.zeros(lead + (4,), dtype=torch.float32, device=counts.device)
            elif (sums.dtype != torch.float32 or not sums.is_cuda or not sums.is_contiguous()
                  or sums.device != counts.device or tuple(sums.shape) != lead + (4,)):
                raise ValueError(f"sums: a contiguous float32 CUDA tensor {lead + (4,)} on "
                                 "counts' device expected")
            mean_plane = (torch.zeros(lead + (4,), dtype=torch.float32, device=counts.device)
                          if mean else None)
            torch.cuda.current_stream(counts.device).synchronize()
            fn, name = lib.vcrt_draw_samples_device, "vcrt_draw_samples_device"
        else:
            try:
                c = np.asarray(counts)
                if c.dtype.kind not in "iu":
                    raise TypeError(f"dtype {c.dtype}")
                if c.size and (c.min() < 0 or c.max() > 65535):
                    raise ValueError("values outside 0 .. 65535")
                counts = np.ascontiguousarray(c, dtype=np.uint16)
            except (TypeError, ValueError) as e:
                raise ValueError(f"counts: an integer plane expected ({e})") from None
            if counts.shape != lead:
                raise ValueError(f"counts: shape {lead} expected, got {counts.shape}")
            if sums is None:
                sums = np.zeros(lead + (4,), np.float32)
            elif (not isinstance(sums, np.ndarray) or sums.dtype != np.float32
                  or not sums.flags.c_contiguous or not sums.flags.writeable
                  or sums.shape != lead + (4,)):
                raise ValueError(f"sums: a writeable C-contiguous float32 array {lead + (4,)} "
                                 "expected")
            mean_plane = np.zeros(lead + (4,), np.float32) if mean else None
            fn, name = lib.vcrt_draw_samples, "vcrt_draw_samples"
        N.check(name, fn(first, max_count, _ptr(counts), 1 if accumulate else 0, _ptr(sums),
                         _ptr(mean_plane), ctypes.byref(st)))
        out = {"sums": sums}
        if mean:
            out["mean"] = mean_plane
        if stats:
            out["stats"] = _stats_dict(st, ("pixels", "samples", "items", "segments",
                                            "listed_rays", "group_tests", "bound_tests",
                                            "scan_ms", "kernel_ms", "resolve_ms", "host_ms"))
        return out

    def sample_counts(self, variance, target: float, min_count: int = 0, max_count: int = 64,
                      stats: bool = False):
        """A count plane for draw_samples from a variance plane (vcrt_sample_counts), on the
        GPU the bits sample_counts_host computes: counts = clamp(ceil(max(variance, 0) /
        target^2), min_count, max_count) as uint16 in variance's shape. variance is a float32
        numpy array or a contiguous torch CUDA tensor (filled through the device call, no host
        trip). With stats=True the result is (counts, stats dict): total (the sum of the
        counts), kernel_ms, host_ms, kernel."""
        lib = self._L()
        p = _sample_count_params(target, min_count, max_count)
        st = N.vcrt_sample_count_stats()
        if _is_torch(variance):
            import torch
            if variance.dtype != torch.float32 or not variance.is_cuda \
                    or not variance.is_contiguous():
                raise ValueError("variance: a contiguous float32 CUDA tensor expected")
            self._same_device(variance)
            _check_count_elements(variance.numel())
            out = torch.empty(tuple(variance.shape), dtype=torch.uint16, device=variance.device)
            torch.cuda.current_stream(variance.device).synchronize()
            fn, name, n = lib.vcrt_sample_counts_device, "vcrt_sample_counts_device", \
                variance.numel()
        else:
            variance = _variance_plane(variance)
            out = np.empty(variance.shape, np.uint16)
            fn, name, n = lib.vcrt_sample_counts, "vcrt_sample_counts", variance.size
        N.check(name, fn(_ptr(variance), n, ctypes.byref(p), _ptr(out), ctypes.byref(st)))
        if stats:
            return out, {"total": st.total, "kernel_ms": st.kernel_ms, "host_ms": st.host_ms,
                         "kernel": st.kernel.decode()}
        return out

    def reproject_moments(self, frame, motion, history=None, *, surface=None, albedo=None,
                          alpha=None, max_history=None, depth_tolerance=None,
                          alpha_moments=None, stats: bool = False):
        """Temporal accumulation that carries the luminance moments along
        (vcrt_reproject_moments): reproject's out and length, bit for bit, and the first and
        second moments of the demodulated luminance -- on the GPU the bits
        reproject_moments_host computes. Returns (out, history'): history' = {"colour": out,
        "surface": surface, "length": out_length, "moments": out_moments} is what the next call
        takes as `history` and what variance() reads.

        frame, motion, surface as for reproject; albedo: draw_features' plane of this frame
        (None: the moments are the colour's luminance). history=None starts a sequence: the call
        runs on history planes of zeros. params: alpha, max_history, depth_tolerance,
        alpha_moments (None: default_reproject_moments_params').

        numpy planes go through the host call, torch tensors on the renderer's device through
        the device call, as reproject's. With stats=True the result is (out, history', stats
        dict). Shape and dtype errors raise ValueError before any native call."""
        lib = self._L()
        p = _reproject_moments_params(dict(alpha=alpha, max_history=max_history,
                                           depth_tolerance=depth_tolerance,
                                           alpha_moments=alpha_moments))
        st = N.vcrt_reproject_stats()
        if history is None:
            if frame is None or (not _is_torch(frame) and np.ndim(frame) != 3):
                raise ValueError("frame: a plane [height, width, 4] expected")
            if _is_torch(frame):
                import torch
                zeros4 = torch.zeros_like(frame)
                zeros1 = torch.zeros(frame.shape[:2], dtype=frame.dtype, device=frame.device)
            else:
                zeros4 = np.zeros(np.shape(frame), np.float32)
                zeros1 = np.zeros(np.shape(frame)[:2], np.float32)
            history = {"colour": zeros4, "surface": zeros4, "length": zeros1, "moments": zeros4}
        if (not isinstance(history, dict)
                or not set(history) >= {"colour", "surface", "length", "moments"}):
            raise ValueError('history: a dict with "colour", "surface", "length" and "moments" '
                             'expected')
        pl = _check_image_planes(dict(colour=frame, motion=motion,
                                      history_colour=history["colour"],
                                      history_surface=history["surface"],
                                      history_length=history["length"], albedo=albedo,
                                      history_moments=history["moments"]),
                                 scalar=("history_length",), optional=("albedo",))
        c = pl["colour"]
        h, w = int(c.shape[0]), int(c.shape[1])
        if _is_torch(c):
            import torch
            self._same_device(c)
            out, moments = torch.empty_like(c), torch.empty_like(c)
            length = torch.empty((h, w), dtype=torch.float32, device=c.device)
            torch.cuda.current_stream(c.device).synchronize()
            fn, name = lib.vcrt_reproject_moments_device, "vcrt_reproject_moments_device"
        else:
            out, moments = np.empty_like(c), np.empty_like(c)
            length = np.empty((h, w), np.float32)
            fn, name = lib.vcrt_reproject_moments, "vcrt_reproject_moments"
        N.check(name, fn(*(_ptr(pl[n]) for n in MOMENTS_PLANES), w, h, ctypes.byref(p),
                         _ptr(out), _ptr(length), _ptr(moments), ctypes.byref(st)))
        hist = {"colour": out, "surface": surface, "length": length, "moments": moments}
        if stats:
            return out, hist, {"kernel_ms": st.kernel_ms, "host_ms": st.host_ms,
                               "accepted_pixels": st.accepted_pixels,
                               "kernel": st.kernel.decode()}
        return out, hist

    def variance(self, history, *, min_history=None, alpha=None, stats: bool = False):
        """The per-pixel variance of the accumulated, demodulated luminance (vcrt_variance) from
        reproject_moments' history' (its "moments" and "surface" planes): float32
        [height, width] -- temporal where the history is min_history long, else the 7 x 7
        spatial estimate over the pixel's surface; on the GPU the bits variance_host computes.
        params: min_history, alpha -- the alpha the sequence's reproject_moments runs with (None:
        default_variance_params'). numpy or torch planes, as reproject's. With stats=True the
        result is (variance, stats dict): kernel_ms, host_ms, spatial_pixels, kernel."""
        lib = self._L()
        p = _variance_params(dict(min_history=min_history, alpha=alpha))
        if not isinstance(history, dict) or not set(history) >= {"moments", "surface"}:
            raise ValueError('history: a dict with "moments" and "surface" expected')
        pl = _check_image_planes(dict(moments=history["moments"], surface=history["surface"]))
        m = pl["moments"]
        h, w = int(m.shape[0]), int(m.shape[1])
        st = N.vcrt_variance_stats()
        if _is_torch(m):
            import torch
            self._same_device(m)
            out = torch.empty((h, w), dtype=torch.float32, device=m.device)
            torch.cuda.current_stream(m.device).synchronize()
            fn, name = lib.vcrt_variance_device, "vcrt_variance_device"
        else:
            out = np.empty((h, w), np.float32)
            fn, name = lib.vcrt_variance, "vcrt_variance"
        N.check(name, fn(_ptr(m), _ptr(pl["surface"]), w, h, ctypes.byref(p), _ptr(out),
                         ctypes.byref(st)))
        if stats:
            return out, {"kernel_ms": st.kernel_ms, "host_ms": st.host_ms,
                         "spatial_pixels": st.spatial_pixels, "kernel": st.kernel.decode()}
        return out

    def denoise_variance(self, frame, variance, guides=None, *, levels=None, sigma_normal=None,
                         sigma_depth=None, sigma_albedo=None, sigma_colour=None, demodulate=None,
                         stats: bool = False):
        """The frame through the variance-steered denoiser (vcrt_denoise_variance): denoise's
        filter with the colour threshold set per pixel by `variance` (variance()'s plane), which
        is filtered along -- on the GPU the bits denoise_variance_host computes. Returns
        (out [height, width, 4], out_variance [height, width]).

        frame: a plane [height, width, 4]; guides: a dict with "albedo" and "normal_depth" as
        draw_features returns them (either may be missing or None: its terms are off; None: no
        guides). params: denoise's keyword parameters (None:
        default_denoise_variance_params'). numpy or torch planes, as denoise's. With stats=True
        the result is (out, out_variance, stats dict) with denoise's fields."""
        lib = self._L()
        p = _denoise_variance_params(dict(levels=levels, sigma_normal=sigma_normal,
                                          sigma_depth=sigma_depth, sigma_albedo=sigma_albedo,
                                          sigma_colour=sigma_colour, demodulate=demodulate))
        guides = guides or {}
        pl = _check_image_planes(dict(colour=frame, albedo=guides.get("albedo"),
                                      normal_depth=guides.get("normal_depth"),
                                      variance=variance), scalar=("variance",),
                                 optional=("albedo", "normal_depth"))
        c = pl["colour"]
        h, w = int(c.shape[0]), int(c.shape[1])
        st = N.vcrt_denoise_stats()
        if _is_torch(c):
            import torch
            self._same_device(c)
            out = torch.empty_like(c)
            out_var = torch.empty((h, w), dtype=torch.float32, device=c.device)
            torch.cuda.current_stream(c.device).synchronize()
            fn, name = lib.vcrt_denoise_variance_device, "vcrt_denoise_variance_device"
        else:
            out, out_var = np.empty_like(c), np.empty((h, w), np.float32)
            fn, name = lib.vcrt_denoise_variance, "vcrt_denoise_variance"
        N.check(name, fn(_ptr(c), _ptr(pl["albedo"]), _ptr(pl["normal_depth"]),
                         _ptr(pl["variance"]), w, h, ctypes.byref(p), _ptr(out), _ptr(out_var),
                         ctypes.byref(st)))
        if stats:
            return out, out_var, {"kernel_ms": st.kernel_ms, "host_ms": st.host_ms,
                                  "pass_ms": list(st.pass_ms)[:st.passes], "passes": st.passes,
                                  "lds_passes": st.lds_passes, "kernel": st.kernel.decode()}
        return out, out_var

    def occluded(self, origins, dirs, tmax=None, stats: bool = False):
        """Is anything in the way within each ray's reach (vcrt_occlude_rays)? Shadow rays,
        ambient occlusion, line of sight, probe visibility.

        origins, dirs as for trace_rays (dirs are not normalised; t is in units of dirs). tmax is
        the reach T: None (the reference's infinity, 1e5: the answer is then "trace_rays finds a
        first hit"), a scalar for every ray, or float32 [n]; with torch rays a tensor tmax must be
        float32, contiguous and on the rays' device. A ray is occluded when hit_sphere with
        min_t = 0.001 and max_t = T accepts some sphere of the scene; T <= 0.001 never is, +inf
        is allowed.

        numpy inputs go through the host call and return a numpy bool_ [n]; torch tensors go
        through the device call on their data_ptr(), after the caller's current stream is
        synchronised, and return a torch bool [n] on the rays' device. With stats=True the result
        is (occluded, stats dict). Shape and dtype errors raise ValueError before any native
        call. The framebuffer and the frame statistics are left alone."""
        origins, dirs = _check_rays(origins, dirs)
        n = int(origins.shape[0])
        tmax = _check_reach(tmax, n, origins)
        st = N.vcrt_ray_stats()
        if _is_torch(origins):
            import torch
            dev = origins.device
            if self.desc.device >= 0 and dev.index != self.desc.device:
                raise ValueError(f"rays on {dev}, the renderer on device {self.desc.device}")
            lib = self._L()
            occ = torch.empty((n,), dtype=torch.uint8, device=dev)
            if n:
                torch.cuda.current_stream(dev).synchronize()
                N.check("vcrt_occlude_rays_device", lib.vcrt_occlude_rays_device(
                    origins.data_ptr(), dirs.data_ptr(),
                    None if tmax is None else tmax.data_ptr(), n, occ.data_ptr(),
                    ctypes.byref(st)))
            occ = occ.view(torch.bool)
        else:
            lib = self._L()
            occ = np.empty(n, dtype=np.uint8)
            if n:
                N.check("vcrt_occlude_rays", lib.vcrt_occlude_rays(
                    origins.ctypes.data, dirs.ctypes.data,
                    None if tmax is None else tmax.ctypes.data, n, occ.ctypes.data,
                    ctypes.byref(st)))
            occ = occ.view(np.bool_)
        if stats:
            return occ, _stats_dict(st, ("segments", "group_tests", "bound_tests", "kernel_ms"),
                                    "vcrt_occlude_rays")
        return occ

    def visible(self, a, b):
        """Line of sight between the points a[i] and b[i] ([n, 3], numpy or torch as for
        occluded): ~occluded(a, b - a, tmax=1.0), the subtraction in fp32.

        min_t = 0.001 is in units of b - a: a segment ignores occluders in its first thousandth,
        whatever its length, and an endpoint exactly on a surface may land on either side of
        T = 1, so a point on a sphere may or may not see itself blocked by that sphere."""
        a, b = _check_rays(a, b)
        return ~self.occluded(a, b - a, tmax=1.0)

    def shader_load(self, path: str) -> None:
        N.check("vcrt_shader_load", self._L().vcrt_shader_load(path.encode()))

    def frame_times(self) -> tuple:
        """(kernel_ms, segments, gather_ms, frame_ms) of the last frame: vcrt_get_stats into a
        reused struct, without building stats()'s dict (a timed loop's per-frame bookkeeping)."""
        s = self._frame_stats
        N.check("vcrt_get_stats", self._L().vcrt_get_stats(ctypes.byref(s)))
        return s.kernel_ms, s.segments, s.gather_ms, s.frame_ms

    def stats(self) -> dict:
        s = N.vcrt_stats()
        N.check("vcrt_get_stats", self._L().vcrt_get_stats(ctypes.byref(s)))
        out = {name: getattr(s, name) for name, _ in N.vcrt_stats._fields_}
        out["debug"] = list(s.debug)
        out["kernel"] = s.kernel.decode()
        return out


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id (vcrt_comm_unique_id) for rank 0 to hand to every rank."""
    cid = N.vcrt_comm_id()
    N.check("vcrt_comm_unique_id", N.lib().vcrt_comm_unique_id(ctypes.byref(cid)))
    return ctypes.string_at(ctypes.addressof(cid), ctypes.sizeof(cid))


def render(desc: RenderDesc, scene="final", frames: int = 1) -> tuple[np.ndarray, dict]:
    """Convenience: Begin, draw `frames` frames, read the rank-local framebuffer, End."""
    with Renderer(desc, scene) as r:
        for _ in range(frames):
            r.draw_next_frame()
        return r.read_framebuffer(), r.stats()
