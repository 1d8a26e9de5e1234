"""The thin lens restated for the tests (no tests here): the camera basis, the per-sample lens
offsets, the ray of (x, y, i) and the accumulation rule in numpy float32, every operation rounded
on its own -- what -ffp-contract=off C does. rand and sin are the CPU oracle's (oracle.rand /
oracle.sin: implementations of their own, not libvcrt's); a frame's reference is the
accumulation of oracle.ray_color over these rays.

Definitions (include/vcrt.h lens_radius, vcrt_lens_offsets), fi = (float)i:
    a   = rand(fi, fi + 0.5f)            b   = rand(fi + 0.5f, fi)
    rho = R * sqrtf(a)                   phi = 6.2831855f * b
    lx  = rho * sin(phi + 1.5707964f)    ly  = rho * sin(phi)
    offset_i = lx * camera_u + ly * camera_v
    origin_i = center + offset_i
    dir      = (corner(x, y) + jitter_i) - origin_i
"""
import ctypes

import numpy as np

F = np.float32
TWO_PI = np.array([0x40C90FDB], np.uint32).view(np.float32)[0]
HALF_PI = np.array([0x3FC90FDB], np.uint32).view(np.float32)[0]
MAX_QUANTA = 512          # quanta per pixel (vcrt.h accumulate_quantum)
Q_LIMIT = 2.0 ** 44       # |quantized quantum sum| bound (csrc/vcrt_math.h "Accumulation")

_cache = {}


def _v(a):
    return np.asarray(a, dtype=F)


def _dot(a, b):  # GLSL dot: (x x' + y y') + z z'
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def _normalize(a):
    return _v(a / np.sqrt(_dot(a, a)))


def _cross(a, b):  # GLSL cross
    return _v([F(a[1] * b[2]) - F(b[1] * a[2]), F(a[2] * b[0]) - F(b[2] * a[0]),
               F(a[0] * b[1]) - F(b[0] * a[1])])


def camera_basis(lookfrom, lookat, vup):
    """(camera_u, camera_v): shader.comp:28-29's unit basis, in make_camera's operation order."""
    w = _normalize(_v(lookfrom) - _v(lookat))
    u = _normalize(_cross(_v(vup), w))
    v = _cross(w, u)
    return u, v


def camera_of(oracle, desc):
    """dict of the oracle's camera for a RenderDesc (pixel00, delta_u, delta_v, center, the
    viewport's size) plus the basis, pinned: (viewport_width * u) / H and (viewport_height * -v)
    / H must reproduce the oracle's delta_u and delta_v bit for bit."""
    cfg = oracle.config(desc.width, desc.height, desc.samples_per_pixel, desc.max_depth,
                        desc.lookfrom, desc.lookat, desc.vup, desc.vfov)
    c = oracle.camera(cfg)
    u, v = camera_basis(desc.lookfrom, desc.lookat, desc.vup)
    cam = dict(p00=c[0:3].copy(), du=c[3:6].copy(), dv=c[6:9].copy(), center=c[9:12].copy(),
               vh=c[13], vw=c[14], u=u, v=v)
    h = F(desc.height)
    with np.errstate(all="ignore"):
        du = _v(_v(cam["vw"] * u) / h)
        dv = _v(_v(cam["vh"] * _v(-v)) / h)
    assert np.array_equal(du.view(np.uint32), cam["du"].view(np.uint32)), "basis pin: delta_u"
    assert np.array_equal(dv.view(np.uint32), cam["dv"].view(np.uint32)), "basis pin: delta_v"
    return cam


def lens_xy(oracle, i, radius):
    """(lx, ly) of sample index i for radius R (float32 scalars)."""
    fi = F(i)
    fh = F(fi + F(0.5))
    a = F(oracle.rand(float(fi), float(fh)))
    b = F(oracle.rand(float(fh), float(fi)))
    rho = F(F(radius) * np.sqrt(a))
    phi = F(TWO_PI * b)
    lx = F(rho * F(oracle.sin(float(F(phi + HALF_PI)))))
    ly = F(rho * F(oracle.sin(float(phi))))
    return lx, ly


def lens_offsets(oracle, u, v, radius, first, count):
    """offset_i for i = first .. first + count - 1: float32 [count, 3]; all +0 for R == 0."""
    out = np.zeros((count, 3), F)
    if not radius > 0:
        return out
    for k in range(count):
        lx, ly = lens_xy(oracle, first + k, radius)
        out[k] = _v(lx * u) + _v(ly * v)
    return out


def jitter_terms(oracle, cam, first, count):
    """jx delta_u + jy delta_v of sample indices first .. (shader.comp:48): float32 [count, 3]."""
    out = np.zeros((count, 3), F)
    for k in range(count):
        i = first + k
        jx = F(F(-0.5) + F(oracle.rand(float(F(i)), float(F(i)))))
        jy = F(F(-0.5) + F(oracle.rand(float(F(i + 1)), float(F(i + 1)))))
        out[k] = _v(jx * cam["du"]) + _v(jy * cam["dv"])
    return out


def frame_rays(oracle, desc, first=0, count=None):
    """The rays of every pixel and sample index first .. first + count - 1 of a lens frame:
    (origins [count, 3], dirs [H, W, count, 3]) float32 (an origin depends on the index only)."""
    count = desc.samples_per_pixel if count is None else count
    cam = camera_of(oracle, desc)
    off = lens_offsets(oracle, cam["u"], cam["v"], desc.lens_radius, first, count)
    origins = _v(cam["center"][None, :] + off)
    jit = jitter_terms(oracle, cam, first, count)
    y, x = np.mgrid[0:desc.height, 0:desc.width]
    fx, fy = x.astype(F)[..., None], y.astype(F)[..., None]
    corner = _v(_v(cam["p00"] + _v(fx * cam["du"])) + _v(fy * cam["dv"]))      # [H, W, 3]
    point = _v(corner[:, :, None, :] + jit[None, None, :, :])                  # [H, W, n, 3]
    dirs = _v(point - origins[None, None, :, :])
    return origins, dirs


def rule_quantum(spp):
    """vcrt.h accumulate_quantum = 0: 4, doubled while a frame's pixel would take more than 512
    quanta."""
    g = 4
    while (spp + g - 1) // g > MAX_QUANTA:
        g *= 2
    return g


def accumulate(oracle, radiance, quantum, frame_spp=None, direct=False):
    """The accumulation rule (csrc/vcrt_math.h "Accumulation") for one pixel's samples
    radiance [n, 3] in sample order -> float32 [4]. Quanta of `quantum` consecutive samples,
    restarting every frame_spp samples (progressive frames); direct: one quantum covers the
    pixel of a non-progressive frame -- the fp32 sum divided by n."""
    rad = _v(radiance)
    n = len(rad)
    frame_spp = n if frame_spp is None else frame_spp
    with np.errstate(all="ignore"):
        if direct:
            acc = np.zeros(3, F)
            for s in rad:
                acc = _v(acc + s)
            return np.append(_v(acc / F(n)), F(1.0))
        sums = []
        for f0 in range(0, n, frame_spp):
            for q0 in range(f0, min(f0 + frame_spp, n), quantum):
                acc = np.zeros(3, F)
                for s in rad[q0:min(q0 + quantum, f0 + frame_spp, n)]:
                    acc = _v(acc + s)
                sums.append(acc)
        sums = np.array(sums, F)
        if not np.isfinite(sums).all():
            return np.array([np.nan, np.nan, np.nan, 1.0], F)
        e = F(np.abs(sums).max())
        s_log2 = 32 if e < F(2.0 ** 12) else oracle.pixel_scale_log2(float(e))
        scaled = _v(sums * F(2.0 ** s_log2))  # exact (a power of two), fp32
        assert np.all(np.abs(scaled) < Q_LIMIT)
        total = np.rint(scaled).astype(np.float64).sum(axis=0)  # exact: integers below 2^53
        out = ((total * 2.0 ** -s_log2) / np.float64(n)).astype(F)
    return np.append(out, F(1.0))


def trace(oracle, scene, origins, dirs, depth):
    """oracle.ray_color of rays (origins [n, 3] broadcast over dirs [..., n, 3]):
    (rgb [..., n, 3] float32, segments [..., n] uint64)."""
    from tests.oracle_py import SPHERE_DTYPE
    scene = np.ascontiguousarray(scene, dtype=SPHERE_DTYPE)
    D = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    O = np.ascontiguousarray(np.broadcast_to(origins, dirs.shape), F).reshape(-1, 3)
    rgb = np.zeros((len(D), 3), F)
    segs = np.zeros(len(D), np.uint64)
    seg_t = ctypes.POINTER(ctypes.c_uint64)
    f = oracle.lib.oracle_ray_color
    sp, ns = scene.ctypes.data, len(scene)
    po, pd, pc, ps = O.ctypes.data, D.ctypes.data, rgb.ctypes.data, segs.ctypes.data
    for i in range(len(D)):
        f(sp, ns, po + 12 * i, pd + 12 * i, depth, pc + 12 * i, ctypes.cast(ps + 8 * i, seg_t))
    return rgb.reshape(dirs.shape), segs.reshape(dirs.shape[:-1])


def accumulate_frame(oracle, rgb, quantum, frame_spp=None, direct=False):
    """accumulate() over every pixel of rgb [H, W, n, 3] -> float32 [H, W, 4]."""
    h, w = rgb.shape[:2]
    out = np.zeros((h, w, 4), F)
    for y in range(h):
        for x in range(w):
            out[y, x] = accumulate(oracle, rgb[y, x], quantum, frame_spp, direct)
    return out


def reference_frame(oracle, scene, desc, frames=1):
    """(image float32 [H, W, 4], segments of the last frame) of a lens frame for a RenderDesc:
    oracle.ray_color over frame_rays, accumulated by the rule. Progressive descs: the image
    after `frames` frames. Cached by its arguments' values (the scene by identity)."""
    key = (id(scene), desc.width, desc.height, desc.samples_per_pixel, desc.max_depth,
           tuple(desc.lookfrom), tuple(desc.lookat), tuple(desc.vup), desc.vfov,
           desc.accumulate_quantum, desc.progressive, float(desc.lens_radius), frames)
    if key in _cache:
        return _cache[key][:2]
    spp = desc.samples_per_pixel
    total = spp * frames if desc.progressive else spp
    origins, dirs = frame_rays(oracle, desc, 0, total)
    rgb, segs = trace(oracle, scene, origins, dirs, desc.max_depth)
    last_segs = int(segs[:, :, total - spp:].sum())
    g = desc.accumulate_quantum or rule_quantum(spp)
    direct = g >= spp and not desc.progressive
    img = accumulate_frame(oracle, rgb, g, spp, direct)
    img.setflags(write=False)
    _cache[key] = (img, last_segs, scene)  # (the scene kept alive: its id is the key)
    return img, last_segs
