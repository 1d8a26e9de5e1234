"""The reprojection map restated for the tests (no tests here): include/vcrt.h vcrt_draw_motion in
numpy float32, built from parts that exist -- the camera from the oracle (tests/lens_ref.camera_of),
the centre rays' first hits from tests/ray_query_ref.first_hit -- and the projection through the
previous camera, one rounded operation per statement."""
import numpy as np

from tests import lens_ref as L
from tests import ray_query_ref as R

F = np.float32
FLT_MAX = np.finfo(np.float32).max

_cache = {}


def _dot(a, b):
    """GLSL dot over the last axis: (x x' + y y') + z z', each operation rounded."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def _cross(a, b):
    return np.asarray([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0],
                       a[0] * b[1] - b[0] * a[1]], F)


def motion_camera(oracle, desc):
    """C', e, nw, nu, nv, num of desc's camera."""
    cam = L.camera_of(oracle, desc)
    c, du, dv = cam["center"].astype(F), cam["du"].astype(F), cam["dv"].astype(F)
    with np.errstate(all="ignore"):
        e = (cam["p00"].astype(F) - c).astype(F)
        nw = _cross(du, dv)
        nu = (du / _dot(du, du)).astype(F)
        nv = (dv / _dot(dv, dv)).astype(F)
        return dict(c=c, e=e, nw=nw, nu=nu, nv=nv, num=_dot(e, nw))


def project(mc, Q):
    """(ok [n] bool, (px, py, z') [n, 3] float32, NaN where not ok) of world points Q [n, 3]."""
    Q = np.asarray(Q, F)
    with np.errstate(all="ignore"):
        q = (Q - mc["c"][None, :]).astype(F)
        den = _dot(q, mc["nw"][None, :])
        lam = (mc["num"] / den).astype(F)
        ok = (lam > 0) & (lam <= FLT_MAX)
        h = ((lam[:, None] * q).astype(F) - mc["e"][None, :]).astype(F)
        out = np.stack([_dot(h, mc["nu"][None, :]), _dot(h, mc["nv"][None, :]),
                        (den / mc["num"]).astype(F)], axis=1).astype(F)
    out[~ok] = np.nan
    return ok, out


def centre_rays(oracle, desc):
    """(origin [3], dirs [H, W, 3]) of the pixels' centre rays: corner - centre."""
    cam = L.camera_of(oracle, desc)
    y, x = np.mgrid[0:desc.height, 0:desc.width]
    fx, fy = x.astype(F)[..., None], y.astype(F)[..., None]
    corner = ((cam["p00"] + (fx * cam["du"]).astype(F)).astype(F) +
              (fy * cam["dv"]).astype(F)).astype(F)
    return cam["center"].astype(F), (corner - cam["center"][None, None, :]).astype(F)


def first_hits(oracle, scene, desc):
    """(t, sphere, normal) of the centre rays, cached by the camera and the scene's identity."""
    key = (id(scene), desc.width, desc.height, tuple(desc.lookfrom), tuple(desc.lookat),
           tuple(desc.vup), desc.vfov)
    if key not in _cache:
        o, d = centre_rays(oracle, desc)
        D = np.ascontiguousarray(d.reshape(-1, 3))
        O = np.ascontiguousarray(np.broadcast_to(o, D.shape))
        _cache[key] = (R.first_hit(scene, O, D), scene)
    return _cache[key][0]


def frame_motion(oracle, scene, desc, prev_desc=None, prev_scene=None):
    """The whole frame's planes: dict of motion [H, W, 4], surface [H, W, 4] float32 and the
    counts hit, projected, identity. prev_desc None: the same camera; prev_scene None: the current
    values."""
    h, w = desc.height, desc.width
    t, s, normal = first_hits(oracle, scene, desc)
    _, d = centre_rays(oracle, desc)
    d = d.reshape(-1, 3)
    hit = s >= 0
    same_cam = prev_desc is None or all(
        np.array_equal(np.asarray(getattr(prev_desc, k), F).view(np.uint32),
                       np.asarray(getattr(desc, k), F).view(np.uint32))
        for k in ("lookfrom", "lookat", "vup", "vfov"))
    mc = motion_camera(oracle, desc if prev_desc is None else prev_desc)
    cur_c = np.asarray(scene["center"], F)
    cur_r = np.asarray(scene["radius"], F)
    prev = scene if prev_scene is None else prev_scene
    assert len(prev) == len(scene)
    pc, pr = np.asarray(prev["center"], F), np.asarray(prev["radius"], F)
    idx = np.where(hit, s, 0)
    with np.errstate(all="ignore"):
        Q = np.where(hit[:, None],
                     (pc[idx] + (pr[idx][:, None] * normal).astype(F)).astype(F),
                     (mc["c"][None, :] + d).astype(F)).astype(F)
    ok, proj = project(mc, Q)
    key0 = (s + 2).astype(F)
    unmoved = ((pc[idx].view(np.uint32) == cur_c[idx].view(np.uint32)).all(axis=1) &
               (pr[idx].view(np.uint32) == cur_r[idx].view(np.uint32)))
    ident = same_cam & (~hit | unmoved)
    motion = np.zeros((h * w, 4), F)
    motion[ok, :3] = proj[ok]
    motion[ok, 3] = key0[ok]
    y, x = np.mgrid[0:h, 0:w]
    idm = np.stack([x.reshape(-1).astype(F), y.reshape(-1).astype(F),
                    np.where(hit, t, F(1.0)).astype(F), key0], axis=1)
    motion[ident] = idm[ident]
    surface = np.zeros((h * w, 4), F)
    surface[:, 0] = key0
    surface[:, 1] = np.where(hit, t, F(0.0))
    return dict(motion=motion.reshape(h, w, 4), surface=surface.reshape(h, w, 4),
                hit=int(hit.sum()), projected=int((ok | ident).sum()), identity=int(ident.sum()),
                sphere=s.reshape(h, w))
