"""The ambient visibility buffer restated for the tests (no tests here): include/vcrt.h
vcrt_draw_occlusion in numpy float32, every operation rounded on its own, built from parts that
exist -- the frame's rays from tests/lens_ref.frame_rays, first hits from
tests/ray_query_ref.first_hit, the any-hit predicate from tests/occlusion_ref.occluded_ref, rand
and sin from the CPU oracle (implementations of their own, not libvcrt's), the packed tiles of a
shard through tests/features_ref.packed.

Definitions, fj = (float)j, j = i * m + k for sample index i and secondary ray k < m:
    a  = rand(fj, fj + 0.5f)             b   = rand(fj + 0.5f, fj)
    zc = 1 - 2 a                         rr  = sqrtf(max(0, 1 - zc zc))
    phi = 6.2831855f * b                 u_j = (rr sin(phi + 1.5707964f), rr sin(phi), zc)
    P  = o + t d                         N   = dot(d, normal) > 0 ? -normal : normal
    d' = N + u_j                         open = !occluded(P, d', reach)
    rgb = (float)(U + m (n - C)) / (float)(n m)          a = (float)C / (float)n
"""
import numpy as np

from tests import lens_ref as L
from tests import occlusion_ref as OC
from tests import ray_query_ref as R
from tests.features_ref import packed  # noqa: F401  (the shard's layout, for the tests)

F = np.float32

_cache = {}


def ambient_dirs(oracle, first, count):
    """u_j of j = first .. first + count - 1: float32 [count, 3]."""
    out = np.zeros((count, 3), F)
    for k in range(count):
        fj = F(first + k)
        fh = F(fj + F(0.5))
        a = F(oracle.rand(float(fj), float(fh)))
        b = F(oracle.rand(float(fh), float(fj)))
        zc = F(F(1.0) - F(F(2.0) * a))
        rr = F(np.sqrt(np.maximum(F(0.0), F(F(1.0) - F(zc * zc)))))
        phi = F(L.TWO_PI * b)
        out[k] = (F(rr * F(oracle.sin(float(F(phi + L.HALF_PI))))),
                  F(rr * F(oracle.sin(float(phi)))), zc)
    return out


def secondary_rays(oracle, O, D, t, normal, first, n, m):
    """(P [rays, 3], d' [rays, m, 3]) float32 of the rays O, D [pixels * n, 3] (sample-minor) with
    first hits (t, normal); the rows of samples that missed are filled like any other and are to
    be masked by the caller."""
    with np.errstate(all="ignore"):
        P = (O + (t[:, None] * D).astype(F)).astype(F)
        dn = ((D[:, 0] * normal[:, 0] + D[:, 1] * normal[:, 1]).astype(F)
              + D[:, 2] * normal[:, 2]).astype(F)
        N = np.where((dn > 0)[:, None], -normal, normal).astype(F)
        u = ambient_dirs(oracle, first * m, n * m).reshape(n, m, 3)
        sample = np.arange(len(O)) % n
        d2 = (N[:, None, :] + u[sample]).astype(F)
    return P, d2


def frame_occlusion(oracle, scene, desc, first, n, m, reach):
    """The whole frame's plane for a RenderDesc (its camera and lens_radius): dict of visibility
    [H, W, 4] float32, the counts hit_rays, secondary_rays, occluded, the per-pixel integer
    counts C and blocked [H, W], and min_d2 (the smallest |d'|^2 over the hit samples). Cached by
    the arguments' values (the scene by identity), read-only."""
    key = (id(scene), desc.width, desc.height, tuple(desc.lookfrom), tuple(desc.lookat),
           tuple(desc.vup), desc.vfov, float(desc.lens_radius), first, n, m, float(reach))
    if key in _cache:
        return _cache[key][0]
    h, w = desc.height, desc.width
    origins, dirs = L.frame_rays(oracle, desc, first, n)          # [n, 3], [H, W, n, 3]
    D = np.ascontiguousarray(dirs.reshape(-1, 3))
    O = np.ascontiguousarray(np.broadcast_to(origins, dirs.shape).reshape(-1, 3))
    t, sphere, normal = R.first_hit(scene, O, D)
    hit = sphere >= 0
    P, d2 = secondary_rays(oracle, O, D, t, normal, first, n, m)
    Ph = np.repeat(P[hit], m, axis=0)
    Dh = np.ascontiguousarray(d2[hit].reshape(-1, 3))
    occ, _, _ = OC.occluded_ref(scene, Ph, Dh, np.full(len(Ph), reach, F))
    blocked_ray = np.zeros(len(O), np.int64)
    blocked_ray[hit] = occ.reshape(-1, m).sum(axis=1)
    pix = h * w
    C = hit.reshape(pix, n).sum(axis=1)
    blocked = blocked_ray.reshape(pix, n).sum(axis=1)
    with np.errstate(all="ignore"):
        v = ((n * m - blocked).astype(F) / F(n * m)).astype(F)    # U + m (n - C) = n m - blocked
        a = (C.astype(F) / F(n)).astype(F)
        len2 = ((Dh[:, 0] * Dh[:, 0] + Dh[:, 1] * Dh[:, 1]).astype(F) + Dh[:, 2] * Dh[:, 2])
    out = dict(visibility=np.stack([v, v, v, a], axis=1).reshape(h, w, 4),
               hit_rays=int(hit.sum()), secondary_rays=int(hit.sum()) * m,
               occluded=int(occ.sum()), C=C.reshape(h, w), blocked=blocked.reshape(h, w),
               min_d2=float(len2.min()) if len(len2) else float("inf"))
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    _cache[key] = (out, scene)  # (the scene kept alive: its id is the key)
    return out
