"""Shared references of the occlusion-query tests (no tests here).

* occluded_ref(): the contract of vcrt_occlude_rays restated in numpy float32, every operation
  rounded on its own -- hit_sphere (functions.glsl:14-40) with min_t = 0.001 and a fixed max_t = T
  per ray, ORed over the spheres.
* reach(): the per-ray tmax of the parity tests, built from each ray's own first hit so that the
  far limit falls on, one ulp above and one ulp below an accepted root.
* reference(): both on the batch of tests/ray_query_ref.py, computed once per scene.
"""
import numpy as np

from tests import ray_query_ref as R

MIN_T = R.MIN_T
_cache = {}


def occluded_ref(scene, O, D, T):
    """(occluded [n] bool, accepting [n] int32: the spheres that accept, far_first [n] bool: the
    first accepting sphere in index order accepted through its far root)."""
    O = np.asarray(O, np.float32)
    D = np.asarray(D, np.float32)
    T = np.asarray(T, np.float32)
    n = len(O)
    ox, oy, oz = O[:, 0], O[:, 1], O[:, 2]
    dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]
    accepting = np.zeros(n, np.int32)
    far_first = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        a = (dx * dx + dy * dy) + dz * dz
        for s in scene:
            cx, cy, cz = (np.float32(v) for v in s["center"])
            r = np.float32(s["radius"])
            ocx, ocy, ocz = ox - cx, oy - cy, oz - cz
            hb = (ocx * dx + ocy * dy) + ocz * dz
            cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - r * r
            disc = hb * hb - a * cc
            cand = ~(disc < 0)
            if not cand.any():
                continue
            sq = np.sqrt(disc)
            root = (-hb - sq) / a
            far = cand & ((root <= MIN_T) | (T <= root))
            root2 = (-hb + sq) / a
            yes = cand & ~(far & ((root2 <= MIN_T) | (T <= root2)))
            far_first = np.where(yes & (accepting == 0), far, far_first)
            accepting = accepting + yes.astype(np.int32)
    return accepting > 0, accepting, far_first


def reach(oracle, scene):
    """tmax [n] float32 for the batch on `scene` (an array of spheres): by a seeded kind per ray,
    the ray's first-hit t, its two neighbours, half and twice it, +inf, 1e5 and min_t."""
    O, D, _ = R.ray_batch(oracle)
    t, _, _ = R.first_hit(scene, O, D)
    return reach_of(t)[0]


def reach_of(t):
    t = np.asarray(t, np.float32)
    n = len(t)
    kind = np.random.default_rng(99).integers(0, 8, n)
    inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        table = [t, np.nextafter(t, inf), np.nextafter(t, np.float32(0)), np.float32(0.5) * t,
                 np.float32(2) * t, np.full(n, inf, np.float32), np.full(n, 1e5, np.float32),
                 np.full(n, MIN_T, np.float32)]
    T = np.choose(kind, table).astype(np.float32)
    return T, kind


def reference(oracle, name):
    """The batch on a scene, computed once: dict of T, kind, occ, accepting, far_first (at T),
    occ_default (at 1e5) and the first hit's t and sphere, with the mask of the contract's rays."""
    key = ("occ", name)
    if key not in _cache:
        O, D, _ = R.ray_batch(oracle)
        sc = R.scene_of(oracle, name)
        t, sphere, _ = R.first_hit(sc, O, D)
        T, kind = reach_of(t)
        occ, accepting, far_first = occluded_ref(sc, O, D, T)
        occ_default, _, _ = occluded_ref(sc, O, D, np.full(len(O), R.INFINITY, np.float32))
        out = dict(T=T, kind=kind, occ=occ, accepting=accepting, far_first=far_first,
                   occ_default=occ_default, t=t, sphere=sphere, finite=R.finite_rays(O, D))
        for v in out.values():
            v.setflags(write=False)
        _cache[key] = out
    return _cache[key]
