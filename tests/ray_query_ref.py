"""Shared inputs and references of the ray-query tests (no tests here).

* ray_batch(): a seeded batch of 4133 rays (64 * 64 + 37: a partly filled last claim and many
  refills) in contiguous classes, the rays outside the culled scans' guarded range last.
* first_hit(): hit_sphere (functions.glsl:14-40) restated in numpy float32, every operation
  rounded on its own -- what -ffp-contract=off C does.
* oracle_paths(): oracle_ray_color for every ray of a batch.
* scene_of(): the scenes the GPU parity runs on.
"""
import ctypes

import numpy as np

N_RAYS = 4133
# class -> rays; A takes the rest. F + G + H stay below a tenth of the batch.
SIZES = {"B": 1000, "C": 500, "D": 500, "E": 400, "F": 200, "G": 100, "H": 30}
SIZES = {"A": N_RAYS - sum(SIZES.values()), **SIZES}
MIN_T = np.float32(0.001)
INFINITY = np.float32(1e5)

_cache = {}


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ray_batch(oracle):
    """(origins [n, 3] float32, dirs [n, 3] float32, classes [n] of 'A'..'H'). The geometry of
    classes D and E is the final scene's; the same batch runs on every scene."""
    if "batch" in _cache:
        return _cache["batch"]
    rng = np.random.default_rng(20261019)
    final = oracle.scene("final")
    cen = final["center"].astype(np.float64)
    rad = final["radius"].astype(np.float64)
    O, D, C = [], [], []

    def put(cls, o, d):
        assert len(o) == len(d) == SIZES[cls], cls
        O.append(np.asarray(o, np.float64).astype(np.float32))
        D.append(np.asarray(d, np.float64).astype(np.float32))
        C.extend(cls * len(o))

    def box(n, ylo=0.05, yhi=3.0):
        return np.stack([rng.uniform(-11, 11, n), rng.uniform(ylo, yhi, n),
                         rng.uniform(-11, 11, n)], axis=1)

    # (A) camera-like: from (13, 2, 3) at points among the spheres, unnormalised
    n = SIZES["A"]
    eye = np.array([13.0, 2.0, 3.0])
    tgt = np.stack([rng.uniform(-9, 9, n), rng.uniform(0.0, 1.2, n), rng.uniform(-9, 9, n)], 1)
    put("A", np.tile(eye, (n, 1)), (tgt - eye) * rng.uniform(0.05, 1.5, (n, 1)))
    # (B) anywhere in the scene's box, any direction, lengths 2^-8 .. 2^8
    n = SIZES["B"]
    put("B", box(n), _unit(rng, n) * np.exp2(rng.integers(-8, 9, (n, 1)).astype(np.float64)))
    # (C) at the small spheres' height, one or two direction components exactly 0: along the
    # y slab of the hierarchy's boxes, and along the axes
    n = SIZES["C"]
    d = _unit(rng, n)
    kind = rng.integers(0, 6, n)
    zero = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 1]], bool)
    d[zero[kind]] = 0.0
    put("C", box(n, 0.02, 0.38), d)
    # (D) inside spheres: small ones, the big three (glass among them) and the ground sphere
    n = SIZES["D"]
    which = rng.integers(0, len(final), n)
    which[: n // 5] = len(final) - 1                       # the ground sphere
    which[n // 5: n // 5 + n // 10] = rng.integers(len(final) - 4, len(final) - 1, n // 10)
    o = cen[which] + rad[which][:, None] * _unit(rng, n) * rng.uniform(0.0, 0.95, (n, 1))
    g = which == len(final) - 1     # just below the ground's surface (0.1 lower at the corners)
    o[g] = np.stack([rng.uniform(-10, 10, g.sum()), rng.uniform(-0.5, -0.11, g.sum()),
                     rng.uniform(-10, 10, g.sum())], 1)
    put("D", o, _unit(rng, n) * rng.uniform(0.5, 2.0, (n, 1)))
    # (E) on sphere surfaces, directions close to the tangent plane (both sides of it)
    n = SIZES["E"]
    which = rng.integers(0, len(final) - 1, n)
    nrm = _unit(rng, n)
    tan = np.cross(nrm, _unit(rng, n))
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    eps = rng.choice([-1e-2, -1e-4, 0.0, 1e-5, 1e-3, 3e-2], n)[:, None]
    put("E", cen[which] + rad[which][:, None] * nrm, tan + eps * nrm)
    # (F) |d|^2 just below and just above the guard's bounds 2^-20 and 2^60
    n = SIZES["F"]
    length = rng.choice([2.0 ** -10, 2.0 ** 30], n) * rng.choice([0.999, 1.001], n)
    tgt = np.stack([rng.uniform(-9, 9, n), rng.uniform(0.0, 1.0, n), rng.uniform(-9, 9, n)], 1)
    o = box(n)
    d = tgt - o
    put("F", o, d / np.linalg.norm(d, axis=1, keepdims=True) * length[:, None])
    # (G) origins 2^27 .. 2^32 away, aimed at the scene (about unit length)
    n = SIZES["G"]
    away = _unit(rng, n)
    away[:, 1] = np.abs(away[:, 1])
    o = away * np.exp2(rng.integers(27, 33, (n, 1)).astype(np.float64))
    tgt = np.stack([rng.uniform(-9, 9, n), rng.uniform(0.0, 1.0, n), rng.uniform(-9, 9, n)], 1)
    d = tgt - o
    put("G", o, d / np.linalg.norm(d, axis=1, keepdims=True))
    # (H) a non-finite component, or a zero direction
    n = SIZES["H"]
    o, d = box(n), _unit(rng, n)
    bad = [np.inf, -np.inf, np.nan]
    for i in range(n):
        if i % 3 == 0:
            d[i] = 0.0
        elif i % 3 == 1:
            d[i, rng.integers(0, 3)] = bad[(i // 3) % 3]
        else:
            o[i, rng.integers(0, 3)] = bad[(i // 3) % 3]
    put("H", o, d)

    O = np.ascontiguousarray(np.concatenate(O))
    D = np.ascontiguousarray(np.concatenate(D))
    C = np.array(C)
    assert O.shape == D.shape == (N_RAYS, 3) and C.shape == (N_RAYS,)
    for a in (O, D, C):
        a.setflags(write=False)
    _cache["batch"] = (O, D, C)
    return _cache["batch"]


def finite_rays(O, D):
    """The rays the parity contract covers: six finite components, a direction not all zero."""
    return np.isfinite(O).all(axis=1) & np.isfinite(D).all(axis=1) & (D != 0).any(axis=1)


def first_hit(scene, O, D):
    """hit_sphere over the whole list in index order (functions.glsl:14-40, 77-81), vectorised
    over the rays: (t [n] float32, 1e5 on a miss; sphere [n] int32, -1; normal [n, 3], 0)."""
    O = np.asarray(O, np.float32)
    D = np.asarray(D, np.float32)
    n = len(O)
    ox, oy, oz = O[:, 0], O[:, 1], O[:, 2]
    dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]
    max_t = np.full(n, INFINITY, np.float32)
    best = np.full(n, -1, np.int32)
    normal = np.zeros((n, 3), np.float32)
    with np.errstate(all="ignore"):
        a = (dx * dx + dy * dy) + dz * dz
        for i, s in enumerate(scene):
            cx, cy, cz = (np.float32(v) for v in s["center"])
            r = np.float32(s["radius"])
            ocx, ocy, ocz = ox - cx, oy - cy, oz - cz
            half_b = (ocx * dx + ocy * dy) + ocz * dz
            cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - r * r
            disc = half_b * half_b - a * cc
            cand = ~(disc < 0)
            if not cand.any():
                continue
            sq = np.sqrt(disc)
            root = (-half_b - sq) / a
            far = cand & ((root <= MIN_T) | (max_t <= root))
            root2 = (-half_b + sq) / a
            root = np.where(far, root2, root)
            take = cand & ~(far & ((root2 <= MIN_T) | (max_t <= root2)))
            if not take.any():
                continue
            max_t = np.where(take, root, max_t)
            best = np.where(take, np.int32(i), best)
            px, py, pz = root * dx + ox, root * dy + oy, root * dz + oz
            nr = np.stack([(px - cx) / r, (py - cy) / r, (pz - cz) / r], axis=1)
            normal = np.where(take[:, None], nr, normal)
    return max_t.astype(np.float32), best, normal.astype(np.float32)


def oracle_paths(oracle, scene, O, D, depth):
    """oracle_ray_color of every ray: (rgb [n, 3] float32, segments [n] uint64)."""
    from tests.oracle_py import SPHERE_DTYPE
    scene = np.ascontiguousarray(scene, dtype=SPHERE_DTYPE)
    O = np.ascontiguousarray(O, np.float32)
    D = np.ascontiguousarray(D, np.float32)
    rgb = np.zeros((len(O), 3), np.float32)
    segs = np.zeros(len(O), np.uint64)
    f = oracle.lib.oracle_ray_color
    sp, ns = scene.ctypes.data, len(scene)
    po, pd, pc, ps = O.ctypes.data, D.ctypes.data, rgb.ctypes.data, segs.ctypes.data
    seg_t = ctypes.POINTER(ctypes.c_uint64)
    for i in range(len(O)):
        f(sp, ns, po + 12 * i, pd + 12 * i, depth, pc + 12 * i,
          ctypes.cast(ps + 8 * i, seg_t))
    return rgb, segs


def mixed_scene():
    """About 40 spheres of mixed radii and heights, all three materials, on a ground sphere:
    culling tables without a shared y slab."""
    rng = np.random.default_rng(41)
    from tests.oracle_py import SPHERE_DTYPE
    arr = np.zeros(41, dtype=SPHERE_DTYPE)
    for i in range(40):
        r = float(rng.choice([0.15, 0.25, 0.4, 0.7]))
        arr[i]["center"] = (rng.uniform(-7, 7), r + float(rng.uniform(0, 1.5)),
                            rng.uniform(-7, 7))
        arr[i]["radius"] = r
        arr[i]["colour"] = rng.uniform(0.2, 1.0, 3)
        arr[i]["texture"] = (1 + i % 3, [0.8, 0.3, 1.5][i % 3], 0.0)
    arr[40]["center"], arr[40]["radius"] = (0, -1000, 0), 1000.0
    arr[40]["colour"], arr[40]["texture"] = (0.5, 0.5, 0.5), (1, 1.0, 0.0)
    return arr


SCENES = ("three", "final", "bright", "stress4096", "mixed")


def scene_of(oracle, name):
    if name not in _cache:
        sc = mixed_scene() if name == "mixed" else oracle.scene(name)
        sc.setflags(write=False)
        _cache[name] = sc
    return _cache[name]





def reference(oracle, name, depth=10):
    """The whole batch on a scene, computed once: dict of rgb, segs (oracle) and t, sphere,
    normal (first_hit), with the mask of the rays the contract covers."""
    key = ("ref", name, depth)
    if key not in _cache:
        O, D, _ = ray_batch(oracle)
        sc = scene_of(oracle, name)
        rgb, segs = oracle_paths(oracle, sc, O, D, depth)
        t, sphere, normal = first_hit(sc, O, D)
        _cache[key] = dict(rgb=rgb, segs=segs, t=t, sphere=sphere, normal=normal,
                           finite=finite_rays(O, D))
    return _cache[key]
