"""Shared inputs of the frame-pass fuzz tests (no tests here): the generated scenes of
tests/query_fuzz_ref.py as 44 x 20 frames for vcrt_draw_features, vcrt_draw_occlusion and
vcrt_draw_motion (tracer.hip parts 8, 10 and 12).

* frame(name): the case's scene and environment, its camera (the case's own, else eye -> box
  centre at vfov 40, else CAMERA's entry), and the seeded parameters: samples n, first index,
  secondary rays m, reach, lens radius, the previous state of the motion pass.
* previous(f): (prev_desc, prev_scene, changed) of the previous state: same, orbit, orbit-moved,
  through, moved-only.
* reference(oracle, f): features, ambient and motion through tests/features_ref.py,
  tests/ambient_ref.py and tests/motion_ref.py, computed once per case.
* routes(oracle, f): which of the passes' three routes the case's rays take, from the host
  builders alone (query_fuzz_ref.tables_of / bounded, scene.primary_sphere_lists).
* fallback(oracle, f): where the hit's normal needs the full division (divs).
tests/test_frame_fuzz_cpu.py holds the conditions on these inputs; tests/test_gpu_frame_fuzz.py
runs them on the GPU.
"""
import math
import os
import zlib

import numpy as np

import vulkancomputeraytracing_amd as vc
from tests import ambient_ref as AR
from tests import features_ref as FR
from tests import lens_ref as L
from tests import motion_ref as M
from tests import query_fuzz_ref as Q
from tests import ray_query_ref as R
from vulkancomputeraytracing_amd.renderer import tile_pixel_map

F = np.float32
W, H = 44, 20              # both edges partial: 6 x 3 tiles, 72 quarters
CASE_NAMES = Q.CASE_NAMES
MIN_T = 0.001
LENS_RADIUS = 0.1
SAMPLES, FIRSTS, SECONDARY = (1, 2, 5), (0, 7), (1, 3)
REACH_KINDS = ("far", "median", "min_t")
PREV_KINDS = ("same", "orbit", "orbit-moved", "through", "moved-only")

# Camera fields that replace the case's own, each with its reason.
_ALONG_THE_LINE = dict(lookfrom=(-8.0, 1.0, 0.8), lookat=(-3.0, 0.5, 0.0), vup=(0.0, 1.0, 0.0),
                       vfov=14.0)
# 0.003 under the glass sphere's surface (centre (0, 1, 6), radius 3) with |d| about 3: the way
# out is a root on either side of min_t = 0.001, so about half of the rays see the glass from
# inside and the others the spheres beyond it
_UNDER_THE_GLASS = dict(lookfrom=(0.0, 1.0, 3.003), lookat=(0.0, 0.5, 0.0), vup=(0.0, 1.0, 0.0),
                        vfov=60.0)
CAMERA = {
    # the query cameras see the line of spheres as a thin strip (1 to 6 % of the frame): from
    # near one end along the row, a narrow field of view
    **{f"fuzz-line-{s}": _ALONG_THE_LINE for s in Q.FUZZ_SEEDS["line"]},
    "edge-line-one-radius": _ALONG_THE_LINE,
    # make_case's camera (vfov 94 from 16 away, a tilted vup) sees the ground alone
    "fuzz-cluster-0": dict(lookfrom=(4.0, 3.0, 12.0), lookat=(0.0, 0.5, 0.0),
                           vup=(0.0, 1.0, 0.0), vfov=30.0),
    # from the field outwards at the ring: every sphere in view (the ground, two of the ring) is
    # in the big groups, so every quarter's list is empty -- count 0, the big groups alone
    "shape-big4": dict(lookfrom=(0.0, 3.0, 5.0), lookat=(-30.0, 8.0, 100.0),
                       vup=(0.0, 1.0, 0.0), vfov=70.0),
    # from the middle of the glass sphere every first hit is the glass itself or a sphere that
    # reaches into it: aimed at one that does (two distinct spheres otherwise) ...
    "fuzz-inside-5": dict(lookat=(-0.42, -0.16, 2.84), vfov=15.0),
    "fuzz-inside-17": dict(lookat=(1.51, 1.15, 2.91), vfov=30.0),
    # ... and where none does, from just under the glass
    "fuzz-inside-11": _UNDER_THE_GLASS,
    "fuzz-inside-23": _UNDER_THE_GLASS,
    "fuzz-inside-29": _UNDER_THE_GLASS,
}

# `through`: where the previous camera stands, as the share of the way from the eye to the centre
# of the box (1: the centre itself, the rule), for the cases whose visible surfaces all lie on one
# side of a camera there.
THROUGH_AT = {
    "fuzz-big-4": 0.7,       # the eye is above the cluster: from its centre 99 % projects
    "fuzz-line-21": 1.4,     # (as fuzz-line-15; 1.4: past the centre, still between the spheres)
    "fuzz-line-15": 0.8,     # from the centre no projected point lands on its own sphere again:
                             # reproject would take no history at all
}

# Reach kinds that replace the seeded draw, each with its reason.
REACH = {
    # a NaN root passes the reference's range test at any reach, while the contract of
    # vcrt_draw_occlusion leaves every ray open at a reach <= min_t: only a reach above min_t is
    # defined by both
    "edge-nan-centre": "far",
}

# Previous states that replace the seeded draw, each with its reason.
PREVIOUS = {
    # every pixel that hits the 2.9e9 sphere takes the divs fallback (nmax > 2^30): the motion
    # pass uses the normal only off the identity route
    "edge-huge-radius": "orbit",
    # a radius below 2^-40 clears kFlagRadiiSafe for the whole scene: likewise
    "edge-tiny-radius": "orbit-moved",
    "edge-zero-radius": "through",
    # every ray "hits" the NaN sphere: under the same camera all 880 pixels are identity
    # pixels; after an orbit the pass has to project the NaN points (none projects)
    "edge-nan-centre": "orbit",
    # around the eye is one glass sphere: a camera anywhere on the way to the box's centre either
    # has all of it in front (nothing rejected) or projects no point onto its own sphere again
    # (reproject takes nothing), so `through` has nothing to show here
    "fuzz-inside-17": "orbit",
}

_cache = {}


# ---------------------------------------------------------------------------------- the cases

def _camera(c):
    cam = dict(c["cam"])
    g = Q.geometry(c["scene"])
    if not cam:
        centre = 0.5 * (g["lo"] + g["hi"])
        cam = dict(lookfrom=c["eye"], lookat=tuple(float(F(v)) for v in centre), vfov=40.0)
    for k, v in CAMERA.get(c["name"], {}).items():
        cam[k] = v
    cam.setdefault("vup", (0.0, 1.0, 0.0))
    return {k: (tuple(float(x) for x in v) if k != "vfov" else float(v)) for k, v in cam.items()}


def frame(name, oracle=None):
    """One frame case: the query fuzz's case (scene, env, ...) plus cam, n, first, m, reach,
    reach_kind, lens, prev and desc (the RenderDesc of the renderer the GPU test opens)."""
    key = ("frame", name)
    if key in _cache:
        return _cache[key]
    c = Q.case(name, oracle)
    rng = np.random.default_rng([20261021, zlib.crc32(name.encode())])
    n = int(rng.choice(SAMPLES))
    first = int(rng.choice(FIRSTS))
    m = int(rng.choice(SECONDARY))
    reach_kind = REACH.get(name, str(rng.choice(REACH_KINDS, p=(0.4, 0.4, 0.2))))
    low = float(rng.choice((MIN_T, 0.0)))
    prev = str(rng.choice(PREV_KINDS))
    rmed = Q.geometry(c["scene"])["rmed"]
    reach = {"far": 1e5, "median": float(F(rmed)), "min_t": low}[reach_kind]
    lens = LENS_RADIUS if CASE_NAMES.index(name) % 4 == 3 else 0.0
    cam = _camera(c)
    desc = vc.RenderDesc(width=W, height=H, samples_per_pixel=4, max_depth=3, device=0,
                         lens_radius=lens, **cam)
    f = dict(c, cam=cam, n=n, first=first, m=m, reach=reach, reach_kind=reach_kind, lens=lens,
             prev=PREVIOUS.get(name, prev), desc=desc, rmed=rmed)
    _cache[key] = f
    return f


def pinhole(f):
    """The case's description without the lens (the motion pass's rays, the lists' camera)."""
    d = f["desc"]
    return vc.RenderDesc(width=W, height=H, samples_per_pixel=4, max_depth=3, device=0, **f["cam"])\
        if d.lens_radius > 0 else d


def frames(oracle=None):
    return [frame(name, oracle) for name in CASE_NAMES]


# ------------------------------------------------------------------------- the previous state

def _orbit(desc, degrees):
    """desc's camera turned about the y axis through lookat (in double, rounded to float)."""
    th = math.radians(degrees)
    dx, dz = desc.lookfrom[0] - desc.lookat[0], desc.lookfrom[2] - desc.lookat[2]
    return desc.with_camera(lookfrom=(
        float(F(desc.lookat[0] + dx * math.cos(th) + dz * math.sin(th))), desc.lookfrom[1],
        float(F(desc.lookat[2] - dx * math.sin(th) + dz * math.cos(th)))))


def _most_seen(oracle, f, among):
    """The sphere of `among` (a mask) under the most centre rays, or -1."""
    _, s, _ = M.first_hits(oracle, f["scene"], pinhole(f))
    seen = np.bincount(s[s >= 0], minlength=len(f["scene"])) * among
    return int(np.argmax(seen)) if seen.any() else -1


def previous(oracle, f):
    """(prev_desc, prev_scene, changed): None is the current one; `changed` the sphere whose
    radius alone differs (-1: none).

    same         nothing moved.
    orbit        the camera 3 degrees further round lookat.
    orbit-moved  that, the spheres up to 8 x the median radius shifted by a quarter of it in x
                 and -z, and the radius of the most seen sphere (shifted or not) grown by a
                 quarter with its previous centre the current one.
    through      the camera at the centre of the box (THROUGH_AT: elsewhere on the line from the
                 eye through it), looking back at the current eye: the surfaces beyond it lie
                 behind it or near its plane.
    moved-only   the same camera; every third sphere shifted, and the most seen of the others
                 with another radius and the same centre, so the identity test's fourth word
                 decides."""
    key = ("prev", f["name"])
    if key in _cache:
        return _cache[key]
    kind, desc, scene = f["prev"], pinhole(f), f["scene"]
    g = Q.geometry(scene)
    step = F(0.25 * f["rmed"])
    prev_desc, prev_scene, changed = None, None, -1
    if kind in ("orbit", "orbit-moved"):
        prev_desc = _orbit(desc, 3.0)
    if kind == "through":
        eye = np.asarray(desc.lookfrom, np.float64)
        at = eye + THROUGH_AT.get(f["name"], 1.0) * (0.5 * (g["lo"] + g["hi"]) - eye)
        prev_desc = desc.with_camera(lookfrom=tuple(float(F(v)) for v in at),
                                     lookat=desc.lookfrom)
    if kind in ("orbit-moved", "moved-only"):
        prev_scene = scene.copy()
        small = g["ok"] & (np.abs(g["rad"]) <= 8.0 * g["rmed"])
        move = small if kind == "orbit-moved" else g["ok"] & (np.arange(len(scene)) % 3 == 0)
        i = np.flatnonzero(move)
        prev_scene["center"][i, 0] += step
        prev_scene["center"][i, 2] -= step
        changed = _most_seen(oracle, f, g["ok"] if kind == "orbit-moved" else g["ok"] & ~move)
        if changed >= 0:
            prev_scene["center"][changed] = scene["center"][changed]
            prev_scene["radius"][changed] = F(scene["radius"][changed] * F(1.25))
        prev_scene.setflags(write=False)
    _cache[key] = (prev_desc, prev_scene, changed)
    return _cache[key]


# ------------------------------------------------------------------------------ the references

def reference(oracle, f):
    """dict of features (features_ref.frame_features), ambient (ambient_ref.frame_occlusion) and
    motion (motion_ref.frame_motion) of the case, computed once."""
    key = ("ref", f["name"])
    if key not in _cache:
        prev_desc, prev_scene, _ = previous(oracle, f)
        _cache[key] = dict(
            features=FR.frame_features(oracle, f["scene"], f["desc"], f["first"], f["n"]),
            ambient=AR.frame_occlusion(oracle, f["scene"], f["desc"], f["first"], f["n"], f["m"],
                                       f["reach"]),
            motion=M.frame_motion(oracle, f["scene"], pinhole(f), prev_desc, prev_scene))
    return _cache[key]


def sample_hits(oracle, f):
    """(O, D, t, sphere, normal) of the frame's own rays, [H * W * n] sample-minor, as the
    feature and ambient references trace them."""
    key = ("hits", f["name"])
    if key not in _cache:
        origins, dirs = L.frame_rays(oracle, f["desc"], f["first"], f["n"])
        D = np.ascontiguousarray(dirs.reshape(-1, 3))
        O = np.ascontiguousarray(np.broadcast_to(origins, dirs.shape).reshape(-1, 3))
        _cache[key] = (O, D) + tuple(R.first_hit(f["scene"], O, D))
    return _cache[key]


def radii_safe(scene):
    """capi.cpp, values_radii_safe: every |radius| in [2^-40, 2^30] (NaN fails)."""
    with np.errstate(invalid="ignore"):
        r = np.abs(scene["radius"])
        return bool(((r >= F(2.0 ** -40)) & (r <= F(2.0 ** 30))).all())


def fallback(oracle, f):
    """dict: radii_safe, and the number of hit samples whose point - centre has a component
    below 2^-40 or above 2^30 in magnitude (tracer.hip: the normal's guarded division falls back
    to divs) among the frame's samples (`samples`) and among the centre rays (`centre`)."""
    def count(O, D, t, s):
        hit = s >= 0
        with np.errstate(all="ignore"):
            P = ((t[:, None] * D).astype(F) + O).astype(F)
            pcv = np.abs((P - f["scene"]["center"][np.where(hit, s, 0)]).astype(F))
            out = hit & ~((pcv.min(axis=1) >= F(2.0 ** -40)) & (pcv.max(axis=1) <= F(2.0 ** 30)))
        return int(out.sum())
    O, D, t, s, _ = sample_hits(oracle, f)
    desc = pinhole(f)
    o, d = M.centre_rays(oracle, desc)
    Dc = np.ascontiguousarray(d.reshape(-1, 3))
    tc, sc, _ = M.first_hits(oracle, f["scene"], desc)
    return dict(radii_safe=radii_safe(f["scene"]), samples=count(O, D, t, s),
                centre=count(np.broadcast_to(o, Dc.shape), Dc, tc, sc))


def colour_planes():
    """(frame, history) float32 [H, W, 4]: seeded colour planes for the consumers (reproject's
    history in the GPU test; both where no renderer draws a frame)."""
    if "colour" not in _cache:
        rng = np.random.default_rng(20261021)
        _cache["colour"] = tuple(rng.uniform(0.0, 2.0, (H, W, 4)).astype(F) for _ in range(2))
        for v in _cache["colour"]:
            v.setflags(write=False)
    return _cache["colour"]


# ----------------------------------------------------------------------------------- the routes

def lists_of(f):
    """scene.primary_sphere_lists of the case's pinhole camera under the case's environment."""
    old = {k: os.environ.get(k) for k in f["env"]}
    os.environ.update(f["env"])
    try:
        return vc.scene.primary_sphere_lists(f["scene"], pinhole(f))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def guard_a(aa):
    """vcrt_math.h guard_a: aa in [2^-20, 2^60]."""
    with np.errstate(invalid="ignore"):
        return (aa >= F(2.0 ** -20)) & (aa <= F(2.0 ** 60))


def _dot_dd(d):
    with np.errstate(all="ignore"):
        return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F) +
                d[..., 2] * d[..., 2]).astype(F)


def routes(oracle, f):
    """What the host builders say about the routes of the case's rays, no GPU:
    tables, bounded     the scene has culling tables / is bounded;
    words               [H, W] uint32, the list word of each pixel's quarter (count in the low
                        four bits, 15: no list), None where the frame has no lists (no tables,
                        unbounded);
    counts              the counts (0 .. 14) of the listed quarters that hold a pixel;
    listed, unlisted    the quarters with a pixel that have / lack a list;
    mixed_tiles         the tiles whose quarters with pixels mix the two;
    pairs, pairs_centre the (pixel, sample) pairs in a listed quarter for the frame's n samples
                        and for the centre rays, and guarded_*: those with dot(d, d) inside
                        guard_a's range (a pinhole frame: the lists serve no other).
    A lens renderer takes no list: the GPU test sets its prediction to 0 itself."""
    key = ("routes", f["name"])
    if key in _cache:
        return _cache[key]
    out = dict(tables=Q.tables_of(f) is not None, bounded=Q.bounded(f["scene"]), words=None,
               counts=np.zeros(0, np.int64), listed=0, unlisted=0, mixed_tiles=0, pairs=0,
               pairs_centre=0, guarded_pairs=0, guarded_centre=0)
    m = tile_pixel_map(W, H, 1)
    slot = m[..., 1].astype(np.int64)
    lane = slot % 64
    quarter = 4 * (slot // 64) + 2 * ((lane >> 5) & 1) + ((lane >> 2) & 1)
    quarters = np.unique(quarter)
    out["unlisted"] = len(quarters)
    sl = lists_of(f)
    if sl is not None:
        info = sl["info"]
        words = info[quarter]
        has = (words & 15) != 15
        cnt = (info[quarters] & 15).astype(np.int64)
        out.update(words=words, counts=cnt[cnt != 15], listed=int((cnt != 15).sum()),
                   unlisted=int((cnt == 15).sum()))
        tile_has = {}
        for q in quarters:
            tile_has.setdefault(int(q) // 4, set()).add(bool((info[q] & 15) != 15))
        out["mixed_tiles"] = sum(len(v) == 2 for v in tile_has.values())
        pin = pinhole(f)
        _, dirs = L.frame_rays(oracle, pin, f["first"], f["n"])          # [H, W, n, 3]
        ga = guard_a(_dot_dd(dirs))
        _, dc = M.centre_rays(oracle, pin)
        gc = guard_a(_dot_dd(dc))
        out.update(pairs=int(has.sum()) * f["n"], pairs_centre=int(has.sum()),
                   guarded_pairs=int((ga & has[..., None]).sum()),
                   guarded_centre=int((gc & has).sum()))
    _cache[key] = out
    return out
