"""Adaptive sampling restated for the tests (no tests here): include/vcrt.h vcrt_draw_samples and
vcrt_sample_counts in numpy float32, built from parts that exist -- the frame's rays from
vcrt_frame_rays (vc.frame_rays, the definition as code), each ray's radiance from the oracle's
ray_color as tests/ray_query_ref.oracle_paths calls it, the two-level sum in explicit fp32, the
packed tiles of a shard through tests/features_ref.packed."""
import numpy as np

import vulkancomputeraytracing_amd as vc
from tests import features_ref as FR
from tests import ray_query_ref as R

F = np.float32
Q = 4  # the quantum: vcrt_work_quantum's base
LOW = 12

_cache = {}


def radiance(oracle, scene, desc, first, n, pixels=None):
    """r_i of sample indices first .. first + n - 1 for the frame's pixels (all, or the flat
    indices `pixels`): float32 [pixels, n, 3], ray_color at desc.max_depth. Cached by the
    arguments' values (the scene by identity), read-only."""
    key = (id(scene), desc.width, desc.height, tuple(desc.lookfrom), tuple(desc.lookat),
           tuple(desc.vup), desc.vfov, float(desc.lens_radius), desc.max_depth, first, n,
           None if pixels is None else tuple(int(p) for p in pixels))
    if key not in _cache:
        h, w = desc.height, desc.width
        idx = np.arange(h * w) if pixels is None else np.asarray(pixels)
        xy = np.stack([idx % w, idx // w], axis=1)
        o, d = vc.frame_rays(desc, xy, first, n)
        rgb, segs = R.oracle_paths(oracle, scene, o.reshape(-1, 3), d.reshape(-1, 3),
                                   desc.max_depth)
        rgb = rgb.reshape(len(idx), n, 3)
        rgb.setflags(write=False)
        _cache[key] = (rgb, segs.reshape(len(idx), n), scene)  # (the scene kept alive)
    return _cache[key][0], _cache[key][1]


def clamp_counts(counts, max_count):
    return np.minimum(np.asarray(counts, np.int64), max_count)


def pixel_sum(r):
    """S_p of one pixel's radiance r [n_p, 3] in index order: quanta of Q summed from +0, then the
    quanta summed from +0 in ascending k; every add rounded to fp32."""
    s_p = np.zeros(3, F)
    with np.errstate(all="ignore"):
        for k in range(0, len(r), Q):
            s_k = np.zeros(3, F)
            for v in r[k:k + Q]:
                s_k = (s_k + v).astype(F)
            s_p = (s_p + s_k).astype(F)
    return s_p


def draw_samples(oracle, scene, desc, counts, first, max_count, sums=None, sparse=False):
    """The whole frame's planes: (sums [H, W, 4], mean [H, W, 4], stats) for a count plane
    [H, W]. sums=None: accumulate == 0; else the old plane, which is accumulated into a copy.
    stats: samples, pixels, items, segments. sparse: the batch of low sample indices covers the
    pixels with a sample only, and only the indices they use (a large frame with few such
    pixels, a `first` whose first + LOW would pass the largest index); the planes are the same."""
    h, w = desc.height, desc.width
    n = clamp_counts(counts, max_count).reshape(-1)
    out = (np.zeros((h * w, 4), F) if sums is None
           else np.array(sums, F, copy=True).reshape(h * w, 4))
    # every pixel's first LOW indices in one batch that the count planes share, the rest per pixel
    low = LOW if n.max() > 0 else 0
    row = None  # pixel -> row of the batch (None: the pixel itself)
    if sparse and low:
        some = np.flatnonzero(n)
        few = n[some][n[some] <= LOW]
        low = int(few.max()) if few.size else 0
        row = np.full(h * w, -1, np.int64)
        row[some] = np.arange(len(some))
    rad, segs = (radiance(oracle, scene, desc, first, low, pixels=None if row is None else some)
                 if low else (None, None))
    nseg = 0
    for p in np.flatnonzero(n):
        if n[p] <= low:
            q = p if row is None else row[p]
            r, sg = rad[q, :n[p]], segs[q, :n[p]]
        else:
            r, sg = radiance(oracle, scene, desc, first, int(n[p]), pixels=[p])
            r, sg = r[0], sg[0]
        nseg += int(sg.sum())
        s = pixel_sum(r)
        if sums is None:
            out[p] = (s[0], s[1], s[2], F(n[p]))
        else:
            out[p, :3] = (out[p, :3] + s).astype(F)
            out[p, 3] = F(out[p, 3] + F(n[p]))
    mean = np.zeros((h * w, 4), F)
    mean[:, 3] = 1
    some = out[:, 3] != 0
    with np.errstate(all="ignore"):
        mean[some, :3] = (out[some, :3] / out[some, 3:4]).astype(F)
    stats = dict(samples=int(n.sum()), pixels=int((n > 0).sum()),
                 items=int(((n + Q - 1) // Q).sum()), segments=nseg)
    return out.reshape(h, w, 4), mean.reshape(h, w, 4), stats


def packed(plane, width, height, world, rank, fill):
    """A frame plane as rank `rank`'s packed tiles; slots outside the frame hold `fill`."""
    return FR.packed(plane, width, height, world, rank, fill)


def sample_counts(variance, target, min_count, max_count):
    """vcrt_sample_counts in numpy: uint16 in variance's shape, and the total."""
    v = np.asarray(variance, F)
    with np.errstate(all="ignore"):
        k = F(1.0) / F(F(target) * F(target))
        t = (np.fmax(v, F(0.0)) * k).astype(F)  # fmax: a NaN gives 0
        big = t >= F(max_count)
        c = np.where(big, max_count, np.ceil(np.where(big, F(0), t))).astype(np.int64)
    c = np.maximum(c, min_count).astype(np.uint16)
    return c, int(c.astype(np.int64).sum())
