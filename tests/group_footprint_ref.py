"""Shared by test_group_footprint_cpu.py, test_gpu_group_footprint.py and
tools/sim/footprint_groups.py: the scenes of the group-footprint tests and an fp32 emulation
(numpy) of the LDS-table flat scan's group mask (tracer.hip group_foot_mask, fact (5g)) beside the
group box test whose survivors it must hold.
"""
import numpy as np

import vulkancomputeraytracing_amd as vc
from tests import footprint_ref as F
from tests.test_cull_cpu import fma, rn
from vulkancomputeraytracing_amd import scene as S

f32 = np.float32


def grid_scene(n_small, scale=1.0, seed=85):
    """A ground sphere (the big list, which the three largest small spheres join) and n_small equal
    spheres at one height on a jittered grid: ceil((n_small - 3) / 4) hierarchy groups with
    members, padded to a multiple of 16."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_small)))
    rows = [((0, -1000, 0), 1000.0, (0.5, 0.5, 0.5), 1, 0.9)]
    for i in range(n_small):
        c = (0.55 * (i % side) - 0.275 * side + float(rng.uniform(-0.1, 0.1)), 0.15,
             0.55 * (i // side) - 0.275 * side + float(rng.uniform(-0.1, 0.1)))
        rows.append((c, 0.15, tuple(rng.uniform(0.2, 1, 3)), 1 + i % 3,
                     float(rng.uniform(0, 1.6))))
    sp = vc.make_spheres(rows)
    if scale != 1.0:
        sp["center"] *= f32(scale)
        sp["radius"] *= f32(scale)
    return sp


def grid128():
    """Exactly 128 hierarchy groups, all with members: the largest eligible scene."""
    return grid_scene(515)


def grid129():
    """129 groups with members (144 with padding): one too many for 128-bit masks."""
    return grid_scene(519)


def grid12():
    """12 groups with members, 4 padding groups."""
    return grid_scene(51)


def tiny_grid():
    """80 groups at one height, scaled by 2^-24: below the coordinate bound of the tables' proof,
    so every mask holds every group with members and every lane pushes them all -- far more than
    the group stack takes at once: the sliced push."""
    return grid_scene(323, scale=2.0 ** -24)


GRID_CAM = dict(lookfrom=(9, 3, 8), lookat=(0, 0.2, 0), vfov=45)
TINY_CAM = dict(lookfrom=(9 * 2.0 ** -24, 3 * 2.0 ** -24, 8 * 2.0 ** -24),
                lookat=(0, 0.2 * 2.0 ** -24, 0), vfov=45)


def group_boxes(t):
    """lo [groups, 3], hi [groups, 3], K [groups], real [groups] (has members) of t["bound"]."""
    b = t["bound"]
    n = 2 * b.shape[0]
    cols = lambda k: np.stack([b[:, k], b[:, k + 1]], 1).reshape(n)  # noqa: E731
    lo = np.stack([cols(0), cols(2), cols(4)], 1)
    hi = np.stack([cols(6), cols(8), cols(10)], 1)
    real = (t["index"][t["nbig"]:] >= 0).any(1)
    return lo, hi, cols(12), real


def box_keep(lo, hi, K, br, slab=None):
    """[rays, boxes] bool: the box test of facts (3), (4) keeps the box (gap >= 0), three-axis
    form, or the slab form (3a) with slab = (lo.y, hi.y)."""
    inv, c, c1, c2 = br
    tn = tf = None
    for k in ((0, 2) if slab is not None else (0, 1, 2)):
        tl = fma(lo[None, :, k], inv[:, k, None], c[:, k, None])
        th = fma(hi[None, :, k], inv[:, k, None], c[:, k, None])
        near, far = np.minimum(tl, th), np.maximum(tl, th)
        tn = near if tn is None else np.maximum(tn, near)
        tf = far if tf is None else np.minimum(tf, far)
    if slab is not None:
        t0, t1 = F.y_interval(br, slab[0], slab[1])
        tn, tf = np.maximum(tn, t0[:, None]), np.minimum(tf, t1[:, None])
    else:
        tn = np.maximum(tn, f32(0))
    with np.errstate(over="ignore", invalid="ignore"):
        gap = fma(np.broadcast_to(K[None, :], tn.shape), np.broadcast_to(c2[:, None], tn.shape),
                  rn(rn(tf - tn) + c1[:, None]))
    return ~(gap < 0)


def group_mask(gf, br, d, y, s_scale=1.0):
    """[rays, 4] uint32 group masks as tracer.hip group_foot_mask computes them: y = the y extent
    whose interval the ray takes (the slab's, or gf["y"]); s_scale scales S for the checker's own
    test."""
    inv, c, c1, c2 = br
    n = gf["tables"].shape[1]
    t0, t1 = F.y_interval(br, y[0], y[1])
    with np.errstate(over="ignore", invalid="ignore"):
        S_ = rn(fma(np.full(len(c1), gf["k2"], f32), c2, rn(c1 + c1)).astype(np.float64) * s_scale)
        ta, tb = rn(t0 - S_), rn(t1 + S_)
        dd = np.where(np.abs(d) < f32(2.0 ** -40), np.copysign(f32(2.0 ** -40), d), d).astype(f32)
        xa, xb = rn(rn(ta - c[:, 0]) * dd[:, 0]), rn(rn(tb - c[:, 0]) * dd[:, 0])
        za, zb = rn(rn(ta - c[:, 2]) * dd[:, 2]), rn(rn(tb - c[:, 2]) * dd[:, 2])
    assert not (np.isnan(xa) | np.isnan(xb) | np.isnan(za) | np.isnan(zb)).any()
    ixa, ixb = F.cell(xa, gf["x"], n), F.cell(xb, gf["x"], n)
    iza, izb = F.cell(za, gf["z"], n), F.cell(zb, gf["z"], n)
    x0, x1 = np.minimum(ixa, ixb), np.maximum(ixa, ixb)
    z0, z1 = np.minimum(iza, izb), np.maximum(iza, izb)
    T = gf["tables"]
    m = T[0][x1] & T[1][x0] & T[2][z1] & T[3][z0]  # [rays, 4]
    m = np.where((tb < ta)[:, None], np.uint32(0), m) | gf["always"][None, :].astype(np.uint32)
    return m


def mask_bits(m, ngroups):
    """[rays, ngroups] bool from [rays, 4] uint32 masks."""
    g = np.arange(ngroups)
    return ((m[:, g >> 5] >> (g & 31).astype(np.uint32)[None, :]) & 1).astype(bool)


def build_tables(lo, hi, real, so_x, so_z, n):
    """cluster.cpp's group tables from the group boxes (lo, hi [groups, 3]) and the cells' (scale,
    offset), in float64: footprint_ref.build_tables' rule with 128-bit masks, [4, n, 4] uint32."""
    out = np.zeros((4, n, 4), np.uint32)
    g = np.arange(len(lo))
    word = (np.uint32(1) << (g & 31).astype(np.uint32)) * real
    for a, so in ((0, so_x), (2, so_z)):
        i = np.arange(n - 1)
        lo_k = np.full(n - 1, F.key_of(f32(-np.inf)))
        hi_k = np.full(n - 1, F.key_of(f32(np.inf)))
        while (hi_k - lo_k > 1).any():
            mid = lo_k + (hi_k - lo_k) // 2
            below = F.cell(F.float_of(mid), so, n) <= i
            lo_k, hi_k = np.where(below, mid, lo_k), np.where(below, hi_k, mid)
        ue = np.concatenate([F.float_of(lo_k).astype(np.float64), [np.inf]])
        le = np.concatenate([[-np.inf], ue[:-1]])
        up = ue + (8.0 * 2.0 ** -24 * np.abs(ue) + 2.0 ** -100)
        dn = le - (8.0 * 2.0 ** -24 * np.abs(le) + 2.0 ** -100)
        A = (lo[None, :, a].astype(np.float64) <= up[:, None])
        B = (hi[None, :, a].astype(np.float64) >= dn[:, None])
        t = 0 if a == 0 else 2
        for w in range(4):
            sel = (g >> 5) == w
            out[t, :, w] = (A[:, sel] * word[None, sel]).sum(1).astype(np.uint32)
            out[t + 1, :, w] = (B[:, sel] * word[None, sel]).sum(1).astype(np.uint32)
    return out


def scene_tables(sp):
    """(cull tables, group footprint tables or None, slab or None) of a scene."""
    return S.cull_tables(sp), S.cull_group_footprint(sp), S.cull_slab(sp)
