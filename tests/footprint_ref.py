"""Shared by test_cull_footprint_cpu.py, test_gpu_footprint.py and tools/sim/footprint_nodes.py: the
scenes of the footprint tests and an fp32 emulation (numpy) of the LDS-table flat scan's node
mask (tracer.hip foot_mask, fact (5)) beside the node box test it replaces.
"""
import numpy as np

import vulkancomputeraytracing_amd as vc
from tests.test_cull_cpu import fma, rn
from vulkancomputeraytracing_amd import scene as S

f32 = np.float32


def tall_scene():
    """120 spheres of varied radii at varied heights over a ground sphere: no shared slab, node
    boxes of different y extents."""
    rng = np.random.default_rng(83)
    rows = [((0, -1000, 0), 1000.0, (0.5, 0.5, 0.5), 1, 0.9)]
    for i in range(120):
        r = float(rng.choice([0.15, 0.25, 0.4]))
        c = (float(rng.uniform(-6, 6)), float(rng.uniform(r, 7.0)), float(rng.uniform(-6, 6)))
        rows.append((c, r, tuple(rng.uniform(0.2, 1, 3)), 1 + i % 3, float(rng.uniform(0, 1.6))))
    return vc.make_spheres(rows)


def many_groups_scene():
    """700 small spheres at one height on a jittered grid: 176 hierarchy groups, 22 nodes -- past
    16-bit node masks, within the LDS-table kernel's 256 groups."""
    rng = np.random.default_rng(84)
    rows = [((0, -1000, 0), 1000.0, (0.5, 0.5, 0.5), 1, 0.9)]
    for i in range(700):
        c = (0.55 * (i % 28) - 7.4 + float(rng.uniform(-0.1, 0.1)), 0.15,
             0.55 * (i // 28) - 6.6 + float(rng.uniform(-0.1, 0.1)))
        rows.append((c, 0.15, tuple(rng.uniform(0.2, 1, 3)), 1 + i % 3,
                     float(rng.uniform(0, 1.6))))
    return vc.make_spheres(rows)


def tiny_scene():
    """test_gpu_slab.py's one-height scene scaled by 2^-24: its largest box coordinate is below
    the 2^-20 the footprint's proof needs, so the host gives all-ones masks."""
    from tests.test_gpu_slab import one_height_scene
    sp = one_height_scene()
    sp["center"] *= f32(2.0 ** -24)
    sp["radius"] *= f32(2.0 ** -24)
    return sp


def node_boxes(t):
    """lo [nodes, 3], hi [nodes, 3], K [nodes], real [nodes] (has members) of t["node"]."""
    b = t["node"]
    n = 2 * b.shape[0]
    cols = lambda k: np.stack([b[:, k], b[:, k + 1]], 1).reshape(n)  # noqa: E731
    lo = np.stack([cols(0), cols(2), cols(4)], 1)
    hi = np.stack([cols(6), cols(8), cols(10)], 1)
    return lo, hi, cols(12), lo[:, 0] != f32(1e20)


def y_interval(br, ylo, yhi):
    """box_ray's slab interval (t0 clamped at 0, t1) of the y extent [ylo, yhi]."""
    inv, c = br[0], br[1]
    n = len(inv)
    tly = fma(np.full(n, ylo, f32), inv[:, 1], c[:, 1])
    thy = fma(np.full(n, yhi, f32), inv[:, 1], c[:, 1])
    return np.maximum(np.minimum(tly, thy), f32(0)), np.maximum(tly, thy)


def node_keep(t, br, slab=None):
    """[rays, nodes] bool: the node box test keeps the node (gap >= 0), three-axis form, or the
    slab form (fact (3a)) with slab = (lo.y, hi.y)."""
    lo, hi, K, _ = node_boxes(t)
    inv, c, c1, c2 = br
    tn = tf = None
    for k in ((0, 2) if slab is not None else (0, 1, 2)):
        tl = fma(lo[None, :, k], inv[:, k, None], c[:, k, None])
        th = fma(hi[None, :, k], inv[:, k, None], c[:, k, None])
        near, far = np.minimum(tl, th), np.maximum(tl, th)
        tn = near if tn is None else np.maximum(tn, near)
        tf = far if tf is None else np.minimum(tf, far)
    if slab is not None:
        t0, t1 = y_interval(br, slab[0], slab[1])
        tn, tf = np.maximum(tn, t0[:, None]), np.minimum(tf, t1[:, None])
    else:
        tn = np.maximum(tn, f32(0))
    with np.errstate(over="ignore", invalid="ignore"):
        gap = fma(np.broadcast_to(K[None, :], tn.shape), np.broadcast_to(c2[:, None], tn.shape),
                  rn(rn(tf - tn) + c1[:, None]))
    return ~(gap < 0)


def cell(x, so, n):
    """The kernel's cell of coordinate x (fp32): trunc(med3(fma(x, scale, offset), 0, n - 1))."""
    x = np.asarray(x, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        f = fma(x, np.full(x.shape, so[0], f32), np.full(x.shape, so[1], f32))
    return np.clip(f, f32(0), f32(n - 1)).astype(np.int64)


def foot_mask(fp, br, d, y, s_scale=1.0, parts=False):
    """[rays] node masks as tracer.hip foot_mask computes them: y = the y extent whose interval
    the ray takes (the slab's, or fp["y"]); s_scale scales S for the checker's own test."""
    inv, c, c1, c2 = br
    n = fp["tables"].shape[1]
    t0, t1 = y_interval(br, y[0], y[1])
    with np.errstate(over="ignore", invalid="ignore"):
        S_ = rn(fma(np.full(len(c1), fp["k2"], f32), c2, rn(c1 + c1)).astype(np.float64) * s_scale)
        ta, tb = rn(t0 - S_), rn(t1 + S_)
        dd = np.where(np.abs(d) < f32(2.0 ** -40), np.copysign(f32(2.0 ** -40), d), d).astype(f32)
        xa, xb = rn(rn(ta - c[:, 0]) * dd[:, 0]), rn(rn(tb - c[:, 0]) * dd[:, 0])
        za, zb = rn(rn(ta - c[:, 2]) * dd[:, 2]), rn(rn(tb - c[:, 2]) * dd[:, 2])
    assert not (np.isnan(xa) | np.isnan(xb) | np.isnan(za) | np.isnan(zb)).any()
    ixa, ixb, iza, izb = cell(xa, fp["x"], n), cell(xb, fp["x"], n), cell(za, fp["z"], n), \
        cell(zb, fp["z"], n)
    x0, x1 = np.minimum(ixa, ixb), np.maximum(ixa, ixb)
    z0, z1 = np.minimum(iza, izb), np.maximum(iza, izb)
    T = fp["tables"]
    m = T[0][x1] & T[1][x0] & T[2][z1] & T[3][z0]
    m = np.where(tb < ta, np.uint32(0), m) | np.uint32(fp["always"])
    if parts:
        return m, (np.minimum(xa, xb), np.maximum(xa, xb), np.minimum(za, zb),
                   np.maximum(za, zb), tb < ta)
    return m


def key_of(x):
    b = np.asarray(x, f32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0x7fffffff - (b & 0x7fffffff), 0x80000000 + b)


def float_of(k):
    k = np.asarray(k, np.int64)
    b = np.where(k >= 0x80000000, k - 0x80000000, 0x80000000 | (0x7fffffff - k))
    return b.astype(np.uint32).view(f32)


def build_tables(lo, hi, real, so_x, so_z, n):
    """cluster.cpp's tables from node boxes (lo, hi [nodes, 3]) and the cells' (scale, offset),
    in float64: per cell the largest float ue and (one float below) the smallest float le that the
    kernel's own cell function puts there, then A = {lo <= ue + g}, B = {hi >= le - g}."""
    out = np.zeros((4, n), np.uint32)
    bits = np.where(real, np.uint32(1) << np.arange(len(lo), dtype=np.uint32), 0).astype(np.uint32)
    for a, so in ((0, so_x), (2, so_z)):
        i = np.arange(n - 1)
        lo_k = np.full(n - 1, key_of(f32(-np.inf)))
        hi_k = np.full(n - 1, key_of(f32(np.inf)))
        while (hi_k - lo_k > 1).any():
            mid = lo_k + (hi_k - lo_k) // 2
            below = cell(float_of(mid), so, n) <= i
            lo_k, hi_k = np.where(below, mid, lo_k), np.where(below, hi_k, mid)
        ue = np.concatenate([float_of(lo_k).astype(np.float64), [np.inf]])
        le = np.concatenate([[-np.inf], ue[:-1]])
        up = ue + (8.0 * 2.0 ** -24 * np.abs(ue) + 2.0 ** -100)
        dn = le - (8.0 * 2.0 ** -24 * np.abs(le) + 2.0 ** -100)
        A = (lo[None, :, a].astype(np.float64) <= up[:, None])
        B = (hi[None, :, a].astype(np.float64) >= dn[:, None])
        t = 0 if a == 0 else 2
        out[t] = (A * bits[None, :]).sum(1).astype(np.uint32)
        out[t + 1] = (B * bits[None, :]).sum(1).astype(np.uint32)
    return out


def scene_tables(sp):
    """(cull tables, footprint tables, slab or None) of a scene."""
    return S.cull_tables(sp), S.cull_footprint(sp), S.cull_slab(sp)
