"""Node entries per bounce segment of the final scene's 1080p camera under three node-level
tests of the LDS-table flat scan: the line test (the node box test of tracer.hip facts (3)/(4)),
the exact rectangle (the xz bounding rectangle of the line's stretch inside the node boxes' y
extent against each node's xz rectangle) and the footprint tables (fact (5)) with N cells per
axis. Statistics only: float64 paths with approximate scattering (as cull_potential.py) over the
real tables of csrc/cluster.cpp (scene.cull_tables); the tables for N cells are built by the
host's rule (tests/footprint_ref.py build_tables) and at the host's own N equal
scene.cull_footprint's.

  python tools/sim/footprint_nodes.py [paths, default 3000]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import footprint_ref as F  # noqa: E402
from tests import oracle_py  # noqa: E402
from vulkancomputeraytracing_amd import scene as S  # noqa: E402

f32 = np.float32
o = oracle_py.load()
SC = o.scene("final")
C = SC["center"].astype(np.float64)
R = SC["radius"].astype(np.float64)
TYP = SC["texture"][:, 0].astype(int)
PAR = SC["texture"][:, 1].astype(np.float64)
W, H = 1920, 1080
cam = o.camera(o.config(W, H, 1, 10)).astype(np.float64)
p00, du, dv, ctr = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
rng = np.random.default_rng(1)


def hit(o_, d_):
    oc = o_[None, :] - C
    a = d_ @ d_
    hb = oc @ d_
    cc = (oc * oc).sum(1) - R * R
    disc = hb * hb - a * cc
    best, bt = -1, 1e5
    for j in np.nonzero(disc >= 0)[0]:
        sq = np.sqrt(disc[j])
        for t in ((-hb[j] - sq) / a, (-hb[j] + sq) / a):
            if 0.001 < t < bt:
                bt, best = t, j
                break
    return best, bt


def bounce_segments(x, y):
    jx, jy = rng.uniform(-0.5, 0.5, 2)
    d = (p00 + x * du + y * dv + jx * du + jy * dv) - ctr
    org = ctr.copy()
    segs = []
    for depth in range(10):
        if depth > 0:
            segs.append((org.copy(), d.copy()))
        j, t = hit(org, d)
        if j < 0:
            break
        p = org + t * d
        n = (p - C[j]) / R[j]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if TYP[j] == 1:
            d = n + u
        elif TYP[j] == 2:
            d = d - 2 * (n @ d) * n + PAR[j] * u
        else:
            d = d - 2 * (n @ d) * n if rng.uniform() < 0.5 else d  # crude glass
        org = p
    return segs


def main():
    paths = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    sp = S.builtin_scene("final")
    t, fp = S.cull_tables(sp), S.cull_footprint(sp)
    lo, hi, _, real = F.node_boxes(t)
    lo, hi = lo[real].astype(np.float64), hi[real].astype(np.float64)
    ylo, yhi = lo[:, 1].min(), hi[:, 1].max()
    segs = []
    for _ in range(paths):
        segs += bounce_segments(rng.integers(0, W), rng.integers(0, H))
    O = np.array([s[0] for s in segs])
    D = np.array([s[1] for s in segs])
    D = np.where(np.abs(D) < 1e-12, 1e-12, D)
    inv = 1.0 / D

    def planes(a, l, h):  # near, far parameters of [l, h] on axis a: [segments, boxes]
        tl, th = (l[None, :] - O[:, a, None]) * inv[:, a, None], \
            (h[None, :] - O[:, a, None]) * inv[:, a, None]
        return np.minimum(tl, th), np.maximum(tl, th)

    nx, fx = planes(0, lo[:, 0], hi[:, 0])
    ny, fy = planes(1, lo[:, 1], hi[:, 1])
    nz, fz = planes(2, lo[:, 2], hi[:, 2])
    line = np.maximum(np.maximum(np.maximum(nx, ny), nz), 0.0) <= np.minimum(np.minimum(fx, fy), fz)
    # the stretch inside the y extent, from the origin on
    n0, f0 = planes(1, np.array([ylo]), np.array([yhi]))
    t0, t1 = np.maximum(n0[:, 0], 0.0), f0[:, 0]
    empty = t1 < t0
    xa, xb = O[:, 0] + t0 * D[:, 0], O[:, 0] + t1 * D[:, 0]
    za, zb = O[:, 2] + t0 * D[:, 2], O[:, 2] + t1 * D[:, 2]
    x0, x1, z0, z1 = np.minimum(xa, xb), np.maximum(xa, xb), np.minimum(za, zb), np.maximum(za, zb)
    rect = (lo[None, :, 0] <= x1[:, None]) & (hi[None, :, 0] >= x0[:, None]) & \
        (lo[None, :, 2] <= z1[:, None]) & (hi[None, :, 2] >= z0[:, None]) & ~empty[:, None]
    assert not (line & ~rect).any()
    n = len(segs)
    ext = np.maximum(x1 - x0, z1 - z0)[~empty]
    print(f"{paths} camera paths, {n} bounce segments, {len(lo)} nodes; "
          f"{100 * empty.mean():.1f} % never reach the y extent; xz extent of the stretch: "
          f"median {np.median(ext):.2f}, p75 {np.percentile(ext, 75):.2f}, "
          f"p90 {np.percentile(ext, 90):.2f}, p95 {np.percentile(ext, 95):.2f}")
    print(f"line test {line.sum() / n:.3f} node entries per bounce segment "
          f"({100 * line.any(1).mean():.0f} % enter a node); exact rectangle {rect.sum() / n:.3f}")
    lo32, hi32, _, real32 = F.node_boxes(t)
    host_n = fp["tables"].shape[1]
    for N in sorted({32, 64, host_n, 128, 256}):
        so = {}
        for a, key in ((0, "x"), (2, "z")):
            w = float(hi[:, a].max()) - float(lo[:, a].min())
            s = f32(N / w)
            so[key] = np.array([s, f32(-float(lo[:, a].min()) * float(s))], f32)
        tabs = F.build_tables(lo32, hi32, real32, so["x"], so["z"], N)
        if N == host_n:
            assert np.array_equal(tabs, fp["tables"])
        cx0, cx1 = F.cell(x0.astype(f32), so["x"], N), F.cell(x1.astype(f32), so["x"], N)
        cz0, cz1 = F.cell(z0.astype(f32), so["z"], N), F.cell(z1.astype(f32), so["z"], N)
        m = tabs[0][cx1] & tabs[1][cx0] & tabs[2][cz1] & tabs[3][cz0]
        m = np.where(empty, 0, m)
        bits = sum(((m >> k) & 1).sum() for k in range(32))
        print(f"N = {N:3d}{' (host)' if N == host_n else '       '}: {bits / n:.3f} node entries per "
              f"bounce segment, {bits / line.sum():.3f} x the line test; "
              f"{4 * N * 2} B of 16-bit masks")


if __name__ == "__main__":
    main()
