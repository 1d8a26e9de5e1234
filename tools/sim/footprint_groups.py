"""footprint_nodes.py extended to the group boxes: node and group entries per bounce segment of
the final scene's 1080p camera under the line test (the box test of tracer.hip facts (3)/(4)), the
exact rectangle (the xz bounding rectangle of the line's stretch inside the boxes' y extent
against each box's xz rectangle) and the footprint tables with N cells per axis, the host's own N
of each level included (facts (5) and (5g)); and, for the group level, the mean over random
64-segment "waves" of the busiest lane's group count (the trips of a push loop that every lane
leaves together). Statistics only: float64 paths with approximate scattering over the real tables
of csrc/cluster.cpp; the tables for N cells are built by the host's rule
(tests/footprint_ref.py, tests/group_footprint_ref.py build_tables) and at the host's own N equal
the host's.

  python tools/sim/footprint_groups.py [paths, default 3000]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import footprint_ref as F  # noqa: E402
from tests import group_footprint_ref as G  # noqa: E402
from tools.sim import footprint_nodes as FN  # noqa: E402
from vulkancomputeraytracing_amd import scene as S  # noqa: E402

f32 = np.float32


def busiest(counts, rng, waves=2000):
    """Mean over random 64-segment waves of the largest per-segment count."""
    idx = rng.integers(0, len(counts), (waves, 64))
    return float(counts[idx].max(1).mean())


def level(name, lo32, hi32, real32, host, build, O, D, rng, words):
    lo, hi = lo32[real32].astype(np.float64), hi32[real32].astype(np.float64)
    inv = 1.0 / D

    def planes(a, l, h):  # near, far parameters of [l, h] on axis a: [segments, boxes]
        tl, th = (l[None, :] - O[:, a, None]) * inv[:, a, None], \
            (h[None, :] - O[:, a, None]) * inv[:, a, None]
        return np.minimum(tl, th), np.maximum(tl, th)

    nx, fx = planes(0, lo[:, 0], hi[:, 0])
    ny, fy = planes(1, lo[:, 1], hi[:, 1])
    nz, fz = planes(2, lo[:, 2], hi[:, 2])
    line = np.maximum(np.maximum(np.maximum(nx, ny), nz), 0.0) <= np.minimum(np.minimum(fx, fy), fz)
    ylo, yhi = lo[:, 1].min(), hi[:, 1].max()
    n0, f0 = planes(1, np.array([ylo]), np.array([yhi]))
    t0, t1 = np.maximum(n0[:, 0], 0.0), f0[:, 0]
    empty = t1 < t0
    xa, xb = O[:, 0] + t0 * D[:, 0], O[:, 0] + t1 * D[:, 0]
    za, zb = O[:, 2] + t0 * D[:, 2], O[:, 2] + t1 * D[:, 2]
    x0, x1, z0, z1 = np.minimum(xa, xb), np.maximum(xa, xb), np.minimum(za, zb), np.maximum(za, zb)
    rect = (lo[None, :, 0] <= x1[:, None]) & (hi[None, :, 0] >= x0[:, None]) & \
        (lo[None, :, 2] <= z1[:, None]) & (hi[None, :, 2] >= z0[:, None]) & ~empty[:, None]
    assert not (line & ~rect).any()
    n = len(O)
    size = (hi - lo).mean(0)
    print(f"-- {name} level: {len(lo)} boxes of mean size {size[0]:.2f} x {size[2]:.2f} (x, z)")
    print(f"line test {line.sum() / n:.3f} {name} entries per bounce segment "
          f"({100 * line.any(1).mean():.0f} % enter one), busiest lane of 64: "
          f"{busiest(line.sum(1), rng):.1f}; exact rectangle {rect.sum() / n:.3f} "
          f"({rect.sum() / line.sum():.3f} x), busiest lane {busiest(rect.sum(1), rng):.1f}")
    host_n = host["tables"].shape[1]
    for N in sorted({32, 64, 84, host_n, 128, 256}):
        so = {}
        for a, key in ((0, "x"), (2, "z")):
            w = float(hi[:, a].max()) - float(lo[:, a].min())
            s = f32(N / w)
            so[key] = np.array([s, f32(-float(lo[:, a].min()) * float(s))], f32)
        tabs = build(lo32, hi32, real32, so["x"], so["z"], N)
        if N == host_n:
            assert np.array_equal(tabs, host["tables"])
        cx0, cx1 = F.cell(x0.astype(f32), so["x"], N), F.cell(x1.astype(f32), so["x"], N)
        cz0, cz1 = F.cell(z0.astype(f32), so["z"], N), F.cell(z1.astype(f32), so["z"], N)
        m = tabs[0][cx1] & tabs[1][cx0] & tabs[2][cz1] & tabs[3][cz0]
        m = m.reshape(n, -1).astype(np.uint32)
        m = np.where(empty[:, None], np.uint32(0), m)
        per = np.zeros(n, np.int64)
        for k in range(32):
            per += ((m >> np.uint32(k)) & np.uint32(1)).sum(1).astype(np.int64)
        has = G.mask_bits(np.pad(m, ((0, 0), (0, 4 - m.shape[1]))), len(lo32))[:, real32]
        assert not (line & ~has).any()  # no box the line test kept is missing
        print(f"N = {N:3d}{' (host)' if N == host_n else '       '}: {per.sum() / n:.3f} {name} "
              f"entries per bounce segment, {per.sum() / line.sum():.3f} x the line test, busiest "
              f"lane {busiest(per, rng):.1f}; {4 * N * words * 4 // (2 if words == 1 else 1)} B")


def main():
    paths = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    rng = np.random.default_rng(2)
    sp = S.builtin_scene("final")
    t, fp, gf = S.cull_tables(sp), S.cull_footprint(sp), S.cull_group_footprint(sp)
    segs = []
    for _ in range(paths):
        segs += FN.bounce_segments(FN.rng.integers(0, FN.W), FN.rng.integers(0, FN.H))
    O = np.array([s[0] for s in segs])
    D = np.array([s[1] for s in segs])
    D = np.where(np.abs(D) < 1e-12, 1e-12, D)
    print(f"{paths} camera paths, {len(segs)} bounce segments of the final scene's 1080p camera")
    lo, hi, _, real = F.node_boxes(t)
    level("node", lo, hi, real, fp, F.build_tables, O, D, rng, 1)
    lo, hi, _, real = G.group_boxes(t)
    print(f"group tables: host N = {gf['n']}, eligible {gf['eligible']}")
    level("group", lo, hi, real, gf, G.build_tables, O, D, rng, 4)


if __name__ == "__main__":
    main()
