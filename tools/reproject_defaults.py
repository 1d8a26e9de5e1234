"""Chooses vcrt_default_reproject_params' numbers on the CPU (no GPU): an orbit of eight views,
3 degrees apart, of the final scene at 64 x 36, depth 10, each rendered by the C oracle at 4 spp;
the reprojection maps from tests/motion_ref; the frames accumulated with vcrt_reproject_host over
a grid of alpha x depth_tolerance (max_history above the step count, so that it never binds); and
the last output scored against the last view's 256-spp frame. The grid point with the smallest
mean squared error becomes the default. Writes the grid, every point's error, the unaccumulated
frame's error and the choice to profiles/reproject_defaults.json; csrc/reproject.cpp and
tests/reproject_ref.DEFAULTS carry the chosen values.

    python tools/reproject_defaults.py
"""
import itertools
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vulkancomputeraytracing_amd as vc  # noqa: E402
from tests import motion_ref as M  # noqa: E402
from tests import oracle_py  # noqa: E402

W, H, DEPTH, SPP, CLEAN_SPP = 64, 36, 10, 4, 256
STEPS, DEGREES = 8, 3.0
GRID = {
    "alpha": [0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9],
    "depth_tolerance": [0.0, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2],
}
FIXED = dict(max_history=32.0)  # >= STEPS: the cap is not what is searched


def mse(a, b):
    return float(((a[..., :3].astype(np.float64) - b[..., :3]) ** 2).mean())


def orbit(desc, degrees):
    th = math.radians(degrees)
    dx, dz = desc.lookfrom[0] - desc.lookat[0], desc.lookfrom[2] - desc.lookat[2]
    return desc.with_camera(lookfrom=(
        float(np.float32(desc.lookat[0] + dx * math.cos(th) + dz * math.sin(th))),
        desc.lookfrom[1],
        float(np.float32(desc.lookat[2] - dx * math.sin(th) + dz * math.cos(th)))))


def render(o, scene, d, spp):
    img, _ = o.render(o.config(d.width, d.height, spp, d.max_depth, d.lookfrom, d.lookat, d.vup,
                               d.vfov), scene)
    return img


def accumulate(frames, maps, **params):
    """(the last output, the share of pixels that accepted history in the last step)."""
    out, length = frames[0], np.ones(frames[0].shape[:2], np.float32)
    for k in range(1, len(frames)):
        out, length = vc.reproject_host(frames[k], maps[k]["motion"], out, maps[k - 1]["surface"],
                                        length, **params)
    return out, float((length > 1).mean())


def main():
    o = oracle_py.load()
    scene = o.scene("final")
    base = vc.RenderDesc(width=W, height=H, samples_per_pixel=SPP, max_depth=DEPTH)
    descs = [orbit(base, DEGREES * k) for k in range(STEPS)]
    frames = [render(o, scene, d, SPP) for d in descs]
    clean = render(o, scene, descs[-1], CLEAN_SPP)
    maps = [M.frame_motion(o, scene, d, descs[k - 1] if k else None)
            for k, d in enumerate(descs)]
    names = list(GRID)
    points = []
    for values in itertools.product(*GRID.values()):
        p = {**FIXED, **dict(zip(names, values))}
        out, accepted = accumulate(frames, maps, **p)
        points.append({**p, "mse": mse(out, clean), "accepted_last_step": accepted})
    points.sort(key=lambda r: r["mse"])
    chosen = {k: points[0][k] for k in names + list(FIXED)}
    out = {
        "what": "mean squared error over rgb of the last of eight accumulated 4-spp frames "
                "against the last view's 256-spp frame; final scene, 64 x 36, depth 10, an orbit "
                "of 3 degrees a step; C oracle frames, motion_ref maps, vcrt_reproject_host",
        "grid": GRID,
        "fixed": FIXED,
        "mse_unaccumulated": mse(frames[-1], clean),
        "chosen": chosen,
        "mse_chosen": points[0]["mse"],
        "points": points,
    }
    path = os.path.join(ROOT, "profiles", "reproject_defaults.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("mse_unaccumulated", "chosen", "mse_chosen")}))
    for r in points[:10]:
        print(r)


if __name__ == "__main__":
    main()
