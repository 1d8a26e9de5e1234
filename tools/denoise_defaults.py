"""Chooses vcrt_default_denoise_params' numbers on the CPU (no GPU): the final scene at 64 x 36,
depth 10, rendered by the C oracle at 4 spp and at 256 spp, the 4-sample guides from
tests/features_ref, and the grid point whose denoised 4-spp frame (vcrt_denoise_host) has the
smallest mean squared error against the 256-spp frame. Writes the grid, every point's error and
the choice to profiles/denoise_defaults.json; csrc/denoise.cpp and tests/denoise_ref.DEFAULTS
carry the chosen values.

    python tools/denoise_defaults.py
"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vulkancomputeraytracing_amd as vc  # noqa: E402
from tests import features_ref as FR  # noqa: E402
from tests import oracle_py  # noqa: E402

W, H, DEPTH, SPP, CLEAN_SPP = 64, 36, 10, 4, 256
# The sigmas' grid. Every guide term stays on (the guides are what the filter is for); the colour
# term may be off, as at the starting point. levels and demodulate are not searched: a 64 x 36
# frame of this scene has spheres a pixel or two wide, so its error only says "filter less" about
# the pass count, while the frames the filter is for (1080p) hold the same features 30 times
# larger. The sweeps over them at the chosen sigmas are recorded for information.
GRID = {
    "sigma_normal": [0.25, 0.5, 1.0],
    "sigma_depth": [0.025, 0.05, 0.1, 0.2],
    "sigma_albedo": [0.125, 0.25, 0.5],
    "sigma_colour": [0.0, 0.5, 0.75, 1.0, 2.0],
}
FIXED = dict(levels=5, demodulate=1)
START = dict(levels=5, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=0.25, sigma_colour=0.0,
             demodulate=1)


def mse(a, b):
    return float(((a[..., :3].astype(np.float64) - b[..., :3]) ** 2).mean())


def main():
    o = oracle_py.load()
    scene = o.scene("final")
    noisy, _ = o.render(o.config(W, H, SPP, DEPTH), scene)
    clean, _ = o.render(o.config(W, H, CLEAN_SPP, DEPTH), scene)
    desc = vc.RenderDesc(width=W, height=H, samples_per_pixel=SPP, max_depth=DEPTH)
    g = FR.frame_features(o, scene, desc, 0, SPP)
    names = list(GRID)
    points = []
    for values in itertools.product(*GRID.values()):
        p = {**FIXED, **dict(zip(names, values))}
        den = vc.denoise_host(noisy, g["albedo"], g["normal_depth"], **p)
        points.append({**p, "mse": mse(den, clean)})
    points.sort(key=lambda r: r["mse"])
    chosen = {k: points[0][k] for k in list(FIXED) + names}

    def error_with(**change):
        p = {**chosen, **change}
        return {**p, "mse": mse(vc.denoise_host(noisy, g["albedo"], g["normal_depth"], **p), clean)}

    start = vc.denoise_host(noisy, g["albedo"], g["normal_depth"], **START)
    out = {
        "what": "mean squared error over rgb of the denoised 4-spp frame against the 256-spp "
                "frame; final scene, 64 x 36, depth 10; C oracle frames, features_ref guides, "
                "vcrt_denoise_host",
        "grid": GRID,
        "fixed": FIXED,
        "mse_noisy": mse(noisy, clean),
        "starting_point": {**START, "mse": mse(start, clean)},
        "chosen": chosen,
        "mse_chosen": points[0]["mse"],
        "levels_sweep_at_chosen": [error_with(levels=n) for n in range(1, 9)],
        "demodulate_0_at_chosen": error_with(demodulate=0),
        "points": points,
    }
    path = os.path.join(ROOT, "profiles", "denoise_defaults.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("mse_noisy", "starting_point", "chosen", "mse_chosen")}))
    for r in points[:8]:
        print(r)


if __name__ == "__main__":
    main()
