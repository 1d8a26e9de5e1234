"""Chooses the defaults of the variance-guided chain on the CPU (no GPU), and scores it against the
chain the project had before it. The frames are tools/reproject_defaults.py's: an orbit of eight
views, 3 degrees apart, of the final scene at 64 x 36, depth 10, each rendered by the C oracle at
4 spp; the reprojection maps from tests/motion_ref and the guide buffers from tests/features_ref.
The new chain -- vcrt_reproject_moments_host over the eight frames, vcrt_variance_host and
vcrt_denoise_variance_host on the last -- runs over a grid of alpha x alpha_moments x min_history
x sigma_colour (everything else at the defaults of vcrt_reproject and vcrt_denoise), and the last
output is scored against the last view's 256-spp frame by its mean squared error. On the same
frames and guides today's chain, vcrt_reproject_host -> vcrt_denoise_host, both at their own
defaults, is scored the same way. Writes the grid, every point's error, both scores and the choice
to profiles/variance_defaults.json; csrc/variance.cpp carries the chosen values. The comparison is
not tuned: whichever chain scores lower, the file says so.

    python tools/variance_defaults.py
"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import vulkancomputeraytracing_amd as vc  # noqa: E402
from reproject_defaults import (CLEAN_SPP, DEGREES, DEPTH, H, SPP, STEPS, W, mse, orbit,  # noqa: E402
                                render)
from tests import features_ref as FR  # noqa: E402
from tests import motion_ref as M  # noqa: E402
from tests import oracle_py  # noqa: E402

GRID = {
    "alpha": [0.1, 0.2, 0.4, 0.6],
    "alpha_moments": [0.1, 0.2, 0.5],
    "min_history": [2.0, 4.0, 8.0],
    "sigma_colour": [1.0, 2.0, 4.0, 8.0],
}


def new_chain(frames, maps, guides, alpha, alpha_moments, min_history, sigma_colour):
    """(the denoised last output, the accumulated last output)."""
    zeros = np.zeros_like(frames[0])
    out, length, mom = zeros, np.zeros(zeros.shape[:2], np.float32), zeros
    for k in range(len(frames)):
        out, length, mom = vc.reproject_moments_host(
            frames[k], maps[k]["motion"], out, maps[k - 1]["surface"] if k else zeros, length,
            mom, albedo=guides[k]["albedo"], alpha=alpha, alpha_moments=alpha_moments)
    var = vc.variance_host(mom, maps[-1]["surface"], min_history=min_history, alpha=alpha)
    clean, _ = vc.denoise_variance_host(out, var, guides[-1]["albedo"],
                                        guides[-1]["normal_depth"], sigma_colour=sigma_colour)
    return clean, out


def old_chain(frames, maps, guides):
    out, length = frames[0], np.ones(frames[0].shape[:2], np.float32)
    for k in range(1, len(frames)):
        out, length = vc.reproject_host(frames[k], maps[k]["motion"], out,
                                        maps[k - 1]["surface"], length)
    return vc.denoise_host(out, guides[-1]["albedo"], guides[-1]["normal_depth"]), out


def main():
    o = oracle_py.load()
    scene = o.scene("final")
    base = vc.RenderDesc(width=W, height=H, samples_per_pixel=SPP, max_depth=DEPTH)
    descs = [orbit(base, DEGREES * k) for k in range(STEPS)]
    frames = [render(o, scene, d, SPP) for d in descs]
    clean = render(o, scene, descs[-1], CLEAN_SPP)
    maps = [M.frame_motion(o, scene, d, descs[k - 1] if k else None)
            for k, d in enumerate(descs)]
    guides = [FR.frame_features(o, scene, d, 0, SPP) for d in descs]
    names = list(GRID)
    points = []
    for values in itertools.product(*GRID.values()):
        p = dict(zip(names, values))
        den, acc = new_chain(frames, maps, guides, **p)
        points.append({**p, "mse": mse(den, clean), "mse_accumulated": mse(acc, clean)})
    points.sort(key=lambda r: r["mse"])
    chosen = {k: points[0][k] for k in names}
    old_den, old_acc = old_chain(frames, maps, guides)
    out = {
        "what": "mean squared error over rgb of the last of eight 4-spp frames, accumulated and "
                "denoised, against the last view's 256-spp frame; final scene, 64 x 36, depth 10, "
                "an orbit of 3 degrees a step; C oracle frames, motion_ref maps, features_ref "
                "guides, the _host functions",
        "grid": GRID,
        "fixed": {"reproject": {k: v for k, v in vc.default_reproject_params().items()
                                if k != "alpha"},
                  "denoise": {k: v for k, v in vc.default_denoise_params().items()
                              if k != "sigma_colour"}},
        "mse_unaccumulated": mse(frames[-1], clean),
        "today": {"chain": "reproject -> denoise, both at their defaults",
                  "reproject": vc.default_reproject_params(),
                  "denoise": vc.default_denoise_params(),
                  "mse_accumulated": mse(old_acc, clean), "mse": mse(old_den, clean)},
        "chosen": chosen,
        "mse_chosen": points[0]["mse"],
        "new_chain_scores_lower": points[0]["mse"] < mse(old_den, clean),
        "points": points,
    }
    path = os.path.join(ROOT, "profiles", "variance_defaults.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("mse_unaccumulated", "today", "chosen", "mse_chosen",
                                          "new_chain_scores_lower")}))
    for r in points[:10]:
        print(r)


if __name__ == "__main__":
    main()
