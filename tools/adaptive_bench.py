"""Adaptive sampling (Renderer.draw_samples) against the routes a caller had before, and its
quality against a uniform frame of the same budget. Writes profiles/adaptive.json.

Speed, on one GPU, for each workload (1080p final scene; 4K with 4100 spheres), in one process:
  (i)  a uniform count plane of 16: scan_ms, kernel_ms, resolve_ms of draw_samples on device
       tensors, against
         * the 16-spp frame's kernel_ms in the same run, and
         * the route before: the same rays (frame_rays, the pixels in 8 x 8 tiles, a pixel's
           samples adjacent) uploaded once and traced by trace_rays on device tensors at the
           frame's depth, kernel_ms only; the upload (24 B per ray) is timed separately;
  (ii) a skewed plane of the same total (to a few samples): the per-sample luminance variance
       estimated from two uniform rounds of 4 (vcrt_render --adaptive's estimator) through
       sample_counts with max_count 256, its target bisected to the total. The route before gets
       this plane's rays, grouped by count.
Every measurement is warmed up and reported as the minimum and the median over its runs. The
condition the feature is held to: on (i) and (ii) the fused call's kernel_ms is below
trace_rays' for the same rays ("fused_below_trace_rays"); its ratio to the frame kernel is recorded.

Quality, at 64 x 36 and depth 10 on the eight views of tools/variance_defaults.py: the mean squared
error against a 256-spp frame of (a) a uniform frame of B samples per pixel and (b) the adaptive
loop at the same total: two uniform rounds of 4, then sample_counts with max_count 64 and the
target bisected so that the third round averages B - 8 per pixel. Both are recorded with the
chosen targets; neither is tuned.

    python tools/adaptive_bench.py --out profiles/adaptive.json
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.environ.get("VCRT_PKG_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import vulkancomputeraytracing_amd as vc  # noqa: E402

WORKLOADS = {
    "1080p_final": dict(width=1920, height=1080, scene="final"),
    "4k_stress4096": dict(width=3840, height=2160, scene="stress4096"),
}
SPP = 16
F = np.float32


def tile_order_pixels(width, height):
    y, x = np.mgrid[0:height, 0:width]
    x, y = x.ravel(), y.ravel()
    key = np.lexsort((x % 8, y % 8, x // 8, y // 8))
    return np.stack([x[key], y[key]], axis=1).astype(np.int32)


def spread(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms), "runs": len(ms)}


def lum(c):
    y = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]).astype(F)
    return (y + F(0.0722) * c[..., 2]).astype(F)


def estimate_variance(r, n0):
    """vcrt_render --adaptive's estimator after two uniform rounds of n0: (variance, sums)."""
    h, w = r.desc.height, r.desc.width
    uniform = np.full((h, w), n0, np.uint16)
    a = r.draw_samples(uniform, first=0, max_count=n0)
    m1 = a["mean"]
    b = r.draw_samples(uniform, first=n0, max_count=n0, sums=a["sums"])
    d = (lum(b["mean"]) - lum(m1)).astype(F)
    return ((d * d).astype(F) * F(2 * n0)).astype(F), b["sums"]


def counts_for_total(var, total, max_count):
    """sample_counts_host with the target bisected (in log space) to the total: (counts, target,
    the total reached)."""
    lo, hi = 1e-6, 1e3  # targets: lo gives the most samples
    for _ in range(60):
        mid = (lo * hi) ** 0.5
        _, got = vc.sample_counts_host(var, mid, 0, max_count, stats=True)
        if got > total:
            lo = mid
        else:
            hi = mid
    counts, got = vc.sample_counts_host(var, hi, 0, max_count, stats=True)
    return counts, hi, got


def rays_of_plane(desc, xy, counts):
    """The plane's rays as trace_rays takes them: grouped by count, inside a group the pixels in
    xy's order and a pixel's samples adjacent."""
    c = counts[xy[:, 1], xy[:, 0]]
    origins, dirs = [], []
    for n in np.unique(c):
        if n == 0:
            continue
        o, d = vc.frame_rays(desc, xy[c == n], 0, int(n))
        origins.append(o.reshape(-1, 3))
        dirs.append(d.reshape(-1, 3))
    return np.concatenate(origins), np.concatenate(dirs)


def time_plane(r, desc, xy, counts, a, dev):
    import torch
    res = {"samples": int(counts.astype(np.int64).sum()),
           "max_count_in_plane": int(counts.max()),
           "pixels_with_samples": int((counts > 0).sum())}
    dc = torch.from_numpy(counts.astype(np.int16)).to(dev)
    acc = {k: [] for k in ("scan_ms", "kernel_ms", "resolve_ms", "host_ms")}
    for i in range(a.warmup + a.runs):
        out = r.draw_samples(dc, first=0, max_count=256, stats=True)
        if i >= a.warmup:
            for k in acc:
                acc[k].append(out["stats"][k])
    st = out["stats"]
    res["draw_samples"] = {k: spread(v) for k, v in acc.items()}
    res["draw_samples"].update({k: st[k] for k in ("items", "segments", "listed_rays",
                                                   "group_tests", "bound_tests")})
    # the route before: the same rays, uploaded once (timed), traced by trace_rays
    t0 = time.perf_counter()
    o, d = rays_of_plane(desc, xy, counts)
    res["frame_rays_host_ms"] = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.cuda.synchronize(dev)
    res["upload_ms"] = (time.perf_counter() - t0) * 1e3
    res["upload_bytes"] = int(o.nbytes + d.nbytes)
    del o, d
    ms = []
    for i in range(a.warmup + a.runs):
        _, st = r.trace_rays(to, td, max_depth=desc.max_depth, stats=True)
        if i >= a.warmup:
            ms.append(st["kernel_ms"])
    res["trace_rays"] = {"kernel_ms": spread(ms), "rays": int(to.shape[0]),
                         "segments": st["segments"]}
    del to, td
    fused = res["draw_samples"]["kernel_ms"]["median"]
    res["fused_over_trace_rays"] = fused / res["trace_rays"]["kernel_ms"]["median"]
    res["fused_below_trace_rays"] = bool(fused < res["trace_rays"]["kernel_ms"]["median"])
    res["same_segments"] = bool(res["draw_samples"]["segments"] == res["trace_rays"]["segments"])
    return res


def run_workload(w, a):
    import torch
    dev = torch.device("cuda", 0)
    desc = vc.RenderDesc(width=w["width"], height=w["height"], samples_per_pixel=SPP,
                         max_depth=a.depth, device=0)
    xy = tile_order_pixels(w["width"], w["height"])
    res = {"workload": dict(w, frame_spp=SPP, depth=a.depth, pixels=len(xy))}
    with vc.Renderer(desc, w["scene"]) as r:
        frame_ms = []
        for i in range(a.warmup + a.runs):
            r.draw_next_frame()
            st = r.stats()
            if i >= a.warmup:
                frame_ms.append(st["kernel_ms"])
        res["frame_16spp"] = {"kernel": st["kernel"], "kernel_ms": spread(frame_ms),
                              "segments": st["segments"]}
        uniform = np.full((w["height"], w["width"]), SPP, np.uint16)
        res["uniform16"] = time_plane(r, desc, xy, uniform, a, dev)
        var, _ = estimate_variance(r, 4)
        counts, target, got = counts_for_total(var, SPP * len(xy), 256)
        res["skewed"] = time_plane(r, desc, xy, counts, a, dev)
        res["skewed"].update(target=target, wanted_samples=SPP * len(xy),
                             share_of_pixels_at_max=float((counts == 256).mean()),
                             share_of_pixels_at_zero=float((counts == 0).mean()))
        for k in ("uniform16", "skewed"):
            res[k]["fused_over_frame_kernel_per_sample"] = (
                res[k]["draw_samples"]["kernel_ms"]["median"] / res[k]["samples"] /
                (res["frame_16spp"]["kernel_ms"]["median"] / (SPP * len(xy))))
    return res


def quality(a):
    from reproject_defaults import DEGREES, DEPTH, H, STEPS, W, mse, orbit
    base = vc.RenderDesc(width=W, height=H, samples_per_pixel=a.budget, max_depth=DEPTH, device=0)
    n0, views = 4, []
    for k in range(STEPS):
        d = orbit(base, DEGREES * k)
        with vc.Renderer(dataclasses.replace(d, samples_per_pixel=256), "final") as r:
            r.draw_next_frame()
            clean = r.read_framebuffer()
        with vc.Renderer(d, "final") as r:
            r.draw_next_frame()
            uniform = r.read_framebuffer()
            var, sums = estimate_variance(r, n0)
            counts, target, got = counts_for_total(var, (a.budget - 2 * n0) * W * H, 64)
            out = r.draw_samples(counts, first=2 * n0, max_count=64, sums=sums)
        views.append({"degrees": DEGREES * k, "target": target,
                      "adaptive_samples_per_pixel": 2 * n0 + got / (W * H),
                      "mse_uniform": mse(uniform, clean), "mse_adaptive": mse(out["mean"], clean)})
    mu = statistics.mean(v["mse_uniform"] for v in views)
    ma = statistics.mean(v["mse_adaptive"] for v in views)
    return {"what": f"mean squared error over rgb against a 256-spp frame; final scene, {W} x {H}, "
                    f"depth {DEPTH}, {STEPS} views {DEGREES} degrees apart; uniform: a frame of "
                    f"{a.budget} spp; adaptive: two uniform rounds of {n0}, then sample_counts "
                    "(max_count 64, target bisected to the budget) and one adaptive round. The "
                    "reference frame holds the sample indices 0 .. 255, which include the uniform "
                    "frame's and most of the adaptive run's: both errors are lower than against "
                    "an independent reference",
            "budget_spp": a.budget, "views": views, "mse_uniform": mu, "mse_adaptive": ma,
            "adaptive_over_uniform": ma / mu, "adaptive_scores_lower": bool(ma < mu)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workloads", nargs="*", default=list(WORKLOADS), choices=list(WORKLOADS))
    p.add_argument("--depth", type=int, default=50)
    p.add_argument("--runs", type=int, default=5, help="timed runs per measurement")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--budget", type=int, default=16, help="the quality runs' samples per pixel")
    p.add_argument("--no-quality", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adaptive_bench: no GPU (there is no CPU path to time)")
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup}
    if a.out and os.path.exists(a.out):  # workloads measured in separate runs share the file
        with open(a.out) as f:
            res = {**json.load(f), **res}
    for name in a.workloads:
        res[name] = run_workload(WORKLOADS[name], a)
    if not a.no_quality:
        res["quality"] = quality(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
