"""Ray-query throughput against the frame path on the same rays.

Builds, on the host, the camera rays of a W x H frame at S samples per pixel (shader.comp:18-52
in float32: the rays the frame kernels generate), traces them through vcrt_trace_rays_device
(torch tensors) and reports segments per second from the call's kernel_ms: the median of
--launches launches after --warmup warm-ups. In the same process the frame path renders the
same scene, size, samples and depth with kernel_variant CULL_LANE (the same per-lane scan: the
gap is what the query's own parts cost -- ray loads, refill, stores, no LDS tables) and with the
default variant (what the flat scan would still buy); the CULL_LANE frames are also timed with
their tables left in global memory, where the query reads them. Prints one JSON object and,
with --out, writes it to a file (profiles/ray_query_bench.json).
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("VCRT_PKG_ROOT",
                                  os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402

import vulkancomputeraytracing_amd as vc  # noqa: E402

f32 = np.float32


def camera(width, height, lookfrom=(13, 2, 3), lookat=(0, 0, 0), vup=(0, 1, 0), vfov=20.0):
    """pixel00, delta_u, delta_v, centre as csrc/vcrt_math.h make_camera computes them."""
    def v(a):
        return np.array(a, f32)

    def norm(a):
        return a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])

    centre, at, up = v(lookfrom), v(lookat), v(vup)
    d = centre - at
    focal = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    theta = f32(vfov) * f32(0.017453292519943295)
    hh = f32(math.tan(float(theta / f32(2.0))))
    vh = f32(2.0) * hh * focal
    vw = vh * f32(width // height)  # the shader's integer aspect ratio
    w = norm(d)
    u = norm(np.cross(up, w).astype(f32))
    vv = np.cross(w, u).astype(f32)
    vu, vd = vw * u, vh * -vv
    du, dv = vu / f32(height), vd / f32(height)
    ul = ((centre - focal * w) - vu / f32(2.0)) - vd / f32(2.0)
    return ul + f32(0.5) * (du + dv), du, dv, centre


def camera_rays(width, height, spp, order):
    """origins, dirs [W * H * spp, 3]: a pixel's samples adjacent, the pixels row-major or in
    8 x 8 tiles (the frame kernels' blocks)."""
    p00, du, dv, centre = camera(width, height)
    rand = vc._native.lib().vcrt_canonical_rand
    y, x = np.mgrid[0:height, 0:width]
    if order == "tile":
        key = np.lexsort((x.ravel() % 8, y.ravel() % 8, x.ravel() // 8, y.ravel() // 8))
        x, y = x.ravel()[key], y.ravel()[key]
    x = x.reshape(-1, 1).astype(f32)
    y = y.reshape(-1, 1).astype(f32)
    pc = (p00 + x * du) + y * dv
    dirs = np.empty((len(pc), spp, 3), f32)
    for s in range(spp):
        jx = f32(-0.5) + f32(rand(float(s), float(s)))
        jy = f32(-0.5) + f32(rand(float(s + 1), float(s + 1)))
        dirs[:, s] = (pc + (jx * du + jy * dv)) - centre
    dirs = dirs.reshape(-1, 3)
    return np.tile(centre, (len(dirs), 1)), dirs


def frame_rate(a, variant, tables=None):
    """Frames of the same workload; tables="global" keeps the per-lane scan's tables in global
    memory (VCRT_CULL_LANE_TABLES, read by vcrt_begin), where the query reads them."""
    if tables:
        os.environ["VCRT_CULL_LANE_TABLES"] = tables
    else:
        os.environ.pop("VCRT_CULL_LANE_TABLES", None)
    desc = vc.RenderDesc(width=a.width, height=a.height, samples_per_pixel=a.spp,
                         max_depth=a.depth, device=0, kernel_variant=variant)
    ms, segs, kernel = [], 0, ""
    with vc.Renderer(desc, a.scene) as r:
        for i in range(a.warmup + a.launches):
            r.draw_next_frame()
            st = r.stats()
            if i >= a.warmup:
                ms.append(st["kernel_ms"])
            segs, kernel = st["segments"], st["kernel"]
    os.environ.pop("VCRT_CULL_LANE_TABLES", None)
    med = statistics.median(ms)
    return {"kernel": kernel, "segments": segs, "kernel_ms_median": med,
            "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
            "segments_per_s": segs / (med * 1e-3), "group_tests": st["group_tests"],
            "bound_tests": st["bound_tests"], "grid_blocks": st["grid_blocks"],
            "block_threads": st["block_threads"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--spp", type=int, default=4)
    p.add_argument("--depth", type=int, default=10)
    p.add_argument("--scene", default="final")
    p.add_argument("--launches", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--order", choices=("tile", "row"), default="tile")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ray_query_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    origins, dirs = camera_rays(a.width, a.height, a.spp, a.order)
    res = {"workload": {"width": a.width, "height": a.height, "spp": a.spp, "depth": a.depth,
                        "scene": a.scene, "rays": len(dirs), "ray_order": a.order,
                        "launches": a.launches, "warmup": a.warmup}}
    desc = vc.RenderDesc(width=a.width, height=a.height, samples_per_pixel=a.spp,
                         max_depth=a.depth, device=0)
    with vc.Renderer(desc, a.scene) as r:
        to, td = torch.from_numpy(origins).to(dev), torch.from_numpy(dirs).to(dev)
        ms, st = [], {}
        for i in range(a.warmup + a.launches):
            _, st = r.trace_rays(to, td, a.depth, stats=True)
            if i >= a.warmup:
                ms.append(st["kernel_ms"])
        del to, td
    med = statistics.median(ms)
    res["query"] = {"kernel": st["kernel"], "segments": st["segments"], "kernel_ms_median": med,
                    "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
                    "segments_per_s": st["segments"] / (med * 1e-3),
                    "group_tests": st["group_tests"], "bound_tests": st["bound_tests"]}
    res["frame_cull_lane"] = frame_rate(a, vc.KERNEL_CULL_LANE)
    res["frame_cull_lane_global"] = frame_rate(a, vc.KERNEL_CULL_LANE, "global")
    res["frame_default"] = frame_rate(a, vc.KERNEL_AUTO)
    q = res["query"]["segments_per_s"]
    res["query_over_cull_lane"] = q / res["frame_cull_lane"]["segments_per_s"]
    res["query_over_cull_lane_global"] = q / res["frame_cull_lane_global"]["segments_per_s"]
    res["query_over_default"] = q / res["frame_default"]["segments_per_s"]
    # the same rays: the frame path counts the same segments
    res["same_segments"] = res["query"]["segments"] == res["frame_cull_lane"]["segments"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
