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

--occlusion instead times the occlusion query (vcrt_occlude_rays) on the same rays: against the
depth-1 closest-hit query, alternating, and on shadow rays from the first-hit points to a point
light (profiles/occlusion_bench.json).
"""
import argparse
import ctypes
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


def summary(ms, st, rays):
    med = statistics.median(ms)
    return {"kernel": st["kernel"], "rays": rays, "kernel_ms_median": med,
            "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "rays_per_s": rays / (med * 1e-3),
            "group_tests_per_ray": st["group_tests"] / rays,
            "bound_tests_per_ray": st["bound_tests"] / rays}


def occlusion(a, origins, dirs):
    """--occlusion: vcrt_occlude_rays against vcrt_trace_rays at depth 1 (hits only) on the same
    rays, the two alternating launch by launch in one renderer; then shadow rays from each first
    hit to a point light. The answers are compared too (the same rays, the same scene)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(dirs)
    res = {"workload": {"width": a.width, "height": a.height, "spp": a.spp, "scene": a.scene,
                        "rays": n, "ray_order": a.order, "launches": a.launches,
                        "warmup": a.warmup, "light": list(a.light)}}
    desc = vc.RenderDesc(width=a.width, height=a.height, samples_per_pixel=a.spp,
                         max_depth=a.depth, device=0)
    lib = vc._native.lib()
    with vc.Renderer(desc, a.scene) as r:
        to, td = torch.from_numpy(origins).to(dev), torch.from_numpy(dirs).to(dev)
        # (a) is anything hit at all: the closest-hit query at depth 1 against the any-hit one
        hits_t = torch.empty((n, 8), dtype=torch.int32, device=dev)
        ms_hit, ms_occ = [], []
        st_hit = vc._native.vcrt_ray_stats()
        for i in range(a.warmup + a.launches):
            torch.cuda.synchronize(dev)
            vc._native.check("vcrt_trace_rays_device", lib.vcrt_trace_rays_device(
                to.data_ptr(), td.data_ptr(), n, 1, None, hits_t.data_ptr(),
                ctypes.byref(st_hit)))
            occ, st_occ = r.occluded(to, td, stats=True)
            if i >= a.warmup:
                ms_hit.append(st_hit.kernel_ms)
                ms_occ.append(st_occ["kernel_ms"])
        hit = {"kernel": st_hit.kernel.decode(), "group_tests": st_hit.group_tests,
               "bound_tests": st_hit.bound_tests}
        res["first_hit_depth1"] = summary(ms_hit, hit, n)
        res["occluded_default_reach"] = summary(ms_occ, st_occ, n)
        rec = hits_t.cpu().numpy()
        occ = occ.cpu().numpy()
        sphere = rec[:, 1]
        res["same_answers"] = bool(np.array_equal(occ, sphere >= 0))
        res["occluded_fraction"] = float(occ.mean())
        res["occluded_over_first_hit"] = (res["first_hit_depth1"]["kernel_ms_median"] /
                                          res["occluded_default_reach"]["kernel_ms_median"])
        # (b) shadow rays: from each first-hit point o + t d (fp32) to the light, reach 1
        sel = sphere >= 0
        t = np.ascontiguousarray(rec[:, 0]).view(f32)[sel].reshape(-1, 1)
        so = np.ascontiguousarray(origins[sel] + t * dirs[sel], dtype=f32)
        sd = np.ascontiguousarray(np.array(a.light, f32) - so, dtype=f32)
        del to, td, hits_t
        to, td = torch.from_numpy(so).to(dev), torch.from_numpy(sd).to(dev)
        ms, st = [], {}
        for i in range(a.warmup + a.launches):
            shadow, st = r.occluded(to, td, 1.0, stats=True)
            if i >= a.warmup:
                ms.append(st["kernel_ms"])
        res["shadow_rays"] = summary(ms, st, len(so))
        res["shadow_rays"]["occluded_fraction"] = float(shadow.cpu().numpy().mean())
        del to, td
    return res


def write(res, out):
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


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
    p.add_argument("--occlusion", action="store_true",
                   help="time vcrt_occlude_rays against vcrt_trace_rays at depth 1, and shadow "
                        "rays to --light (profiles/occlusion_bench.json)")
    p.add_argument("--light", type=float, nargs=3, default=(0.0, 20.0, 0.0))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ray_query_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    origins, dirs = camera_rays(a.width, a.height, a.spp, a.order)
    if a.occlusion:
        write(occlusion(a, origins, dirs), a.out)
        return
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
    write(res, a.out)


if __name__ == "__main__":
    main()
