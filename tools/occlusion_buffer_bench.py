"""The ambient visibility buffer (Renderer.draw_occlusion) against the route a caller had before.

On one GPU, for each workload (1080p final scene; 4K with 4100 spheres) and (n, m) = (1, 8) and
(16, 8) samples per pixel and secondary rays per hit sample, in one process:
  (a) draw_occlusion(device=True): kernel_ms and host_ms of the call;
  (b) the route before: trace_rays(max_depth=1, hits=True) on the frame's rays (frame_rays, a
      pixel's samples adjacent, the pixels in 8 x 8 tiles), then occluded() on the secondary rays
      of the samples that hit, one batch per sample index, a sample's m rays adjacent. The rays
      are built on the device with torch, one rounded fp32 operation at a time, outside the
      timing: the two kernel times are reported alone, and again with the uploads a caller who
      builds the rays on the host pays (the same arrays copied from pageable host memory, timed
      once, wall clock);
  (c) the 16-spp frame's kernel_ms at the description's depth;
  (d) draw_features(device=True) for the same n: kernel_ms.
Every measurement is warmed up and reported as the minimum and the median of its runs. (b)'s
counts of hit samples and of occluded rays must be (a)'s. The counters: (a)'s group and box tests
less (d)'s are its secondary rays' (the camera rays take the same routes in both), next to
occlude_rays' for the same rays. Prints one JSON object and, with --out, writes it
(profiles/occlusion_buffer.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("VCRT_PKG_ROOT",
                                  os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402

import vulkancomputeraytracing_amd as vc  # noqa: E402

WORKLOADS = {
    "1080p_final": dict(width=1920, height=1080, scene="final"),
    "4k_stress4096": dict(width=3840, height=2160, scene="stress4096"),
}
CASES = ((1, 8), (16, 8))
FRAME_SPP = 16
REACH = 1e5


def tile_order_pixels(width, height):
    y, x = np.mgrid[0:height, 0:width]
    x, y = x.ravel(), y.ravel()
    key = np.lexsort((x % 8, y % 8, x // 8, y // 8))
    return np.stack([x[key], y[key]], axis=1).astype(np.int32)


def spread(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms), "runs": len(ms)}


def upload_ms(torch, dev, tensors):
    """Wall time of copying the tensors' contents from pageable host memory to the device."""
    host = [t.cpu().numpy() for t in tensors]
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    keep = [torch.from_numpy(h).to(dev) for h in host]
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) * 1e3
    del keep, host
    return ms


def route_before(torch, dev, r, desc, xy, n, m, a):
    """(b): per run the two kernel times; once the uploads; the counts and counters."""
    o, d = vc.frame_rays(desc, xy, 0, n)
    to = torch.from_numpy(o.reshape(-1, 3)).to(dev)
    td = torch.from_numpy(d.reshape(-1, 3)).to(dev)
    del o, d
    u = torch.from_numpy(vc.ambient_dirs(0, n * m).reshape(n, m, 3)).to(dev)
    trace, occl = [], []
    res = {}
    for run in range(a.warmup + a.runs):
        first_run = run == 0
        _, hits, st = r.trace_rays(to, td, max_depth=1, hits=True, stats=True)
        t_ms, o_ms = st["kernel_ms"], 0.0
        up = upload_ms(torch, dev, (to, td)) if first_run else 0.0
        occluded = groups = bounds = rays = 0
        nhit = int((hits[:, 1] >= 0).sum())
        for i in range(n):  # one batch per sample index
            h = hits[i::n]
            sel = h[:, 1] >= 0
            f = h[sel][:, [0, 4, 5, 6]].contiguous().view(torch.float32)
            O, D = to[i::n][sel], td[i::n][sel]
            t, nrm = f[:, 0:1], f[:, 1:4]
            P = O + t * D
            dn = (D[:, 0] * nrm[:, 0] + D[:, 1] * nrm[:, 1]) + D[:, 2] * nrm[:, 2]
            nn = torch.where((dn > 0)[:, None], -nrm, nrm)
            d2 = (nn[:, None, :] + u[i][None, :, :]).reshape(-1, 3).contiguous()
            P = P[:, None, :].expand(-1, m, -1).reshape(-1, 3).contiguous()
            occ, so = r.occluded(P, d2, tmax=REACH, stats=True)
            o_ms += so["kernel_ms"]
            occluded += int(occ.sum())
            groups += so["group_tests"]
            bounds += so["bound_tests"]
            rays += int(P.shape[0])
            if first_run:
                up += upload_ms(torch, dev, (P, d2))
            del P, d2, occ, f, O, D
        if first_run:
            res["upload_ms_once"] = up
        if run >= a.warmup:
            trace.append(t_ms)
            occl.append(o_ms)
        res.update(hit_rays=nhit, secondary_rays=rays, occluded=occluded,
                   trace_rays_counters={"group_tests": st["group_tests"],
                                        "bound_tests": st["bound_tests"]},
                   occlude_rays_counters={"group_tests": groups, "bound_tests": bounds})
        del hits
    res["trace_rays_kernel_ms"] = spread(trace)
    res["occlude_rays_kernel_ms"] = spread(occl)
    res["kernels_ms"] = spread([x + y for x, y in zip(trace, occl)])
    res["kernels_and_uploads_ms"] = res["kernels_ms"]["median"] + res["upload_ms_once"]
    return res


def run_workload(w, a):
    import torch
    dev = torch.device("cuda", 0)
    desc = vc.RenderDesc(width=w["width"], height=w["height"], samples_per_pixel=FRAME_SPP,
                         max_depth=a.depth, device=0)
    xy = tile_order_pixels(w["width"], w["height"])
    res = {"workload": dict(w, frame_spp=FRAME_SPP, depth=a.depth, pixels=len(xy), reach=REACH)}
    agree = True
    with vc.Renderer(desc, w["scene"]) as r:
        frame = []
        for i in range(a.warmup + a.runs):  # (c)
            r.draw_next_frame()
            st = r.stats()
            if i >= a.warmup:
                frame.append(st["kernel_ms"])
        res["frame_16spp"] = {"kernel": st["kernel"], "kernel_ms": spread(frame)}
        for n, m in CASES:
            e = {}
            kernel, host, feat = [], [], []
            for i in range(a.warmup + a.runs):  # (a)
                _, sa = r.draw_occlusion(samples=n, rays=m, reach=REACH, device=True, stats=True)
                if i >= a.warmup:
                    kernel.append(sa["kernel_ms"])
                    host.append(sa["host_ms"])
            for i in range(a.warmup + a.runs):  # (d)
                sf = r.draw_features(samples=n, device=True, stats=True)["stats"]
                if i >= a.warmup:
                    feat.append(sf["kernel_ms"])
            e["draw_occlusion"] = {
                "kernel_ms": spread(kernel), "host_ms": spread(host),
                **{k: sa[k] for k in ("rays", "hit_rays", "secondary_rays", "occluded",
                                      "listed_rays", "group_tests", "bound_tests")}}
            e["draw_features"] = {"kernel_ms": spread(feat), "group_tests": sf["group_tests"],
                                  "bound_tests": sf["bound_tests"]}
            b = route_before(torch, dev, r, desc, xy, n, m, a)
            e["route_before"] = b
            agree = agree and (b["hit_rays"], b["occluded"]) == (sa["hit_rays"], sa["occluded"])
            sec = max(sa["secondary_rays"], 1)
            e["per_secondary_ray"] = {
                "fused_group_tests": (sa["group_tests"] - sf["group_tests"]) / sec,
                "fused_bound_tests": (sa["bound_tests"] - sf["bound_tests"]) / sec,
                "occlude_rays_group_tests": b["occlude_rays_counters"]["group_tests"] / sec,
                "occlude_rays_bound_tests": b["occlude_rays_counters"]["bound_tests"] / sec}
            a_med = e["draw_occlusion"]["kernel_ms"]["median"]
            e["fused_over_route_before_kernels"] = a_med / b["kernels_ms"]["median"]
            e["fused_over_frame_16spp"] = a_med / res["frame_16spp"]["kernel_ms"]["median"]
            res[f"n{n}_m{m}"] = e
            print(f"{w['scene']} n{n} m{m}: fused {a_med:.3f} ms, before "
                  f"{b['kernels_ms']['median']:.3f} ms", file=sys.stderr, flush=True)
    res["same_results"] = agree
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    p.add_argument("--depth", type=int, default=50)
    p.add_argument("--runs", type=int, default=5, help="timed runs per measurement")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("occlusion_buffer_bench: no GPU (there is no CPU path to time)")
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup}
    for name in a.workloads:
        res[name] = run_workload(WORKLOADS[name], a)
        if a.out:  # (kept after every workload)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    if not all(res[name]["same_results"] for name in a.workloads):
        sys.exit("occlusion_buffer_bench: the routes disagree")


if __name__ == "__main__":
    main()
