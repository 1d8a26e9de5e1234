"""The reprojection map (Renderer.draw_motion) and temporal accumulation (Renderer.reproject) on
one GPU, for each workload (1080p final scene; 4K with 4100 spheres) at 16 spp, in one process:
  (a) vcrt_frame_motion's kernel_ms for a previous camera 3 degrees back on the orbit and for the
      same camera (the identity rule), beside vcrt_frame_features' with one sample on the same
      renderer: all three run the same first-hit work for one ray a pixel;
  (b) vcrt_reproject_pass's kernel_ms and the call's host_ms on torch device planes -- the 16-spp
      frame, the map of (a), the previous view's frame and surface plane as the history -- with
      the default parameters, with and without the statistics (the per-wave tally of accepted
      pixels), against
        the same filter composed from torch ops on the same planes (wall time around a
        synchronise; its plane is compared with the kernel's and the largest difference is
        recorded: torch's operation order is its own), and
        the traffic floor: 88 bytes a pixel that must move (four float4 planes and a float plane
        read, a float4 and a float plane written) at 6.3 TB/s;
  (c) the 16-spp frame's own kernel_ms.
Every measurement is warmed up and reported as the minimum, median and maximum over all rounds'
runs, the kinds taken in turn within a round. Prints one JSON object and, with --out, writes it
(profiles/reproject.json).
"""
import argparse
import json
import math
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
FRAME_SPP = 16
BYTES_PER_PIXEL = 4 * 16 + 4 + 16 + 4  # read: four float4 and a float; written: a float4, a float
ACHIEVABLE_BYTES_PER_S = 6.3e12


def spread(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms), "runs": len(ms)}


def orbit(desc, degrees):
    th = math.radians(degrees)
    dx, dz = desc.lookfrom[0] - desc.lookat[0], desc.lookfrom[2] - desc.lookat[2]
    return desc.with_camera(lookfrom=(
        float(np.float32(desc.lookat[0] + dx * math.cos(th) + dz * math.sin(th))),
        desc.lookfrom[1],
        float(np.float32(desc.lookat[2] - dx * math.sin(th) + dz * math.cos(th)))))


def torch_reproject(colour, motion, hcol, hsurf, hlen, p):
    """The filter of vcrt.h composed from torch ops: what a caller writes without vcrt_reproject."""
    import torch
    H, W = colour.shape[:2]
    mx, my, mz, mw = motion.unbind(-1)
    valid = (mw >= 1) & (mx > -1) & (mx < W) & (my > -1) & (my < H)
    sx, sy = torch.where(valid, mx, 0.0), torch.where(valid, my, 0.0)
    fx, fy = sx.floor(), sy.floor()
    ax, ay = sx - fx, sy - fy
    ix, iy = fx.long(), fy.long()
    acc = torch.zeros_like(colour[..., :3])
    lsum, wsum = torch.zeros_like(mx), torch.zeros_like(mx)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        b = (ax if dx else 1 - ax) * (ay if dy else 1 - ay)
        qx, qy = ix + dx, iy + dy
        inside = valid & (b != 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        flat = qy.clamp(0, H - 1) * W + qx.clamp(0, W - 1)
        s = hsurf.reshape(-1, 4)[flat]
        lq = hlen.reshape(-1)[flat]
        rz = (mz - s[..., 1]).abs() / (mz.abs() + s[..., 1].abs() + 2.0 ** -20)
        ok = (mw == 1) | (rz <= p["depth_tolerance"]) if p["depth_tolerance"] else True
        take = inside & (s[..., 0] == mw) & (lq >= 1) & ok
        b = torch.where(take, b, 0.0)
        acc += b[..., None] * hcol.reshape(-1, 4)[flat][..., :3]
        lsum += b * lq
        wsum += b
    took = wsum > 0
    safe = torch.where(took, wsum, 1.0)
    h3 = acc / safe[..., None]
    n = torch.clamp(lsum / safe + 1, max=p["max_history"])
    a = torch.clamp(1 / n, min=p["alpha"])
    out = colour.clone()
    out[..., :3] = torch.where(took[..., None], h3 + a[..., None] * (colour[..., :3] - h3),
                               colour[..., :3])
    return out, torch.where(took, n, 1.0)


def run_workload(w, a):
    import torch
    desc = vc.RenderDesc(width=w["width"], height=w["height"], samples_per_pixel=FRAME_SPP,
                         max_depth=a.depth, device=0)
    prev = orbit(desc, -3.0)
    params = vc.default_reproject_params()
    pixels = w["width"] * w["height"]
    res = {"workload": dict(w, frame_spp=FRAME_SPP, depth=a.depth, pixels=pixels),
           "params": params}
    ms = {k: [] for k in ("frame", "motion_orbit", "motion_same", "features_1", "reproject",
                          "reproject_host", "reproject_no_stats_wall", "torch")}
    with vc.Renderer(prev, w["scene"]) as r:
        # the history: the previous view's frame and surface plane
        r.draw_next_frame()
        hcol = torch.from_numpy(r.read_framebuffer()).cuda()
        hsurf = r.draw_motion(device=True)["surface"]
        hlen = torch.full((w["height"], w["width"]), 4.0, device=hcol.device)
        r.set_camera(lookfrom=desc.lookfrom)
        for i in range(a.warmup + a.runs):  # (c)
            r.draw_next_frame()
            st = r.stats()
            if i >= a.warmup:
                ms["frame"].append(st["kernel_ms"])
        frame_kernel = st["kernel"]
        frame = torch.from_numpy(r.read_framebuffer()).cuda()
        for _ in range(a.rounds):  # (a): the kinds in turn within a round
            for i in range(a.warmup + a.runs):
                mo = r.draw_motion(prev_camera=prev, device=True, stats=True)
                same = r.draw_motion(device=True, stats=True)
                ft = r.draw_features(samples=1, device=True, stats=True)
                if i >= a.warmup:
                    ms["motion_orbit"].append(mo["stats"]["kernel_ms"])
                    ms["motion_same"].append(same["stats"]["kernel_ms"])
                    ms["features_1"].append(ft["stats"]["kernel_ms"])
        motion_stats = {k: mo["stats"][k] for k in ("rays", "hit_rays", "projected", "identity",
                                                    "listed_rays")}
        hist = dict(colour=hcol, surface=hsurf, length=hlen)
        for _ in range(a.rounds):  # (b)
            for i in range(a.warmup + a.runs):
                out, h2, st = r.reproject(frame, mo["motion"], hist, stats=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r.reproject(frame, mo["motion"], hist)
                wall = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    ms["reproject"].append(st["kernel_ms"])
                    ms["reproject_host"].append(st["host_ms"])
                    ms["reproject_no_stats_wall"].append(wall)
        accepted = st["accepted_pixels"]
        for i in range(a.torch_warmup + a.torch_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            composed, clen = torch_reproject(frame, mo["motion"], hcol, hsurf, hlen, params)
            torch.cuda.synchronize()
            if i >= a.torch_warmup:
                ms["torch"].append((time.perf_counter() - t0) * 1e3)
        d = (composed[..., :3] - out[..., :3]).abs()
        diff = {"max_abs": float(d.max()), "mean_abs": float(d.mean()),
                "words_equal": float((composed.view(torch.int32) ==
                                      out.view(torch.int32)).float().mean()),
                "lengths_equal": float((clen == h2["length"]).float().mean())}
    floor_ms = pixels * BYTES_PER_PIXEL / ACHIEVABLE_BYTES_PER_S * 1e3
    res["frame_16spp"] = {"kernel": frame_kernel, "kernel_ms": spread(ms["frame"])}
    res["motion"] = {"orbit_3_degrees": {"kernel_ms": spread(ms["motion_orbit"]), **motion_stats},
                     "same_camera": {"kernel_ms": spread(ms["motion_same"])},
                     "features_1_sample": {"kernel_ms": spread(ms["features_1"])}}
    res["motion_over_features_1"] = (res["motion"]["orbit_3_degrees"]["kernel_ms"]["median"] /
                                     res["motion"]["features_1_sample"]["kernel_ms"]["median"])
    res["reproject"] = {"kernel_ms": spread(ms["reproject"]),
                        "host_ms": spread(ms["reproject_host"]),
                        "wall_ms_without_stats": spread(ms["reproject_no_stats_wall"]),
                        "accepted_share": accepted / pixels,
                        "traffic_floor_ms": floor_ms,
                        "bytes_per_pixel": BYTES_PER_PIXEL}
    res["reproject_over_floor"] = res["reproject"]["kernel_ms"]["median"] / floor_ms
    res["torch_composition"] = {"wall_ms": spread(ms["torch"]),
                                "difference_from_reproject": diff}
    res["torch_over_reproject_host_ms"] = (res["torch_composition"]["wall_ms"]["median"] /
                                           res["reproject"]["host_ms"]["median"])
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    p.add_argument("--depth", type=int, default=50)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--runs", type=int, default=5, help="timed runs per round and measurement")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--torch-runs", type=int, default=3)
    p.add_argument("--torch-warmup", type=int, default=1)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("reproject_bench: no GPU (there is no CPU path to time)")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "runs_per_round": a.runs, "warmup": a.warmup}
    for name in a.workloads:
        res[name] = run_workload(WORKLOADS[name], a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
