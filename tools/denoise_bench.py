"""The denoiser (Renderer.denoise) against the route a caller had before: the same filter composed
from torch ops.

On one GPU, for each workload (1080p final scene; 4K with 4100 spheres) at 16 spp, in one process:
  (a) denoise(frame, guides) on torch device tensors -- the 16-spp framebuffer and the guide
      planes of draw_features(samples=16, device=True) -- with the default parameters: kernel_ms
      (all passes), each pass's ms and host_ms (the whole call), for VCRT_DENOISE_LDS = 2 (the
      passes of step 1 and 2 stage their footprint in LDS), 1 and 0 (every pass reads its taps
      directly), the three taken in turn within every round; their planes must agree bit for bit;
  (b) the same filter written with torch ops on the same device and the same planes (tap by tap,
      slices of the planes, tests/denoise_ref's formulas): wall time around a synchronise. Its
      plane is compared with (a)'s and the largest difference is recorded (torch's division and
      its operation order are its own, so bits may differ);
  (c) the 16-spp frame's and the guide buffers' own kernel_ms.
Every measurement is warmed up and reported as the minimum, median and maximum over all rounds'
runs. Prints one JSON object and, with --out, writes it (profiles/denoise.json).
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
FRAME_SPP = 16
LDS_SETTINGS = ("2", "1", "0")
K5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def spread(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms), "runs": len(ms)}


def torch_denoise(colour, albedo, nd, p):
    """The filter of vcrt.h composed from torch ops: what a caller writes without vcrt_denoise."""
    import torch
    H, W = colour.shape[:2]
    k = [0.0 if s == 0 else 1.0 / (s * s) for s in (p["sigma_normal"], p["sigma_depth"],
                                                    p["sigma_albedo"], p["sigma_colour"])]
    floor = torch.clamp(albedo[..., :3], min=2.0 ** -10)
    s = colour[..., :3] / floor if p["demodulate"] else colour[..., :3].clone()
    kl = k[3]
    for level in range(p["levels"]):
        step = 1 << level
        acc = torch.zeros_like(s)
        wsum = torch.zeros((H, W), dtype=s.dtype, device=s.device)
        for dy in range(-2, 3):
            oy = step * dy
            y0, y1 = max(0, -oy), min(H, H - oy)
            if y0 >= y1:
                continue
            for dx in range(-2, 3):
                ox = step * dx
                x0, x1 = max(0, -ox), min(W, W - ox)
                if x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                X = torch.zeros((y1 - y0, x1 - x0), dtype=s.dtype, device=s.device)
                if k[0]:
                    X = X + ((nd[P][..., :3] - nd[Q][..., :3]) ** 2).sum(-1) * k[0]
                if k[1]:
                    zp, zq = nd[P][..., 3], nd[Q][..., 3]
                    rz = (zp - zq) / (zp.abs() + zq.abs() + 2.0 ** -20)
                    X = X + rz * rz * k[1]
                if k[2]:
                    X = X + ((albedo[P] - albedo[Q]) ** 2).sum(-1) * k[2]
                if kl:
                    X = X + ((s[P] - s[Q]) ** 2).sum(-1) * kl
                e = 1.0 - torch.clamp(X, max=1.0)
                w = (K5[dx + 2] * K5[dy + 2]) * (e * e)
                acc[P] += w[..., None] * s[Q]
                wsum[P] += w
        s = acc / wsum[..., None]
        kl *= 4.0
    out = torch.empty_like(colour)
    out[..., :3] = s * floor if p["demodulate"] else s
    out[..., 3] = colour[..., 3]
    return out


def run_workload(w, a):
    import torch
    desc = vc.RenderDesc(width=w["width"], height=w["height"], samples_per_pixel=FRAME_SPP,
                         max_depth=a.depth, device=0)
    params = vc.default_denoise_params()
    res = {"workload": dict(w, frame_spp=FRAME_SPP, depth=a.depth,
                            pixels=w["width"] * w["height"]), "params": params}
    acc = {lds: {"kernel_ms": [], "host_ms": [], "pass_ms": []} for lds in LDS_SETTINGS}
    frame_ms, feature_ms, torch_ms = [], [], []
    agree, diff = True, {}
    with vc.Renderer(desc, w["scene"]) as r:
        for i in range(a.warmup + a.runs):  # (c)
            r.draw_next_frame()
            st = r.stats()
            g = r.draw_features(samples=FRAME_SPP, sphere=False, device=True, stats=True)
            if i >= a.warmup:
                frame_ms.append(st["kernel_ms"])
                feature_ms.append(g["stats"]["kernel_ms"])
        frame_kernel = st["kernel"]
        frame = torch.from_numpy(r.read_framebuffer()).cuda()
        guides = dict(albedo=g["albedo"], normal_depth=g["normal_depth"])
        planes = {}
        for _ in range(a.rounds):  # (a): the settings in turn within a round
            for i in range(a.warmup + a.runs):
                for lds in LDS_SETTINGS:
                    os.environ["VCRT_DENOISE_LDS"] = lds
                    out, st = r.denoise(frame, guides, stats=True)
                    if i >= a.warmup:
                        acc[lds]["kernel_ms"].append(st["kernel_ms"])
                        acc[lds]["host_ms"].append(st["host_ms"])
                        acc[lds]["pass_ms"].append(st["pass_ms"])
                    acc[lds]["lds_passes"] = st["lds_passes"]
                    planes[lds] = out
            for lds in LDS_SETTINGS[1:]:
                agree = agree and bool(torch.equal(planes[lds].view(torch.int32),
                                                   planes[LDS_SETTINGS[0]].view(torch.int32)))
        os.environ.pop("VCRT_DENOISE_LDS", None)
        default_out, default_st = r.denoise(frame, guides, stats=True)
        for i in range(a.torch_warmup + a.torch_runs):  # (b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            composed = torch_denoise(frame, guides["albedo"], guides["normal_depth"], params)
            torch.cuda.synchronize()
            if i >= a.torch_warmup:
                torch_ms.append((time.perf_counter() - t0) * 1e3)
        d = (composed[..., :3] - default_out[..., :3]).abs()
        diff = {"max_abs": float(d.max()), "mean_abs": float(d.mean()),
                "words_equal": float((composed.view(torch.int32) ==
                                      default_out.view(torch.int32)).float().mean())}
    res["denoise"] = {}
    for lds in LDS_SETTINGS:
        per_pass = np.array(acc[lds]["pass_ms"])
        res["denoise"][f"lds_{lds}"] = {
            "lds_passes": acc[lds]["lds_passes"],
            "kernel_ms": spread(acc[lds]["kernel_ms"]),
            "host_ms": spread(acc[lds]["host_ms"]),
            "pass_ms_median": [float(v) for v in np.median(per_pass, axis=0)],
        }
    res["default_lds_passes"] = default_st["lds_passes"]
    res["torch_composition"] = {"wall_ms": spread(torch_ms), "difference_from_denoise": diff}
    best = min(res["denoise"].values(), key=lambda e: e["kernel_ms"]["median"])
    res["torch_over_denoise_host_ms"] = (res["torch_composition"]["wall_ms"]["median"] /
                                         best["host_ms"]["median"])
    res["frame_16spp"] = {"kernel": frame_kernel, "kernel_ms": spread(frame_ms)}
    res["features_16"] = {"kernel_ms": spread(feature_ms)}
    res["same_results"] = agree
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
        sys.exit("denoise_bench: no GPU (there is no CPU path to time)")
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
    if not all(res[name]["same_results"] for name in a.workloads):
        sys.exit("denoise_bench: the LDS and the direct passes disagree")


if __name__ == "__main__":
    main()
