"""The variance-guided chain (Renderer.reproject_moments, variance, denoise_variance) on one GPU,
for each workload (1080p final scene; 4K with 4100 spheres) at 16 spp, in one process, on torch
device planes -- the 16-spp frame, its guides and map, the previous view's frame and surface plane
and a moments plane as the history: kernel_ms of
  vcrt_reproject_moments_pass  beside vcrt_reproject_pass on the same planes
  vcrt_variance_pass           read directly (VCRT_VARIANCE_LDS=0) and staged in LDS (the default),
                               with the history the sequence has (a seventh of the pixels young),
                               with every pixel young (all 49 taps everywhere) and with none
  vcrt_denoise_var_pass        beside vcrt_denoise_pass, both at five levels with every term on,
                               pass by pass
each beside the time its bytes per pixel take at 6.3 TB/s:
  reproject 88 B    (four float4 and a float plane read, a float4 and a float written)
  moments   136 B   (+ albedo and history moments read, moments written)
  variance  36 B    (moments and surface read, a float written: a pixel with the history)
  a denoise pass 64 B (input, albedo, guides read, a float4 written; pass 0 reads the variance
                       plane, the last writes one: + 4 B each)
The two existing calls are the yardsticks: their code is the parent commit's. Every measurement
is warmed up and reported as the minimum, median and maximum over all rounds' runs, the kinds
taken in turn within a round. Prints one JSON object and, with --out, writes it
(profiles/variance.json).
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

WORKLOADS = {
    "1080p_final": dict(width=1920, height=1080, scene="final"),
    "4k_stress4096": dict(width=3840, height=2160, scene="stress4096"),
}
FRAME_SPP = 16
LEVELS = 5
BYTES = {"reproject": 4 * 16 + 4 + 16 + 4, "reproject_moments": 6 * 16 + 4 + 2 * 16 + 4,
         "variance": 2 * 16 + 4, "denoise": LEVELS * 64, "denoise_variance": LEVELS * 64 + 8}
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


def run_workload(w, a):
    import torch
    desc = vc.RenderDesc(width=w["width"], height=w["height"], samples_per_pixel=FRAME_SPP,
                         max_depth=a.depth, device=0)
    prev = orbit(desc, -3.0)
    pixels = w["width"] * w["height"]
    res = {"workload": dict(w, frame_spp=FRAME_SPP, depth=a.depth, pixels=pixels)}
    kinds = ("reproject", "reproject_moments", "variance", "variance_lds", "variance_all_young",
             "variance_all_young_lds", "variance_none_young", "variance_none_young_lds", "denoise",
             "denoise_variance")
    ms = {k: [] for k in kinds}
    passes = {"denoise": [], "denoise_variance": []}
    with vc.Renderer(prev, w["scene"]) as r:
        # the history: the previous view's frame, surface plane and moments; every third column
        # starts over (a pixel whose taps all fall there is young: a seventh of the frame)
        r.draw_next_frame()
        hcol = torch.from_numpy(r.read_framebuffer()).cuda()
        hsurf = r.draw_motion(device=True)["surface"]
        g0 = r.draw_features(samples=4, sphere=False, device=True)
        _, h0 = r.reproject_moments(hcol, r.draw_motion(device=True)["motion"], None,
                                    surface=hsurf, albedo=g0["albedo"])
        hlen = torch.full((w["height"], w["width"]), 8.0, device=hcol.device)
        hlen[:, ::3] = 0.0
        hist = dict(colour=hcol, surface=hsurf, length=hlen, moments=h0["moments"])
        r.set_camera(lookfrom=desc.lookfrom)
        r.draw_next_frame()
        frame = torch.from_numpy(r.read_framebuffer()).cuda()
        mo = r.draw_motion(prev_camera=prev, device=True)
        g = r.draw_features(samples=4, sphere=False, device=True)
        mp = vc.default_reproject_moments_params()
        rp = {k: mp[k] for k in ("alpha", "max_history", "depth_tolerance")}
        dn = dict(levels=LEVELS, sigma_colour=vc.default_denoise_variance_params()["sigma_colour"])

        def variance(lds, **kw):
            os.environ["VCRT_VARIANCE_LDS"] = "1" if lds else "0"
            return r.variance(h2, stats=True, **kw)

        for _ in range(a.rounds):  # the kinds in turn within a round
            for i in range(a.warmup + a.runs):
                out_old, _, st_old = r.reproject(frame, mo["motion"], hist, stats=True, **rp)
                out, h2, st_new = r.reproject_moments(frame, mo["motion"], hist,
                                                      surface=mo["surface"], albedo=g["albedo"],
                                                      stats=True)
                var, sv = variance(False)
                var_lds, sv_lds = variance(True)
                _, sv_all = variance(False, min_history=65535.0)
                _, sv_all_lds = variance(True, min_history=65535.0)
                _, sv_none = variance(False, min_history=1.0)
                _, sv_none_lds = variance(True, min_history=1.0)
                _, sd_old = r.denoise(out_old, g, stats=True, levels=LEVELS)
                _, _, sd_new = r.denoise_variance(out, var, g, stats=True, **dn)
                if i < a.warmup:
                    continue
                for k, st in (("reproject", st_old), ("reproject_moments", st_new),
                              ("variance", sv), ("variance_lds", sv_lds),
                              ("variance_all_young", sv_all),
                              ("variance_all_young_lds", sv_all_lds),
                              ("variance_none_young", sv_none),
                              ("variance_none_young_lds", sv_none_lds), ("denoise", sd_old),
                              ("denoise_variance", sd_new)):
                    ms[k].append(st["kernel_ms"])
                passes["denoise"].append(sd_old["pass_ms"])
                passes["denoise_variance"].append(sd_new["pass_ms"])
        os.environ.pop("VCRT_VARIANCE_LDS", None)
        same = {"reproject_out_words_equal": bool(torch.equal(out.view(torch.int32),
                                                              out_old.view(torch.int32))),
                "variance_lds_words_equal": bool(torch.equal(var.view(torch.int32),
                                                             var_lds.view(torch.int32)))}
        shares = {"accepted": st_new["accepted_pixels"] / pixels,
                  "young": sv["spatial_pixels"] / pixels}
    for k in kinds:
        name = k.split("_lds")[0].split("_all")[0].split("_none")[0]
        floor = pixels * BYTES[name] / ACHIEVABLE_BYTES_PER_S * 1e3
        res[k] = {"kernel_ms": spread(ms[k]), "bytes_per_pixel": BYTES[name],
                  "traffic_floor_ms": floor,
                  "over_floor": statistics.median(ms[k]) / floor}
    for k, v in passes.items():
        res[k]["pass_ms_median"] = [statistics.median(p[l] for p in v) for l in range(LEVELS)]
        res[k]["lds_passes"] = 2
    med = {k: res[k]["kernel_ms"]["median"] for k in kinds}
    res["ratios"] = {
        "moments_over_reproject": med["reproject_moments"] / med["reproject"],
        "moments_over_reproject_bytes": BYTES["reproject_moments"] / BYTES["reproject"],
        "denoise_variance_over_denoise": med["denoise_variance"] / med["denoise"],
        "denoise_variance_over_denoise_bytes": BYTES["denoise_variance"] / BYTES["denoise"],
        "variance_lds_over_direct": med["variance_lds"] / med["variance"],
        "variance_all_young_lds_over_direct": (med["variance_all_young_lds"] /
                                               med["variance_all_young"]),
        "variance_none_young_lds_over_direct": (med["variance_none_young_lds"] /
                                                med["variance_none_young"]),
    }
    res["shares"] = shares
    res["checks"] = same
    res["params"] = {"reproject_moments": mp, "variance": vc.default_variance_params(),
                     "denoise": dn}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    p.add_argument("--depth", type=int, default=50)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--runs", type=int, default=5, help="timed runs per round and measurement")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("variance_bench: no GPU (there is no CPU path to time)")
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
