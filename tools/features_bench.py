"""Feature buffers (Renderer.draw_features) against the routes a caller had before.

On one GPU, for each workload (1080p final scene; 4K with 4100 spheres) and n = 1 and 16 samples
per pixel, in one process:
  (a) draw_features(device=True): kernel_ms and host_ms of the call;
  (b) the same with VCRT_FEATURE_LISTS=0 (no ray takes the camera-ray lists);
  (c) the route before: trace_rays on torch device tensors holding the same rays -- built once,
      outside the timing, by frame_rays, a pixel's samples adjacent, the pixels in 8 x 8 tiles --
      with max_depth=1, hits=True: kernel_ms only (the caller's upload, download and averaging
      are not counted);
  (d) the 16-spp frame's kernel_ms.
VCRT_FEATURE_LISTS is read when a renderer begins, so every round begins one renderer with the
lists (a, c, d) and one without (b); each measurement is warmed up and reported as the minimum and
the median over all rounds' runs (at least 5). The planes of (a) and (b) must agree bit for bit,
and (c)'s sphere ids must be (a)'s. Prints one JSON object and, with --out, writes it
(profiles/features.json).
"""
import argparse
import json
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
SAMPLES = (1, 16)
FRAME_SPP = 16


def tile_order_pixels(width, height):
    y, x = np.mgrid[0:height, 0:width]
    x, y = x.ravel(), y.ravel()
    key = np.lexsort((x % 8, y % 8, x // 8, y // 8))
    return np.stack([x[key], y[key]], axis=1).astype(np.int32)


def spread(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms), "runs": len(ms)}


def time_features(r, n, warmup, runs, into):
    out = None
    for i in range(warmup + runs):
        out = r.draw_features(samples=n, device=True, stats=True)
        if i >= warmup:
            into.setdefault("kernel_ms", []).append(out["stats"]["kernel_ms"])
            into.setdefault("host_ms", []).append(out["stats"]["host_ms"])
    st = out["stats"]
    into["counters"] = {k: st[k] for k in ("rays", "listed_rays", "group_tests", "bound_tests")}
    return out


def run_workload(name, w, a):
    import torch
    dev = torch.device("cuda", 0)
    desc = vc.RenderDesc(width=w["width"], height=w["height"], samples_per_pixel=FRAME_SPP,
                         max_depth=a.depth, device=0)
    xy = tile_order_pixels(w["width"], w["height"])
    res = {"workload": dict(w, frame_spp=FRAME_SPP, depth=a.depth, pixels=len(xy))}
    acc = {n: {"lists": {}, "no_lists": {}, "trace_rays": []} for n in SAMPLES}
    frame_ms, frame_kernel = [], ""
    agree = True
    for _ in range(a.rounds):
        os.environ.pop("VCRT_FEATURE_LISTS", None)
        planes = {}
        with vc.Renderer(desc, w["scene"]) as r:
            for n in SAMPLES:
                out = time_features(r, n, a.warmup, a.runs, acc[n]["lists"])
                planes[n] = {k: out[k].cpu().numpy() for k in ("albedo", "normal_depth", "sphere")}
                # (c) the same rays through the ray query, built and uploaded outside the timing
                o, d = vc.frame_rays(desc, xy, 0, n)
                to = torch.from_numpy(o.reshape(-1, 3)).to(dev)
                td = torch.from_numpy(d.reshape(-1, 3)).to(dev)
                del o, d
                for i in range(a.warmup + a.runs):
                    _, hits, st = r.trace_rays(to, td, max_depth=1, hits=True, stats=True)
                    if i >= a.warmup:
                        acc[n]["trace_rays"].append(st["kernel_ms"])
                acc[n]["trace_rays_counters"] = {
                    "rays": int(to.shape[0]), "group_tests": st["group_tests"],
                    "bound_tests": st["bound_tests"]}
                first = hits[:, 1].reshape(len(xy), n)[:, 0].cpu().numpy()
                agree = agree and bool(np.array_equal(first, planes[n]["sphere"][xy[:, 1], xy[:, 0]]))
                del to, td, hits
            for i in range(a.warmup + a.runs):  # (d)
                r.draw_next_frame()
                st = r.stats()
                if i >= a.warmup:
                    frame_ms.append(st["kernel_ms"])
                frame_kernel = st["kernel"]
        os.environ["VCRT_FEATURE_LISTS"] = "0"
        with vc.Renderer(desc, w["scene"]) as r:
            for n in SAMPLES:
                out = time_features(r, n, a.warmup, a.runs, acc[n]["no_lists"])
                for k, v in planes[n].items():
                    agree = agree and bool(np.array_equal(out[k].cpu().numpy().view(np.uint32),
                                                          v.view(np.uint32)))
        os.environ.pop("VCRT_FEATURE_LISTS", None)
    for n in SAMPLES:
        e = {}
        for route in ("lists", "no_lists"):
            e[route] = {"kernel_ms": spread(acc[n][route]["kernel_ms"]),
                        "host_ms": spread(acc[n][route]["host_ms"]),
                        **acc[n][route]["counters"]}
        e["trace_rays_depth1_hits"] = {"kernel_ms": spread(acc[n]["trace_rays"]),
                                       **acc[n]["trace_rays_counters"]}
        a_med = e["lists"]["kernel_ms"]["median"]
        e["lists_over_no_lists"] = a_med / e["no_lists"]["kernel_ms"]["median"]
        e["lists_over_trace_rays"] = a_med / e["trace_rays_depth1_hits"]["kernel_ms"]["median"]
        res[f"n{n}"] = e
    res["frame_16spp"] = {"kernel": frame_kernel, "kernel_ms": spread(frame_ms)}
    res["same_results"] = agree
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
        sys.exit("features_bench: no GPU (there is no CPU path to time)")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "runs_per_round": a.runs, "warmup": a.warmup}
    for name in a.workloads:
        res[name] = run_workload(name, WORKLOADS[name], a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not all(res[name]["same_results"] for name in a.workloads):
        sys.exit("features_bench: the routes disagree")


if __name__ == "__main__":
    main()
