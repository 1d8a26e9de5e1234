"""What moving the spheres costs: vcrt_update_spheres against vcrt_set_scene.

For the final scene at 1920x1080 and stress4096 at 3840x2160, 16 samples per pixel, every sphere
but the ground drifts a little each step (x and z by up to +-STEP, a random walk from an integer
hash) and each step is timed four ways, alternating in one process so that they share the
machine's noise:

  (a) update      update_spheres from a numpy array (the refit kernels), host wall time, and the
                  refit's and the list kernels' HIP-event times from scene_update_stats
  (b) device      update_spheres from a torch tensor on the device, host wall time
  (c) host        update_spheres with VCRT_SCENE_UPDATE=host (the host refit), host wall time
  (d) set_scene   set_scene of the same values (the rebuild), host wall time

Medians and ranges of --reps steps after --warmup warm-ups. Then the cost of the stale grouping:
the 16-spp frame before the drift and after 1, 10 and 100 accumulated steps refitted on the
device, and after a set_scene of the last values (regrouped). A tree without update_spheres (the
parent commit, through VCRT_PKG_ROOT) measures (d) alone; --parent-json merges such a result in.
Prints one JSON object and writes it to --out (profiles/scene_update.json).
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

CONFIGS = [
    ("final_1920x1080", "final", 1920, 1080),
    ("stress4096_3840x2160", "stress4096", 3840, 2160),
]
SPP, DEPTH, STEP = 16, 50, 0.02
f32 = np.float32


def signed(i, salt):
    """fp32 in [-1, 1) from an integer hash of the indices i and a salt."""
    x = (np.asarray(i, np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) \
        & np.uint64(0xFFFFFFFF)
    for _ in range(2):
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return (x >> np.uint64(8)).astype(f32) * f32(2.0 ** -23) - f32(1)


def drift(scene, step):
    """One more step of the walk: x, z of every sphere below radius 10 by up to +-STEP."""
    out = scene.copy()
    i = np.flatnonzero(np.abs(scene["radius"]) < f32(10))
    out["center"][i, 0] += f32(STEP) * signed(i, 2 * step + 1)
    out["center"][i, 2] += f32(STEP) * signed(i, 2 * step + 2)
    return out


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def frame_ms(r, frames=5):
    out = []
    for _ in range(frames):
        r.draw_next_frame()
        out.append(r.stats()["frame_ms"])
    return statistics.median(out[1:])  # the first frame of a scene measures the cost order


def run(name, scene_name, width, height, reps, warmup):
    has_update = hasattr(vc.Renderer, "update_spheres")
    scene = vc.builtin_scene(scene_name)
    desc = vc.RenderDesc(width=width, height=height, samples_per_pixel=SPP, max_depth=DEPTH,
                         device=0)
    ways = ("update", "device", "host", "set_scene") if has_update else ("set_scene",)
    samples = {w + "_ms": [] for w in ways}
    samples.update({k: [] for k in ("update_refit_ms", "update_lists_ms")} if has_update else {})
    out = {}
    with vc.Renderer(desc, scene) as r:
        out["frame_ms_before"] = frame_ms(r)
        out["frame_kernel"] = r.stats()["kernel"]
        cur, step = scene, 0
        if has_update:
            import torch
        for i in range(warmup + reps):
            rec = i >= warmup
            for k in range(len(ways)):  # the order rotates
                way = ways[(i + k) % len(ways)]
                step += 1
                cur = drift(cur, step)
                if way == "set_scene":
                    ms = timed(lambda: r.set_scene(cur))
                elif way == "device":
                    t = torch.from_numpy(cur.view(f32).reshape(-1, 10)).to("cuda:0")
                    torch.cuda.synchronize()
                    ms = timed(lambda: r.update_spheres(t))
                else:
                    if way == "host":
                        os.environ["VCRT_SCENE_UPDATE"] = "host"
                    try:
                        ms = timed(lambda: r.update_spheres(cur))
                    finally:
                        os.environ.pop("VCRT_SCENE_UPDATE", None)
                if way != "set_scene":
                    us = r.scene_update_stats()
                    assert (us["on_device"], us["rebuilt"]) == (0 if way == "host" else 1, 0), us
                    if rec and way == "update":
                        samples["update_refit_ms"].append(us["refit_ms"])
                        samples["update_lists_ms"].append(us["lists_ms"])
                if rec:
                    samples[way + "_ms"].append(ms)
                r.draw_next_frame()
        out.update({k: summary(v) for k, v in samples.items()})
        if has_update:
            # the stale grouping: the scene set again, then drifting by refits alone
            r.set_scene(scene)
            cur, frames = scene, {}
            for step in range(1, 101):
                cur = drift(cur, 1000 + step)
                if step in (1, 10, 100):
                    r.update_spheres(cur)
                    frames[str(step)] = frame_ms(r)
            out["frame_ms_after_steps"] = frames
            r.set_scene(cur)
            out["frame_ms_regrouped_after_100"] = frame_ms(r)
            out["update_over_set_scene"] = (out["update_ms"]["median"] /
                                            out["set_scene_ms"]["median"])
            out["update_share_of_step"] = out["update_ms"]["median"] / (
                out["update_ms"]["median"] + out["frame_ms_before"])
    out.update(scene=scene_name, spheres=len(scene), width=width, height=height, spp=SPP,
               max_depth=DEPTH)
    return name, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "scene_update.json"))
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    ap.add_argument("--parent-json", default=None,
                    help="this tool's output at the parent commit: its set_scene times are "
                         "recorded as parent_set_scene_ms")
    args = ap.parse_args()
    result = {"tool": "tools/scene_update_bench.py", "reps": args.reps, "warmup": args.warmup,
              "host_threads": min(16, os.cpu_count() or 1), "step": STEP, "configs": {}}
    for cfg in CONFIGS:
        if cfg[0] in args.configs.split(","):
            name, out = run(*cfg, args.reps, args.warmup)
            result["configs"][name] = out
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        for name, out in result["configs"].items():
            if name in parent["configs"]:
                out["parent_set_scene_ms"] = parent["configs"][name]["set_scene_ms"]
                out["update_over_parent_set_scene"] = (
                    out["update_ms"]["median"] / out["parent_set_scene_ms"]["median"])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
