"""What a camera move costs: vcrt_set_camera against the only route before it.

For the final scene at 1920x1080 and stress4096 at 3840x2160, 16 samples per pixel, the camera
steps round an orbit about the world y axis (every move is a new view) and each step is timed
four ways, alternating in one process so that they share the machine's noise:

  (a) reopen      close the renderer and open a new one with the new camera
                  (vcrt_end + vcrt_begin + vcrt_set_scene), host wall time
  (b) host        set_camera with VCRT_CAMERA_LISTS=host (the host list builders), host wall time
  (c) device      set_camera (the camera-list kernels), host wall time and the list kernels'
                  HIP-event time from camera_stats
  (d) frame       the first frame after (b) and after (c): frame and kernel milliseconds

Medians and ranges of --reps steps after --warmup warm-ups. At each size the lists of (b) and
(c) are read back once and compared byte for byte. Prints one JSON object and writes it to --out
(profiles/camera_move.json).
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

CONFIGS = [
    ("final_1920x1080", "final", 1920, 1080),
    ("stress4096_3840x2160", "stress4096", 3840, 2160),
]
SPP, DEPTH, STEP_DEG = 16, 50, 7.0


def orbit(k):
    """Step k of the orbit: the default lookfrom turned by k * STEP_DEG about the y axis."""
    th = k * STEP_DEG * math.pi / 180.0
    return dict(lookfrom=(13.0 * math.cos(th) + 3.0 * math.sin(th), 2.0,
                          -13.0 * math.sin(th) + 3.0 * math.cos(th)))


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def set_camera(r, how, cam):
    if how == "host":
        os.environ["VCRT_CAMERA_LISTS"] = "host"
    else:
        os.environ.pop("VCRT_CAMERA_LISTS", None)
    try:
        ms, _ = timed(lambda: r.set_camera(**cam))   # returns when the lists are installed
    finally:
        os.environ.pop("VCRT_CAMERA_LISTS", None)
    cs = r.camera_stats()
    assert cs["on_device"] == (0 if how == "host" else 1), cs
    return ms, cs


def same_lists(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("group_info", "ids", "sphere_info", "rec"))


def run(name, scene_name, width, height, reps, warmup):
    scene = vc.builtin_scene(scene_name)
    desc = vc.RenderDesc(width=width, height=height, samples_per_pixel=SPP, max_depth=DEPTH,
                         device=0)
    keys = ("reopen_ms", "host_ms", "device_ms", "device_lists_ms", "frame_after_host_ms",
            "kernel_after_host_ms", "frame_after_device_ms", "kernel_after_device_ms")
    samples = {k: [] for k in keys}
    r = vc.Renderer(desc, scene)
    r.draw_next_frame()
    step, identical, kernel, counts = 0, True, "", {}
    for i in range(warmup + reps):
        rec = i >= warmup
        # (a) the route without set_camera
        step += 1

        def reopen(r=r, step=step):
            r.close()
            return vc.Renderer(desc.with_camera(**orbit(step)), scene)
        ms, r = timed(reopen)
        r.draw_next_frame()
        if rec:
            samples["reopen_ms"].append(ms)
        # (b) and (c), each followed by its frame (d); the order alternates
        for how in (("host", "device") if i % 2 == 0 else ("device", "host")):
            step += 1
            ms, cs = set_camera(r, how, orbit(step))
            r.draw_next_frame()
            st = r.stats()
            kernel = st["kernel"]
            if rec:
                samples[how + "_ms"].append(ms)
                samples[f"frame_after_{how}_ms"].append(st["frame_ms"])
                samples[f"kernel_after_{how}_ms"].append(st["kernel_ms"])
                if how == "device":
                    samples["device_lists_ms"].append(cs["lists_ms"])
                    counts = {k: cs[k] for k in ("quarters", "group_ids", "pair_records")}
    # the two builders' lists for one more view, byte for byte
    step += 1
    set_camera(r, "host", orbit(step))
    a = r.camera_lists()
    set_camera(r, "device", orbit(step))
    identical = same_lists(a, r.camera_lists())
    r.close()
    out = {k: summary(v) for k, v in samples.items()}
    out.update(scene=scene_name, width=width, height=height, spp=SPP, max_depth=DEPTH,
               frame_kernel=kernel, lists_identical=identical, **counts)
    dev, frame = out["device_ms"]["median"], out["frame_after_device_ms"]["median"]
    out["device_over_reopen"] = dev / out["reopen_ms"]["median"]
    out["device_over_host"] = dev / out["host_ms"]["median"]
    out["move_share_of_step"] = dev / (dev + frame)
    return name, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "camera_move.json"))
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    args = ap.parse_args()
    result = {"tool": "tools/camera_move_bench.py", "reps": args.reps, "warmup": args.warmup,
              "host_threads": min(16, os.cpu_count() or 1), "step_degrees": STEP_DEG,
              "configs": {}}
    for cfg in CONFIGS:
        if cfg[0] in args.configs.split(","):
            name, out = run(*cfg, args.reps, args.warmup)
            result["configs"][name] = out
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not all(c["lists_identical"] for c in result["configs"].values()):
        sys.exit("the host's and the device's lists differ")


if __name__ == "__main__":
    main()
