"""What the thin lens costs a frame (vcrt_render_desc.lens_radius).

At 1920x1080, 1024 spp, depth 10, the final scene and the default camera, renders in one process
    (a) the pinhole with every default,
    (b) the pinhole without its camera-ray lists (VCRT_PRIMARY_LISTS=0: no fast trace, no
        group-level footprint -- the path a lens frame's rays take),
    (c) lens_radius 0.05,
and reports for each the median vcrt_stats.kernel_ms of --frames frames after --warmup
warm-ups, the frame's segments and the ns per segment, with c/b and c/a in ns per segment.
Prints one JSON object and writes it to --out (profiles/lens_bench.json).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("VCRT_PKG_ROOT",
                                  os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import vulkancomputeraytracing_amd as vc  # noqa: E402


def measure(a, lens_radius, primary_lists):
    """One configuration: kernel, median kernel ms, segments, ns per segment."""
    if primary_lists:
        os.environ.pop("VCRT_PRIMARY_LISTS", None)
    else:
        os.environ["VCRT_PRIMARY_LISTS"] = "0"  # read by vcrt_begin
    desc = vc.RenderDesc(width=a.width, height=a.height, samples_per_pixel=a.spp,
                         max_depth=a.depth, device=a.device, lens_radius=lens_radius)
    times = []
    with vc.Renderer(desc, "final") as r:
        for k in range(a.warmup + a.frames):
            r.draw_next_frame()
            if k >= a.warmup:
                times.append(r.stats()["kernel_ms"])
        st = r.stats()
    os.environ.pop("VCRT_PRIMARY_LISTS", None)
    ms = statistics.median(times)
    return {"kernel": st["kernel"], "kernel_ms": ms, "kernel_ms_min": min(times),
            "kernel_ms_max": max(times), "segments": st["segments"],
            "ns_per_segment": ms * 1e6 / st["segments"], "lens_radius": lens_radius,
            "primary_lists": bool(primary_lists)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--lens-radius", type=float, default=0.05)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "lens_bench.json"))
    a = ap.parse_args()
    res = {"width": a.width, "height": a.height, "spp": a.spp, "depth": a.depth,
           "scene": "final", "frames": a.frames, "warmup": a.warmup,
           "a_pinhole": measure(a, 0.0, True),
           "b_pinhole_no_lists": measure(a, 0.0, False),
           "c_lens": measure(a, a.lens_radius, True)}
    ns = {k: res[k]["ns_per_segment"] for k in ("a_pinhole", "b_pinhole_no_lists", "c_lens")}
    res["c_over_b_ns_per_segment"] = ns["c_lens"] / ns["b_pinhole_no_lists"]
    res["c_over_a_ns_per_segment"] = ns["c_lens"] / ns["a_pinhole"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
