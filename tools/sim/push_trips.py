"""The push loops of the group-footprint level (tracer.hip fact (5g)) over whole sampled waves:
what a cap on the per-lane push (kPushCap) does to the loops' trips. A wave is 64 paths of a 2x2
pixel neighbourhood of the final scene's 1080p camera, one random bounce segment of each, with
each lane's 128-bit group mask from the host's own tables (footprint_groups.py's sampler: float64
paths with approximate scattering; statistics only).

The kernel pushes a light lane's groups (at most `cap`) with one ctz loop per mask word, which the
wave leaves with its busiest light lane, and deals each heavy lane's groups across the wave. Per
cap this prints the per-lane count histogram, the trips per wave (the sum over the four words of
the largest light per-word count), the heavy lanes per wave and a modelled VALU cost:
kTripValu per trip, kHeavyValu per heavy lane, kFixedValu per wave with a cap. The "now" line (no
cap) is what the stats build counts in kPushGroups0..3 per wave-iteration.

  python tools/sim/push_trips.py [waves, default 400] [caps, default 4,6,8]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

kTripValu, kHeavyValu, kFixedValu = 8, 26, 6
f32 = np.float32


def wave_cost(words, cap=None):
    """One wave. words: [lanes, 4] groups per lane and mask word; cap: kPushCap, None = no cap
    (every lane pushes its own). -> dict(trips, heavy, entries, valu)."""
    words = np.asarray(words, np.int64).reshape(-1, 4)
    cnt = words.sum(1)
    heavy = np.zeros(len(cnt), bool) if cap is None else cnt > cap
    light = words[~heavy]
    trips = int(light.max(0).sum()) if len(light) else 0
    nh = int(heavy.sum())
    valu = kTripValu * trips + (0 if cap is None else kHeavyValu * nh + kFixedValu)
    return {"trips": trips, "heavy": nh, "entries": int(cnt.sum()), "valu": valu}


def model(waves, cap=None):
    """Means over waves ([waves, lanes, 4]) of wave_cost's fields, and trips' median and p90."""
    rows = [wave_cost(w, cap) for w in waves]
    out = {k: float(np.mean([r[k] for r in rows])) for k in rows[0]}
    t = np.array([r["trips"] for r in rows])
    out["trips_median"], out["trips_p90"] = float(np.median(t)), float(np.percentile(t, 90))
    return out


def count_histogram(waves, top=8):
    """Fractions of lanes with 0, 1, ..., top - 1 groups and with top or more."""
    cnt = np.asarray(waves).reshape(-1, 4).sum(1)
    h = np.bincount(np.minimum(cnt, top), minlength=top + 1).astype(np.float64)
    return h / h.sum()


def sample_waves(nwaves, seed=3):
    """[nwaves, 64, 4] groups per lane and mask word of sampled waves of the final scene."""
    from tests import footprint_ref as F
    from tests import group_footprint_ref as G
    from tools.sim import footprint_nodes as FN
    from vulkancomputeraytracing_amd import scene as S

    rng = np.random.default_rng(seed)
    sp = S.builtin_scene("final")
    t, gf = S.cull_tables(sp), S.cull_group_footprint(sp)
    lo, hi, _, real = G.group_boxes(t)
    ylo, yhi = float(lo[real][:, 1].min()), float(hi[real][:, 1].max())
    n = gf["tables"].shape[1]
    O, D = [], []
    for _ in range(nwaves):
        x, y = int(rng.integers(0, FN.W - 1)), int(rng.integers(0, FN.H - 1))
        for lane in range(64):
            segs = []
            for _try in range(8):  # a path that leaves the scene at once has no bounce segment
                segs = FN.bounce_segments(x + (lane & 1), y + ((lane >> 1) & 1))
                if segs:
                    break
            if not segs:  # a pixel of sky: a ray that meets no group box
                segs = [(np.array([0.0, 1e6, 0.0]), np.array([0.0, 1.0, 0.0]))]
            o, d = segs[int(rng.integers(0, len(segs)))]
            O.append(o)
            D.append(d)
    O, D = np.array(O), np.array(D)
    D = np.where(np.abs(D) < 1e-12, 1e-12, D)
    ty = np.stack([(ylo - O[:, 1]) / D[:, 1], (yhi - O[:, 1]) / D[:, 1]])
    t0, t1 = np.maximum(ty.min(0), 0.0), ty.max(0)
    empty = t1 < t0
    xa, xb = O[:, 0] + t0 * D[:, 0], O[:, 0] + t1 * D[:, 0]
    za, zb = O[:, 2] + t0 * D[:, 2], O[:, 2] + t1 * D[:, 2]
    cell = lambda v, key: F.cell(v.astype(f32), gf[key], n)  # noqa: E731
    T = gf["tables"]
    m = T[0][cell(np.maximum(xa, xb), "x")] & T[1][cell(np.minimum(xa, xb), "x")] & \
        T[2][cell(np.maximum(za, zb), "z")] & T[3][cell(np.minimum(za, zb), "z")]
    m = np.where(empty[:, None], np.uint32(0), m.astype(np.uint32)) | \
        gf["always"][None, :].astype(np.uint32)
    words = np.zeros(m.shape, np.int64)
    for k in range(32):
        words += (m >> np.uint32(k)) & np.uint32(1)
    return words.reshape(nwaves, 64, 4)


def main():
    nwaves = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    caps = [int(c) for c in (sys.argv[2] if len(sys.argv) > 2 else "4,6,8").split(",")]
    waves = sample_waves(nwaves)
    h = count_histogram(waves)
    print(f"{nwaves} waves of 64 bounce segments; lanes by group count: " +
          ", ".join(f"{k}: {100 * v:.1f} %" for k, v in enumerate(h[:-1])) +
          f", {len(h) - 1}+: {100 * h[-1]:.1f} %")
    for cap in [None] + caps:
        r = model(waves, cap)
        cnt = waves.sum(2)
        over = "" if cap is None else f" ({100 * (cnt > cap).mean():.2f} % of lanes above the cap)"
        print(f"{'now  ' if cap is None else f'cap {cap}'}: {r['entries']:.1f} entries per wave, "
              f"{r['trips']:.2f} trips (median {r['trips_median']:.0f}, p90 {r['trips_p90']:.0f}), "
              f"{r['heavy']:.2f} heavy lanes per wave{over}, modelled VALU {r['valu']:.0f}")


if __name__ == "__main__":
    main()
