"""The group passes of the group-footprint scan's drain (tracer.hip flat_drain_groups) over whole
sampled waves: how many group entries a wave-iteration holds and how many group-pass trips its
drain runs with single passes (min(ng, nact) entries a trip) and with double passes (min(ng,
2 nact) a trip wherever ng > nact). The waves are push_trips.py's: 64 paths of a 2x2 pixel
neighbourhood of the final scene's 1080p camera, one random bounce segment of each, with each
lane's 128-bit group mask from the host's own tables (float64 paths with approximate scattering;
statistics only). A wave with fewer live lanes (nact < 64) is modelled by its first nact lanes.

The sampler mixes random segments of random paths; the kernel's waves hold neighbouring pixels at
similar depths and are less uniform, so the stats build's counts of a real frame belong beside
these figures (profiles/r12_ab_log.md).

  python tools/sim/pass_trips.py [waves, default 400] [nact list, default 64,48,32,16]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tools.sim.push_trips import sample_waves  # noqa: E402


def trips(entries, nact, double):
    """Group-pass trips of a drain over `entries` group entries with nact live lanes."""
    per = 2 * nact if double else nact
    return -(-np.asarray(entries) // per)


def model(waves, nact):
    """waves: [n, 64, 4] groups per lane and mask word. -> dict of the wave statistics."""
    e = np.asarray(waves)[:, :nact].sum((1, 2))
    one, two = trips(e, nact, False), trips(e, nact, True)
    return {
        "entries": float(e.mean()),
        "le_nact": float((e <= nact).mean()),
        "le_2nact": float(((e > nact) & (e <= 2 * nact)).mean()),
        "gt_2nact": float((e > 2 * nact).mean()),
        "single": float(one.mean()),
        "double": float(two.mean()),
        "second_half": float((e > nact).mean()),  # drains with at least one double pass
        "double_passes": float((e // (2 * nact) + ((e % (2 * nact)) > nact)).mean()),
    }


def main():
    nwaves = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    nacts = [int(c) for c in (sys.argv[2] if len(sys.argv) > 2 else "64,48,32,16").split(",")]
    waves = sample_waves(nwaves)
    print(f"{nwaves} waves of 64 bounce segments")
    for nact in nacts:
        r = model(waves, nact)
        print(f"nact {nact}: {r['entries']:.1f} entries per wave; waves with <= nact entries "
              f"{100 * r['le_nact']:.1f} %, nact+1..2 nact {100 * r['le_2nact']:.1f} %, more "
              f"{100 * r['gt_2nact']:.1f} %; group-pass trips single {r['single']:.2f} -> double "
              f"{r['double']:.2f} ({r['double_passes']:.2f} double passes per wave)")


if __name__ == "__main__":
    main()
