"""tools/sim/push_trips.py's model of the capped push (tracer.hip kPushCap) on hand-made waves, and
on sampled waves of the final scene the properties tests/test_gpu_push_heavy.py's mixed cases
rely on. No GPU."""
import re

import numpy as np

from tools import valu_regions
from tools.sim import push_trips as P


def kernel_cap():
    with open(valu_regions.TRACER) as f:
        return int(re.search(r"#define VCRT_PUSH_CAP (\d+)", f.read()).group(1))


C = kernel_cap()


def wave(counts_per_word):
    """[64, 4] from {lane: (w0, w1, w2, w3)}."""
    w = np.zeros((64, 4), np.int64)
    for lane, words in counts_per_word.items():
        w[lane] = words
    return w


def test_cap_is_the_kernels_and_fits_the_prefix():
    assert 1 <= C <= 7  # light counts go through the 3-bit wave prefix


def test_all_light_lanes():
    """No lane above the cap: the trips are the per-word maxima, with or without the cap, and
    the cap costs only its fixed part."""
    w = wave({0: (1, 0, 0, 0), 5: (0, 2, 0, 1), 9: (1, 1, 1, 0), 63: (0, 0, 0, 3)})
    assert w.sum(1).max() <= C
    now, cap = P.wave_cost(w), P.wave_cost(w, C)
    assert now["trips"] == cap["trips"] == 1 + 2 + 1 + 3
    assert now["heavy"] == cap["heavy"] == 0
    assert now["entries"] == cap["entries"] == 10
    assert now["valu"] == P.kTripValu * 7
    assert cap["valu"] == P.kTripValu * 7 + P.kFixedValu


def test_one_heavy_lane_among_zeros():
    """The heavy lane leaves the loops: no trip at all, one co-operative lane, whatever its
    count."""
    for words in ((C + 1, 0, 0, 0), (3, 4, 5, 6), (32, 32, 16, 0)):
        w = wave({17: words})
        now, cap = P.wave_cost(w), P.wave_cost(w, C)
        assert now["trips"] == sum(words) and now["heavy"] == 0
        assert cap["trips"] == 0 and cap["heavy"] == 1
        assert cap["entries"] == now["entries"] == sum(words)
        assert cap["valu"] == P.kHeavyValu + P.kFixedValu


def test_counts_at_the_cap_and_one_above():
    at = (C - C // 2, C // 2, 0, 0)           # exactly C groups: light
    above = (C - C // 2, C // 2, 1, 0)        # C + 1: heavy
    w = wave({1: at, 2: above})
    cap = P.wave_cost(w, C)
    assert sum(at) == C and sum(above) == C + 1
    assert cap["heavy"] == 1 and cap["trips"] == sum(at)  # only lane 1's words set the trips
    assert P.wave_cost(w)["trips"] == sum(above)
    assert P.wave_cost(w, C + 1)["heavy"] == 0
    assert P.wave_cost(w, C - 1)["heavy"] == 2 and P.wave_cost(w, C - 1)["trips"] == 0


def test_histogram_and_means():
    waves = np.stack([wave({0: (1, 0, 0, 0)}), wave({0: (0, 0, 9, 0), 1: (1, 1, 0, 0)})])
    h = P.count_histogram(waves, top=8)
    assert h.shape == (9,) and abs(h.sum() - 1) < 1e-12
    assert h[1] == 1 / 128 and h[2] == 1 / 128 and h[8] == 1 / 128 and h[0] == 125 / 128
    m = P.model(waves, 6)
    assert m["heavy"] == 0.5 and m["trips"] == (1 + 2) / 2 and m["entries"] == 6.0


def test_sampled_waves_of_the_final_scene():
    """50 waves: some lanes hold more groups than the cap, most at most the cap (the mixed GPU
    cases need both kinds in one wave), and the cap shortens the loops."""
    waves = P.sample_waves(50)
    assert waves.shape == (50, 64, 4)
    cnt = waves.sum(2)
    assert 0 <= cnt.min() and cnt.max() <= 128
    heavy = cnt > C
    assert heavy.any()
    assert heavy.mean() < 0.1 and (cnt <= C).mean() > 0.9
    assert (heavy.any(1) & (~heavy & (cnt > 0)).any(1)).any()  # both kinds in one wave
    now, cap = P.model(waves), P.model(waves, C)
    assert cap["entries"] == now["entries"]
    assert cap["trips"] < now["trips"]
