"""GPU parity of the capped push of the group-footprint level (tracer.hip fact (5g), kPushCap): a
lane whose mask holds more than kPushCap groups is a heavy lane and takes no part in the per-word
push loops; the wave deals its groups across its lanes, the bits that fall on masked-off lanes
through the first live lane. The group stack receives the same multiset of entries, so every
case is bit-identical to the CPU oracle with equal segment counts through the LDS-table kernel
and its cost-order build, and issues exactly the parent commit's group tests (PARENT_GROUP_TESTS,
PARENT_STATS: counts of the parent commit's code object under this host library, rendered beside
this build's; they do not come from the build under test).

 tiny sweep   the grid of 80 groups below the tables' coordinate bound (all-ones masks: every
              lane with a mask is heavy, bits in words 0 to 2) at 1 to 9 pixels, one wave with up
              to 63 lanes masked off, so most bits fall on dead positions; these frames hold 1 to
              3 such lanes. At 47 x 1 a wave holds 7 (560 entries <= 576: the one-step push), at
              55 x 1 two more waves hold 8 (640: the sliced push).
 mixed waves  the final scene and the 128-group grid: light and heavy lanes in one wave, above the
              listed camera lanes' entries.
 ragged       1x1, 5x3 and 63x1 frames of the final scene: partial waves, the drain with masked
              lanes.
"""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import group_footprint_ref as G
from tests import test_gpu_group_footprint as GF
from tests.stats_layout import REGION_DEBUG_BASE, dbg, region
from tools import valu_regions

pytestmark = pytest.mark.gpu

#        scene, w, h, spp, depth, camera
# widths 1 to 9: up to 63 lanes masked off, 1 to 3 lanes with a mask; 47 and 55: a wave of 7 such
# lanes (560 entries, the one-step push) and, at 55, two waves of 8 (640: the sliced push)
TINY_WIDTHS = list(range(1, 10)) + [47, 55]
CASES = {f"tiny{w}": (G.tiny_grid, w, 1, 1, 6, G.TINY_CAM) for w in TINY_WIDTHS}
CASES.update({
    "final": GF.CASES["final"][:6],      # ("final", 96, 54, 4, 10, {}): the oracle frame is shared
    "grid128": GF.CASES["grid128"][:6],  # (G.grid128, 64, 36, 2, 8, G.GRID_CAM)
})
CASES.update({f"final_{w}x{h}x{spp}": ("final", w, h, spp, 10, {})
              for w, h in ((1, 1), (5, 3), (63, 1)) for spp in (1, 3)})

# group_tests of the last frame (plain: the only one; cost: the cost-ordered second one) from the
# parent commit's code object
PARENT_GROUP_TESTS = {
    ("tiny1", False): 162,
    ("tiny1", True): 162,
    ("tiny2", False): 162,
    ("tiny2", True): 162,
    ("tiny3", False): 162,
    ("tiny3", True): 162,
    ("tiny4", False): 162,
    ("tiny4", True): 162,
    ("tiny5", False): 162,
    ("tiny5", True): 162,
    ("tiny6", False): 162,
    ("tiny6", True): 162,
    ("tiny7", False): 162,
    ("tiny7", True): 162,
    ("tiny8", False): 162,
    ("tiny8", True): 162,
    ("tiny9", False): 243,
    ("tiny9", True): 243,
    ("tiny47", False): 486,
    ("tiny47", True): 486,
    ("tiny55", False): 567,
    ("tiny55", True): 567,
    ("final", False): 5028,
    ("final", True): 5028,
    ("grid128", False): 974,
    ("grid128", True): 974,
    ("final_1x1x1", False): 7,
    ("final_1x1x1", True): 7,
    ("final_1x1x3", False): 18,
    ("final_1x1x3", True): 18,
    ("final_5x3x1", False): 11,
    ("final_5x3x1", True): 11,
    ("final_5x3x3", False): 25,
    ("final_5x3x3", True): 25,
    ("final_63x1x1", False): 9,
    ("final_63x1x1", True): 9,
    ("final_63x1x3", False): 26,
    ("final_63x1x3", True): 26,
}

# the parent commit's stats build (VCRT_DEBUG_STATS=1): debug[36] group_pass_entries per case,
# and kSliceGroups of test_gpu_group_footprint's `sliced` case
PARENT_STATS = {
    "tiny1": 80,
    "tiny2": 160,
    "tiny3": 240,
    "tiny4": 160,
    "tiny5": 160,
    "tiny6": 160,
    "tiny7": 160,
    "tiny8": 160,
    "tiny9": 160,
    "tiny47": 560,
    "tiny55": 1840,
    "tiny55 kSliceGroups": 32,
    "final": 41830,
    "sliced": 131680,
    "sliced kSliceGroups": 576,
}

_want = {}


def reference(oracle, case, st):
    if case in GF.CASES:
        return GF.reference(oracle, case, st)
    key = (case, st["accumulate_quantum"])
    if key not in _want:
        scene, w, h, spp, depth, cam = CASES[case]
        sc = oracle.scene(scene) if isinstance(scene, str) else scene()
        cfg = oracle.config(w, h, spp, depth, **oracle.partition(st), **cam)
        _want[key] = oracle.render(cfg, sc)
    return _want[key]


def render(oracle, case, cost, code_object=None):
    """The case through the LDS-table kernel, every frame checked against the oracle; the last
    frame's stats. code_object: another tracer code object (the parent commit's, to record its
    counts)."""
    scene, w, h, spp, depth, cam = CASES[case]
    sc = scene if isinstance(scene, str) else scene()
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=vc.KERNEL_CULL_FLAT, code_object_path=code_object, **cam)
    with vc.Renderer(desc, sc) as r:
        for frame in range(2 if cost else 1):  # cost order: the measuring frame, then the order
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
            want, segs = reference(oracle, case, st)
            what = f"{case} cost={cost} frame {frame}"
            assert st["kernel"] == "vcrt_trace_cull_flat" + ("_cost" if cost else ""), what
            assert np.array_equal(GF.bits(got), GF.bits(want)), what
            assert st["segments"] == segs, what
    return st


@pytest.mark.parametrize("cost", [False, True], ids=["plain", "cost"])
@pytest.mark.parametrize("case", list(CASES))
def test_push_heavy_bitwise(oracle, monkeypatch, case, cost):
    monkeypatch.delenv("VCRT_GROUP_FOOT", raising=False)
    monkeypatch.delenv("VCRT_DEBUG_STATS", raising=False)
    if cost:
        monkeypatch.setenv("VCRT_WORK_ORDER", "cost")
    else:
        monkeypatch.delenv("VCRT_WORK_ORDER", raising=False)
    st = render(oracle, case, cost)
    print(f"{case} cost={cost}: group_tests {st['group_tests']} segments {st['segments']}")
    assert st["bound_tests"] == 0  # the group footprint: no box test on this path
    assert st["group_tests"] == PARENT_GROUP_TESTS[case, cost]


# ---- the stats build ---------------------------------------------------------------------------

with open(valu_regions.TRACER) as _f:
    REG = valu_regions.enum_values(_f.read())


def reg(st, name):
    """A region counter by its name in tracer.hip's reg enum (tests/stats_layout.py's table names
    only the regions the older tests read)."""
    return st["debug"][REGION_DEBUG_BASE + REG[name]]


def stats_frame(oracle, monkeypatch, case, code_object=None):
    """One frame of the case from the LDS-table stats kernel, with every check of
    tests/test_gpu_stats_builds.py (image, segments, counter identities)."""
    from tests import test_gpu_stats_builds as SB
    scene, w, h, spp, depth, cam = CASES[case] if case in CASES else GF.CASES[case][:6]
    key = "sliced" if scene is G.tiny_grid else "grid128" if scene is G.grid128 else scene
    kw = {"code_object_path": code_object} if code_object else {}
    (st,) = SB.stats_frames(oracle, monkeypatch, (key, w, h, spp, depth), *SB.FLAT, cam=cam, **kw)
    return st


def push_trips(st):
    return sum(reg(st, f"kPushGroups{k}") for k in range(4))


def test_stats_tiny_sweep_heavy_and_sliced(oracle, monkeypatch):
    """Over the sweep both the heavy-lane loop and the sliced push run, and every frame takes the
    parent's group-pass entries and the parent's slices. The widths 1 to 9 alone reach the heavy
    loop only (1 to 3 lanes with a mask per frame, kSliceGroups 0 from the parent's code object
    too); widths 47 and 55 hold the totals on either side of the stack's 576: at 47 one wave of 7
    masked lanes, 560 entries in one step, 7 trips of the heavy loop and no slice; at 55 that
    wave and two waves of 8 lanes, 640 entries each, which take the sliced push."""
    heavy = sliced = 0
    for w in TINY_WIDTHS:
        st = stats_frame(oracle, monkeypatch, f"tiny{w}")
        heavy += reg(st, "kPushHeavy")
        sliced += region(st, "kSliceGroups")
        print(f"tiny{w}: kPushHeavy {reg(st, 'kPushHeavy')} kSliceGroups "
              f"{region(st, 'kSliceGroups')} group_pass_entries {dbg(st, 'group_pass_entries')}")
        assert dbg(st, "group_pass_entries") == PARENT_STATS[f"tiny{w}"], w
        assert region(st, "kSliceGroups") == PARENT_STATS.get(f"tiny{w} kSliceGroups", 0), w
        if w in (47, 55):  # the wave of 7 lanes, all heavy, pushed in one step
            assert reg(st, "kPushHeavy") == 7 and push_trips(st) == 0, w
    print(f"tiny sweep: kPushHeavy {heavy} kSliceGroups {sliced}")
    assert heavy > 0 and sliced > 0


def test_stats_final_light_and_heavy_in_one_frame(oracle, monkeypatch):
    st = stats_frame(oracle, monkeypatch, "final")
    print(f"final: kPushHeavy {reg(st, 'kPushHeavy')} push trips {push_trips(st)} "
          f"group_pass_entries {dbg(st, 'group_pass_entries')}")
    assert reg(st, "kPushHeavy") > 0 and push_trips(st) > 0
    assert dbg(st, "group_pass_entries") == PARENT_STATS["final"]


def test_stats_sliced_case_as_the_parent(oracle, monkeypatch):
    st = stats_frame(oracle, monkeypatch, "sliced")
    assert region(st, "kSliceGroups") == PARENT_STATS["sliced kSliceGroups"]
    assert dbg(st, "group_pass_entries") == PARENT_STATS["sliced"]
