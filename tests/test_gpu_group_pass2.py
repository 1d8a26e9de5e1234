"""GPU parity of the double group pass of the group-footprint scan (tracer.hip flat_group_pass2):
where a wave's group stack holds more than its nact live lanes, one pass tests two entries per
lane, one after the other, and pushes both tests' candidates with one prefix and one loop, onto a
candidate stack kept in the unused node stack. Entries and candidates are unordered multisets and
a double pass counts as two, so every case is bit-identical to the CPU oracle with equal segment
counts through the LDS-table kernel and its cost-order build, and issues exactly the parent
commit's group tests and group-pass entries (the constants of tests/test_gpu_push_heavy.py where
the case is one of its cases, else PARENT_GROUP_TESTS / PARENT_STATS below: counts of the parent
commit's code object under this host library, rendered beside this build's).

 final        the final scene at 96 x 54 x 4: full and ragged waves, listed camera lanes.
 tiny1-9      the one-height all-ones grid, nact = 1 to 9 live lanes, one to three of them pushing
              80 entries each: many double passes with masked-off lanes (the bit-sliced prefix), the
              last of them partly filled in either half.
 tiny47, 55   560 entries in one step and 640 sliced: double passes between the slices, where
              only full halves are taken.
 grid128      the 128-group grid at 64 x 36 x 2: light and heavy lanes in full waves.
 grid128_e*   the same grid in one 8 x 8 tile at depth 1: one wave, one scan of its 64 camera rays
              (or 32, the tile's upper half), so the stats build's group-pass entries are that
              wave's stack height. The field of view sets it: 65 entries on 64 lanes (nact + 1: a
              double pass whose second half holds one entry), 128 (2 nact: both halves full), 131
              (just over: a double pass and a single one of 3), and 65 on 32 lanes (2 nact + 1).
 foot_off     the final scene with VCRT_GROUP_FOOT=0: the node path, which takes no double pass.
"""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import group_footprint_ref as G
from tests import test_gpu_group_footprint as GF
from tests import test_gpu_push_heavy as PH
from tests.stats_layout import dbg, region

pytestmark = pytest.mark.gpu

TINY = [f"tiny{w}" for w in list(range(1, 10)) + [47, 55]]
#        scene, w, h, spp, depth, camera
GRID = {
    "grid128_e65": (G.grid128, 8, 8, 1, 1, dict(G.GRID_CAM, vfov=58.0)),
    "grid128_e128": (G.grid128, 8, 8, 1, 1, dict(G.GRID_CAM, vfov=31.875)),
    "grid128_e131": (G.grid128, 8, 8, 1, 1, dict(G.GRID_CAM, vfov=31.75)),
    "grid128_e65_32": (G.grid128, 8, 4, 1, 1, dict(G.GRID_CAM, vfov=26.0)),
}
CASES = {c: PH.CASES[c] for c in ["final"] + TINY + ["grid128"]}
CASES.update(GRID)

# group_tests of the last frame (plain / cost order) from the parent commit's code object, for the
# cases tests/test_gpu_push_heavy.py does not record
PARENT_GROUP_TESTS = {
    ("grid128_e65", False): 3,
    ("grid128_e65", True): 3,
    ("grid128_e128", False): 3,
    ("grid128_e128", True): 3,
    ("grid128_e131", False): 4,
    ("grid128_e131", True): 4,
    ("grid128_e65_32", False): 4,
    ("grid128_e65_32", True): 4,
    ("foot_off", False): 4454,
    ("foot_off", True): 4454,
}
# debug[36] group_pass_entries of the parent commit's stats build: in the one-scan frames the
# wave's group stack height
PARENT_STATS = {
    "grid128": 9092,
    "grid128_e65": 65,
    "grid128_e128": 128,
    "grid128_e131": 131,
    "grid128_e65_32": 65,
}
# double passes of the one-scan frames: ceil(entries / nact) group passes, paired from the top
DOUBLE_PASSES = {"grid128_e65": 1, "grid128_e128": 1, "grid128_e131": 1, "grid128_e65_32": 1}

_want = {}


def reference(oracle, case, st):
    if case in PH.CASES:
        return PH.reference(oracle, case, st)  # the oracle frames are shared with that module
    key = (case, st["accumulate_quantum"])
    if key not in _want:
        scene, w, h, spp, depth, cam = CASES[case]
        cfg = oracle.config(w, h, spp, depth, **oracle.partition(st), **cam)
        _want[key] = oracle.render(cfg, scene())
    return _want[key]


def render(oracle, case, cost, code_object=None):
    """The case through the LDS-table kernel, every frame checked against the oracle; the last
    frame's stats. code_object: the parent commit's, to record its counts."""
    if case in PH.CASES:
        return PH.render(oracle, case, cost, code_object)
    scene, w, h, spp, depth, cam = CASES[case]
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=vc.KERNEL_CULL_FLAT, code_object_path=code_object, **cam)
    with vc.Renderer(desc, scene()) as r:
        for frame in range(2 if cost else 1):  # cost order: the measuring frame, then the order
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
            want, segs = reference(oracle, case, st)
            what = f"{case} cost={cost} frame {frame}"
            assert st["kernel"] == "vcrt_trace_cull_flat" + ("_cost" if cost else ""), what
            assert np.array_equal(GF.bits(got), GF.bits(want)), what
            assert st["segments"] == segs, what
    return st


def parent_group_tests(case, cost):
    if (case, cost) in PH.PARENT_GROUP_TESTS:
        return PH.PARENT_GROUP_TESTS[case, cost]
    return PARENT_GROUP_TESTS[case, cost]


def set_order(monkeypatch, cost):
    monkeypatch.delenv("VCRT_DEBUG_STATS", raising=False)
    if cost:
        monkeypatch.setenv("VCRT_WORK_ORDER", "cost")
    else:
        monkeypatch.delenv("VCRT_WORK_ORDER", raising=False)


@pytest.mark.parametrize("cost", [False, True], ids=["plain", "cost"])
@pytest.mark.parametrize("case", list(CASES))
def test_group_pass2_bitwise(oracle, monkeypatch, case, cost):
    monkeypatch.delenv("VCRT_GROUP_FOOT", raising=False)
    set_order(monkeypatch, cost)
    st = render(oracle, case, cost)
    print(f"{case} cost={cost}: group_tests {st['group_tests']} segments {st['segments']}")
    assert st["bound_tests"] == 0  # the group footprint: no box test on this path
    assert st["group_tests"] == parent_group_tests(case, cost)


@pytest.mark.parametrize("cost", [False, True], ids=["plain", "cost"])
def test_group_footprint_off_takes_the_node_path(oracle, monkeypatch, cost):
    monkeypatch.setenv("VCRT_GROUP_FOOT", "0")
    set_order(monkeypatch, cost)
    st = render(oracle, "final", cost)
    print(f"foot_off cost={cost}: group_tests {st['group_tests']} bound_tests {st['bound_tests']}")
    assert st["bound_tests"] > 0
    assert st["group_tests"] == PARENT_GROUP_TESTS["foot_off", cost]


# ---- the stats build ---------------------------------------------------------------------------

def stats_frame(oracle, monkeypatch, case, env=None, code_object=None):
    """One frame of the case from the LDS-table stats kernel, with every check of
    tests/test_gpu_stats_builds.py (image, segments, counter identities)."""
    from tests import test_gpu_stats_builds as SB
    scene, w, h, spp, depth, cam = CASES[case]
    key = "sliced" if scene is G.tiny_grid else "grid128" if scene is G.grid128 else scene
    kw = {"code_object_path": code_object} if code_object else {}
    (st,) = SB.stats_frames(oracle, monkeypatch, (key, w, h, spp, depth), *SB.FLAT, env=env,
                            cam=cam, **kw)
    return st


def pass_counts(st):
    return (f"group_pass_entries {dbg(st, 'group_pass_entries')} kPassGroup "
            f"{PH.reg(st, 'kPassGroup')} kGroupPass2 {PH.reg(st, 'kGroupPass2')} kDrainTrip "
            f"{PH.reg(st, 'kDrainTrip')} kLevelGroups {region(st, 'kLevelGroups')}")


@pytest.mark.parametrize("case", list(CASES))
def test_stats_second_half_taken(oracle, monkeypatch, case):
    """Every case holds a wave with more than nact group entries (the final scene about 100 per
    scan; the one-scan grids 65 to 131 on 64 or 32 lanes; the tiny grids 80 per masked lane in
    waves of 1 to 9 live lanes, 560 and 640 in the waves of 47 and 55), so the double pass runs,
    each counted as two group passes, and takes the parent's group-pass entries."""
    st = stats_frame(oracle, monkeypatch, case)
    print(f"{case}: {pass_counts(st)}")
    want = PH.PARENT_STATS[case] if case in PH.PARENT_STATS else PARENT_STATS[case]
    assert dbg(st, "group_pass_entries") == want
    assert 0 < 2 * PH.reg(st, "kGroupPass2") <= PH.reg(st, "kPassGroup")
    if case in DOUBLE_PASSES:
        assert PH.reg(st, "kGroupPass2") == DOUBLE_PASSES[case]
        assert PH.reg(st, "kPassGroup") == -(-want // st["segments"])  # nact = the camera rays
    assert region(st, "kSliceGroups") == PH.PARENT_STATS.get(f"{case} kSliceGroups", 0)


def test_stats_group_footprint_off_takes_no_double_pass(oracle, monkeypatch):
    st = stats_frame(oracle, monkeypatch, "final", env={"VCRT_GROUP_FOOT": "0"})
    print(f"foot_off: {pass_counts(st)}")
    assert PH.reg(st, "kGroupPass2") == 0 and PH.reg(st, "kPassGroup") > 0
    assert region(st, "kLevelGroups") == 0 and region(st, "kLevelNodes") > 0
