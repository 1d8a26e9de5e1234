"""GPU parity of the big list's test by sign bits (tracer.hip big_roots, kBigSign / kBigPeel): the
members' roots are entered by hit_sign's sign bits, the block by "some member may hit", and the
second pair of a big group is tested whether or not it has members. Only the block's entries may
change: every frame is the CPU oracle's bit for bit with its segment count.

The scenes give the big list each of its shapes (the host's tables are checked for it, BIG):
 big1..big4  the ground alone (members 1, 2 and 3 are padding: the second pair is absent) and
             with one, two and three large spheres; VCRT_BIG_FILL=0 keeps small spheres out of the
             free slots.
 big6        the ground and five large spheres: two big groups, the loop behind the peeled test.
 glass       the camera inside a large glass sphere: cc < 0 for every camera ray.
 away        no ground, two large spheres behind the camera: every camera ray has hb > 0 and
             cc > 0 for both, so the camera phase never enters the block (kCamBig 0), while the
             line of many such rays still meets a sphere (disc >= 0: the parent's gate passed).
 final       the final scene at 96 x 54 (the oracle frame of test_gpu_group_footprint).
Each runs through the LDS-table flat kernel, the same with VCRT_GROUP_FOOT=0, the cost-order build,
one thin-lens frame, and the stats build, whose counters are held against PARENT: the parent
commit's code object under this host library, rendered beside this build's (the constants do not
come from the build under test). Both runs of the parent gave the same numbers.
"""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import lens_ref as L
from tests import test_gpu_group_footprint as GF
from tests.stats_layout import REGION_DEBUG_BASE
from tests.test_gpu_lens import assert_same
from tools import valu_regions
from vulkancomputeraytracing_amd import scene as S

pytestmark = pytest.mark.gpu

ENV = ("VCRT_DEBUG_STATS", "VCRT_GROUP_FOOT", "VCRT_WORK_ORDER", "VCRT_BIG_FILL",
       "VCRT_CULL_LANE_TABLES", "VCRT_PRIMARY_LISTS", "VCRT_SLAB")

GROUND = ((0, -100, 0), 100.0, (0.5, 0.5, 0.5), 1, 0.9)
LARGE = [((-14, 6, -6), 6.0, (0.8, 0.3, 0.3), 1, 0.5),
         ((12, 6, -10), 6.0, (0.7, 0.6, 0.5), 2, 0.1),
         ((0, 6, -16), 6.0, (1.0, 1.0, 1.0), 3, 1.5),
         ((-20, 6, 8), 6.0, (0.3, 0.8, 0.3), 2, 0.4),
         ((18, 6, 10), 6.0, (0.3, 0.3, 0.8), 1, 0.7)]
CAM = dict(lookfrom=(6, 2.5, 7), lookat=(0, 0.4, 0), vfov=40)
AWAY_CAM = dict(lookfrom=(0, 3, 9), lookat=(0, 0.4, 0), vfov=40)


def small_spheres():
    """64 spheres of radius 0.3 on a jittered 8 x 8 grid at one height, all materials."""
    rng = np.random.default_rng(130)
    rows = []
    for i in range(64):
        c = (1.1 * (i % 8) - 3.85 + float(rng.uniform(-0.2, 0.2)), 0.5,
             1.1 * (i // 8) - 3.85 + float(rng.uniform(-0.2, 0.2)))
        rows.append((c, 0.3, tuple(rng.uniform(0.2, 1, 3)), 1 + i % 3,
                     float(rng.uniform(0, 1.6))))
    return rows


def with_big(*big):
    return lambda: vc.make_spheres(list(big) + small_spheres())


GLASS = (CAM["lookfrom"], 6.0, (1.0, 1.0, 1.0), 3, 1.5)
BEHIND = [((-8, 3, 30), 6.0, (0.8, 0.3, 0.3), 1, 0.5), ((8, 5, 32), 6.0, (0.7, 0.6, 0.5), 2, 0.1)]

#        scene, w, h, spp, depth, camera, VCRT_BIG_FILL
CASES = {
    "big1": (with_big(GROUND), 64, 48, 8, 6, CAM, "0"),
    "big2": (with_big(GROUND, *LARGE[:1]), 64, 48, 8, 6, CAM, "0"),
    "big3": (with_big(GROUND, *LARGE[:2]), 64, 48, 8, 6, CAM, "0"),
    "big4": (with_big(GROUND, *LARGE[:3]), 64, 48, 8, 6, CAM, "0"),
    "big6": (with_big(GROUND, *LARGE), 64, 48, 8, 6, CAM, "0"),
    "glass": (with_big(GROUND, GLASS), 64, 48, 8, 6, CAM, None),
    "away": (with_big(*BEHIND), 64, 48, 8, 6, AWAY_CAM, "0"),
    "final": GF.CASES["final"][:6] + (None,),
}
# members of each big group in the host's tables
BIG = {"big1": [1], "big2": [2], "big3": [3], "big4": [4], "big6": [4, 2], "glass": [4],
       "away": [2], "final": [4]}
LENS = (32, 24, 4, 6, 0.1)  # w, h, spp, depth, lens radius of the lens frame

with open(valu_regions.TRACER) as _f:
    REG = valu_regions.enum_values(_f.read())
M_REGIONS = [f"k{p}BigM{k}" for p in ("Main", "Cam") for k in range(4)]
EQUAL = M_REGIONS + ["kCamRootTrip", "group_tests", "segments"]
AT_MOST = ["kMainBig", "kCamBig"]

# the parent commit's stats build (vcrt_trace_cull_flat_stats), one frame of each case:
# EQUAL + AT_MOST in that order
PARENT = {
    "big1": [622, 0, 0, 0, 570, 0, 0, 0, 757, 3124, 48113, 671, 570],
    "big2": [705, 170, 0, 0, 573, 87, 0, 0, 765, 3399, 51360, 764, 656],
    "big3": [722, 183, 266, 0, 580, 94, 0, 0, 772, 3451, 51835, 779, 670],
    "big4": [733, 185, 266, 288, 582, 95, 0, 94, 778, 3686, 57972, 902, 749],
    "big6": [358, 626, 274, 759, 94, 105, 0, 589, 800, 5456, 59379, 1475, 991],
    "glass": [1061, 1245, 15, 24, 894, 1031, 13, 19, 982, 5054, 80272, 1277, 1031],
    "away": [105, 189, 0, 0, 0, 0, 0, 0, 563, 2066, 33811, 365, 181],
    "final": [217, 147, 450, 896, 125, 91, 196, 777, 1137, 5028, 47097, 1102, 817],
}


def scene_of(oracle, case, for_oracle):
    scene = CASES[case][0]
    if isinstance(scene, str):
        return oracle.scene(scene) if for_oracle else scene
    if case not in _scenes:
        _scenes[case] = scene()
    return _scenes[case]


_scenes, _want = {}, {}


def set_env(monkeypatch, case, **env):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if CASES[case][6] is not None:
        monkeypatch.setenv("VCRT_BIG_FILL", CASES[case][6])
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def reference(oracle, case, st):
    key = (case, st["accumulate_quantum"])
    if key not in _want:
        _, w, h, spp, depth, cam, _ = CASES[case]
        cfg = oracle.config(w, h, spp, depth, **oracle.partition(st), **cam)
        _want[key] = oracle.render(cfg, scene_of(oracle, case, True))
    return _want[key]


def frames(oracle, case, kernel, n=1, code_object=None):
    """n frames of the case through the LDS-table flat kernel, each checked against the oracle;
    the last frame's stats."""
    _, w, h, spp, depth, cam, _ = CASES[case]
    kw = {"code_object_path": code_object} if code_object else {}
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=vc.KERNEL_CULL_FLAT, **cam, **kw)
    with vc.Renderer(desc, scene_of(oracle, case, False)) as r:
        for f in range(n):
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
            want, segs = reference(oracle, case, st)
            what = f"{case} {kernel} frame {f}"
            assert st["kernel"] == kernel, what
            assert_same(got, want, what)
            assert st["segments"] == segs, what
    return st


def test_big_groups_of_the_host_tables(monkeypatch):
    """The shapes the cases claim (host computation only)."""
    for case, members in BIG.items():
        set_env(monkeypatch, case)
        scene = CASES[case][0]
        t = S.cull_tables(S.builtin_scene(scene) if isinstance(scene, str) else scene())
        got = [int((t["index"][g] >= 0).sum()) for g in range(t["nbig"])]
        assert got == members, case


@pytest.mark.parametrize("case", list(CASES))
def test_flat_kernel_bitwise(oracle, monkeypatch, case):
    set_env(monkeypatch, case)
    on = frames(oracle, case, "vcrt_trace_cull_flat")
    set_env(monkeypatch, case, VCRT_GROUP_FOOT="0")
    off = frames(oracle, case, "vcrt_trace_cull_flat")
    print(f"{case}: group_tests {on['group_tests']} / {off['group_tests']} bound_tests "
          f"{on['bound_tests']} / {off['bound_tests']}")
    assert off["bound_tests"] > 0


@pytest.mark.parametrize("case", list(CASES))
def test_cost_order_bitwise(oracle, monkeypatch, case):
    set_env(monkeypatch, case, VCRT_WORK_ORDER="cost")
    frames(oracle, case, "vcrt_trace_cull_flat_cost", n=2)  # the measuring frame, then the order


@pytest.mark.parametrize("case", list(CASES))
def test_lens_frame_bitwise(oracle, monkeypatch, case):
    set_env(monkeypatch, case)
    w, h, spp, depth, radius = LENS
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=vc.KERNEL_CULL_FLAT, lens_radius=radius, **CASES[case][5])
    with vc.Renderer(desc, scene_of(oracle, case, False)) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    want, segs = L.reference_frame(oracle, scene_of(oracle, case, True), desc)
    assert st["kernel"].startswith("vcrt_trace_cull_flat_lens"), case
    assert_same(got, want, f"{case} lens")
    assert st["segments"] == segs, case


def stats_counters(oracle, monkeypatch, case, code_object=None):
    """EQUAL + AT_MOST of one stats-build frame of the case (image and segments checked)."""
    set_env(monkeypatch, case, VCRT_DEBUG_STATS="1")
    st = frames(oracle, case, "vcrt_trace_cull_flat_stats", code_object=code_object)
    return [st[n] if n in st else st["debug"][REGION_DEBUG_BASE + REG[n]]
            for n in EQUAL + AT_MOST]


@pytest.mark.parametrize("case", list(CASES))
def test_stats_counters_as_the_parent(oracle, monkeypatch, case):
    got = stats_counters(oracle, monkeypatch, case)
    print(f"{case}: {dict(zip(EQUAL + AT_MOST, got))}")
    want = PARENT[case]
    n = len(EQUAL)
    assert got[:n] == want[:n], dict(zip(EQUAL, zip(got, want)))
    assert all(g <= p for g, p in zip(got[n:], want[n:])), dict(zip(AT_MOST, zip(got[n:], want[n:])))
    if case == "away":  # no camera ray may hit a sphere behind the camera
        assert got[n + 1] == 0 and want[n + 1] > 0
    else:
        assert got[n] > 0 and got[n + 1] > 0
