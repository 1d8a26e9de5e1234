"""GPU parity of the trimmed per-iteration code of the flat tracer (tracer.hip: the camera
phase's guard with its origin half decided by the host, which withholds the camera-ray lists
from a frame that fails it; guard_a's integer form; the fast sine's degree-15 polynomial): every frame bit for bit against the CPU oracle with equal segment counts,
and on the frames tests/test_gpu_push_heavy.py pins (the final scene 96x54x4 plain and cost
order, the tiny grid at 47x1 and 55x1) the parent commit's group_tests and group_pass_entries,
read from that module's tables.

Besides those: a 12-group grid, a progressive two-frame render, a 2-way shard, a thin-lens frame,
and the guards' other side -- a scene with a centre beyond 2^30 (no culled scan at all), a camera
beyond 2^30 (no lists: no camera fast trace, every wave with a ray from the camera scans
linearly), camera rays with dot(d, d) below 2^-20 (guard_a false) -- and a frame whose drain
steals (kSteal > 0 in the stats build).
"""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import group_footprint_ref as G
from tests import lens_ref as L
from tests import ray_query_ref as R
from tests import test_gpu_push_heavy as PH
from tests import test_gpu_stats_builds as SB
from tests.stats_layout import dbg, region
from tests.test_gpu_lens import assert_same

pytestmark = pytest.mark.gpu
N = vc._native

FAR_CAM = dict(lookfrom=(3e9, 2.0, 3.0))  # |x| > 2^30: the camera centre fails the range guard


def far_centre_scene():
    sp = vc.builtin_scene("final").copy()
    sp["center"][7, 0] = 3e9  # beyond 2^30: the scene is not bounded, no culled scan
    return sp


SCENES = {"grid12": G.grid12, "tiny": G.tiny_grid, "far_centre": far_centre_scene}
_want = {}


def scene_of(oracle, scene):
    return (SCENES[scene](),) * 2 if scene in SCENES else (scene, oracle.scene(scene))


def frames(oracle, monkeypatch, case, variant=N.KERNEL_CULL_FLAT, cam=None, nframes=1,
           stats=False, **desc_kw):
    """Renders the case with the product kernel (stats: its statistics build); every frame's
    image and segments are checked against the oracle (a rank's own pixels, a progressive
    frame's own samples). The frames' stats."""
    scene, w, h, spp, depth = case
    cam = cam or {}
    for name in SB.ENV:
        monkeypatch.delenv(name, raising=False)
    if stats:
        monkeypatch.setenv("VCRT_DEBUG_STATS", "1")
    gpu_scene, cpu_scene = scene_of(oracle, scene)
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=variant, **cam, **desc_kw)
    world, rank = desc.world_size, desc.rank
    m = vc.tile_pixel_map(w, h, world)
    mine = m[..., 0] == rank

    def want(total, part, frame_spp):
        key = (scene, w, h, total, depth, part["quantum"], frame_spp, tuple(sorted(cam.items())))
        if key not in _want:
            cfg = oracle.config(w, h, total, depth, frame_spp=frame_spp, **part, **cam)
            _want[key] = oracle.render(cfg, cpu_scene)
        return _want[key]

    out = []
    with vc.Renderer(desc, gpu_scene) as r:
        for f in range(nframes):
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
            what = f"{case} {cam} {desc_kw} frame {f}"
            part = oracle.partition(st)
            fs = spp if desc.progressive else 0
            img, segs = want((f + 1) * spp if desc.progressive else spp, part, fs)
            if world > 1:
                got, img = got.reshape(-1, 4)[m[..., 1][mine]], img[mine]
                cfg = oracle.config(w, h, spp, depth, **part, **cam)
                segs = oracle.render_pixels(cfg, cpu_scene, np.argwhere(mine)[:, ::-1])[1]
            elif desc.progressive and f > 0:
                segs -= want(f * spp, part, fs)[1]
            assert_same(got, img, what)
            assert st["segments"] == segs, what
            assert st["kernel"].endswith("_stats") == stats, what
            out.append(st)
    return out


# ---- the frames test_gpu_push_heavy.py pins: the parent's counts -----------------------------

@pytest.mark.parametrize("case,cost", [("final", False), ("final", True), ("tiny47", False),
                                       ("tiny55", False)])
def test_parent_counts(oracle, monkeypatch, case, cost):
    monkeypatch.delenv("VCRT_GROUP_FOOT", raising=False)
    monkeypatch.delenv("VCRT_DEBUG_STATS", raising=False)
    if cost:
        monkeypatch.setenv("VCRT_WORK_ORDER", "cost")
    else:
        monkeypatch.delenv("VCRT_WORK_ORDER", raising=False)
    st = PH.render(oracle, case, cost)  # image and segments against the oracle, every frame
    assert st["bound_tests"] == 0
    assert st["group_tests"] == PH.PARENT_GROUP_TESTS[case, cost]
    if not cost:  # the stats build renders in plain order
        ss = PH.stats_frame(oracle, monkeypatch, case)
        assert ss["segments"] == st["segments"]
        assert dbg(ss, "group_pass_entries") == PH.PARENT_STATS[case]


# ---- other frames ----------------------------------------------------------------------------

def test_grid12(oracle, monkeypatch):
    (st,) = frames(oracle, monkeypatch, ("grid12", 24, 16, 8, 8), cam=G.GRID_CAM)
    assert st["kernel"].startswith("vcrt_trace_cull_flat")


def test_progressive_two_frames(oracle, monkeypatch):
    s1, s2 = frames(oracle, monkeypatch, ("final", 44, 20, 4, 6), nframes=2, progressive=True)
    assert (s1["accumulated_spp"], s2["accumulated_spp"]) == (4, 8)


@pytest.mark.parametrize("rank", [0, 1])
def test_two_way_shard(oracle, monkeypatch, rank):
    frames(oracle, monkeypatch, ("final", 44, 20, 8, 6), rank=rank, world_size=2)


def test_lens_frame(oracle):
    sc = R.scene_of(oracle, "final")
    desc = vc.RenderDesc(width=24, height=16, samples_per_pixel=8, max_depth=6, device=0,
                         lens_radius=0.1)
    with vc.Renderer(desc, sc) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    want, segs = L.reference_frame(oracle, sc, desc)
    assert st["kernel"].startswith("vcrt_trace_cull_flat_lens")
    assert_same(got, want, "lens 24x16x8")
    assert st["segments"] == segs


# ---- the guards' other side ------------------------------------------------------------------

def test_centre_beyond_the_bound(oracle, monkeypatch):
    """Not kFlagSceneBounded: the host gives such a scene no tables, so no culled kernel runs."""
    (st,) = frames(oracle, monkeypatch, ("far_centre", 24, 16, 4, 6), variant=N.KERNEL_AUTO)
    assert "cull" not in st["kernel"]


def test_camera_beyond_the_bound(oracle, monkeypatch):
    """The camera centre fails |x| <= 2^30: the kernel gets no lists, no camera ray takes the fast
    trace, and a wave that holds a ray from the camera scans the whole list (kScanLinear)."""
    case = ("final", 24, 16, 4, 6)
    (st,) = frames(oracle, monkeypatch, case, cam=FAR_CAM)
    assert st["kernel"].startswith("vcrt_trace_cull_flat")
    # (not SB.stats_frames: its counter identities take a culled scan in every frame)
    (ss,) = frames(oracle, monkeypatch, case, cam=FAR_CAM, stats=True)
    assert region(ss, "kCam") == 0 and region(ss, "kScanLinear") > 0


def test_short_camera_rays(oracle, monkeypatch):
    """The tiny grid (coordinates scaled by 2^-24): its camera rays have dot(d, d) < 2^-20, so
    guard_a is false for them (no fast trace, kScanLinear) and true for the bounced rays (kScan)."""
    case = ("tiny", 24, 16, 2, 6)
    (st,) = frames(oracle, monkeypatch, case, cam=G.TINY_CAM)
    (ss,) = SB.stats_frames(oracle, monkeypatch, ("sliced",) + case[1:], *SB.FLAT, cam=G.TINY_CAM)
    assert ss["segments"] == st["segments"]
    assert region(ss, "kCam") == 0
    assert region(ss, "kScanLinear") > 0 and region(ss, "kScan") > 0


# ---- the drain -------------------------------------------------------------------------------

def test_drain_steals(oracle, monkeypatch):
    """One item of 16 quanta per pixel: once the queues are empty idle lanes take later quanta of
    the wave's longest item. The product frame is the oracle's; the stats build of the same frame
    counts the steal loop's trips."""
    case = ("final", 24, 16, 64, 6)
    kw = dict(accumulate_chunk=64, accumulate_quantum=4, accumulate_tail=-1)
    (st,) = frames(oracle, monkeypatch, case, **kw)
    (ss,) = SB.stats_frames(oracle, monkeypatch, case, *SB.FLAT, **kw)
    assert ss["segments"] == st["segments"]
    assert region(ss, "kSteal") > 0
    assert dbg(ss, "items_started") > 24 * 16  # some trip handed a range out
