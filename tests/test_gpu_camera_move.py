"""The moving camera on the GPU (vcrt_set_camera): the camera-ray lists the device builds equal
the host builders' word for word, and every frame after a move equals a fresh renderer's and
the oracle's bit for bit -- for each frame kernel, progressive frames, the thin lens, a shard, a
scene change after the move, degenerate cameras and the command line's --orbit.

Shapes: the final scene at 44x20x8 (both edges partial, two quanta of the rule's G = 4), the
final scene at 100x52 as rank 1 of 3, and stress4096 at 96x56x4 (17 chunks, the boxes-in-LDS
kernel). Cameras: tests/test_cull_cpu.py's."""
import math
import os
import subprocess

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import lens_ref as L
from tests import ray_query_ref as R
from tests.test_cull_cpu import DOWN, INSIDE
from tests.test_gpu_lens import assert_same

pytestmark = pytest.mark.gpu
N = vc._native

DEFAULT = dict(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vfov=20)
ORBIT = dict(lookfrom=(-9, 3, 10), lookat=(0, 0.5, 0), vfov=30)
CAMERAS = {"default": DEFAULT, "inside": INSIDE, "down": DOWN, "orbit": ORBIT}
NONE = 15

# name -> (scene, RenderDesc keywords, quarters = 4 x local tiles)
SHAPES = {
    "final44": ("final", dict(width=44, height=20, samples_per_pixel=8, max_depth=6), 72),
    "final100r1": ("final", dict(width=100, height=52, samples_per_pixel=4, max_depth=4, rank=1,
                                 world_size=3), 120),
    "stress96": ("stress4096", dict(width=96, height=56, samples_per_pixel=4, max_depth=4), 336),
}


def desc_of(shape, cam=None, **kw):
    base = dict(SHAPES[shape][1], device=0)
    base.update(cam or {})
    base.update(kw)
    return vc.RenderDesc(**base)


def scene_of(oracle, shape):
    return R.scene_of(oracle, SHAPES[shape][0])


def draw(r):
    r.draw_next_frame()
    return r.read_framebuffer(), r.stats()


_fresh = {}


def fresh(oracle, shape, cam_name, cam=None, **kw):
    """(frame, stats) of a new renderer with that camera; cached per configuration."""
    key = (shape, cam_name, tuple(sorted(kw.items())), tuple(sorted(
        (k, os.environ.get(k)) for k in ("VCRT_CULL_LANE_TABLES", "VCRT_CAMERA_LISTS"))))
    if key not in _fresh:
        with vc.Renderer(desc_of(shape, cam or CAMERAS[cam_name], **kw),
                         scene_of(oracle, shape)) as r:
            _fresh[key] = draw(r)
    return _fresh[key]


_oracle_frames = {}


def oracle_frame(oracle, shape, cam_name, st):
    """The oracle's frame for a shape and camera (the whole frame, also for a shard)."""
    key = (shape, cam_name, st["accumulate_quantum"])
    if key not in _oracle_frames:
        d = SHAPES[shape][1]
        cfg = oracle.config(d["width"], d["height"], d["samples_per_pixel"], d["max_depth"],
                            **oracle.partition(st), **CAMERAS[cam_name])
        _oracle_frames[key] = oracle.render(cfg, scene_of(oracle, shape))
    return _oracle_frames[key]


def assert_oracle(oracle, shape, cam_name, got, st):
    want, segs = oracle_frame(oracle, shape, cam_name, st)
    d = SHAPES[shape][1]
    world, rank = d.get("world_size", 1), d.get("rank", 0)
    if world == 1:
        assert_same(got, want, f"{shape} {cam_name} against the oracle")
        assert st["segments"] == segs
    else:  # the shard's packed tiles against its pixels of the whole frame
        m = vc.tile_pixel_map(d["width"], d["height"], world)
        mine = m[..., 0] == rank
        assert_same(got.reshape(-1, 4)[m[..., 1][mine]], want[mine],
                    f"{shape} {cam_name} rank {rank} against the oracle")


def host_lists(oracle, shape, cam):
    sc, d = scene_of(oracle, shape), desc_of(shape, cam)
    g, s = vc.scene.primary_lists(sc, d), vc.scene.primary_sphere_lists(sc, d)
    return {"group_info": g["info"], "ids": g["ids"], "sphere_info": s["info"],
            "rec": np.asarray(s["rec"], np.float32).reshape(-1, 12)}


def assert_lists_equal(got, want, what):
    for key in ("group_info", "ids", "sphere_info"):
        assert got[key].shape == want[key].shape, f"{what}: {key} sizes differ"
        assert np.array_equal(got[key], want[key]), f"{what}: {key} differs"
    assert got["rec"].shape == want["rec"].shape, f"{what}: rec sizes differ"
    a, b = got["rec"].view(np.uint32), want["rec"].view(np.uint32)
    assert np.array_equal(a, b), f"{what}: rec differs in {int((a != b).sum())} words"


# ---- 1. the device-built lists are the host's --------------------------------------------------

def any_none(lists):
    return bool((lists["group_info"] == NONE).any() or (lists["sphere_info"] == NONE).any())


@pytest.mark.parametrize("cam_name", list(CAMERAS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_lists_equal_the_host_builders(oracle, shape, cam_name):
    cam = CAMERAS[cam_name]
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        # straight after vcrt_begin: the host-built lists of the default camera
        assert_lists_equal(r.camera_lists(), host_lists(oracle, shape, DEFAULT), "after begin")
        assert r.camera_stats()["on_device"] == 0
        r.set_camera(**cam)
        got, cs = r.camera_lists(), r.camera_stats()
    want = host_lists(oracle, shape, cam)
    n = SHAPES[shape][2]
    print(f"{shape} {cam_name}: {cs}")
    assert cs["on_device"] == 1
    assert (cs["quarters"], cs["group_ids"], cs["pair_records"]) == (
        n, len(want["ids"]), len(want["rec"]))
    assert len(want["group_info"]) == n
    assert_lists_equal(got, want, f"{shape} {cam_name}")
    # not vacuous: listed non-empty quarters of each kind ...
    for key in ("group_info", "sphere_info"):
        info = want[key]
        assert ((info != NONE) & ((info & 15) > 0)).any(), key
    # ... and quarters without a list: the default camera has them at every shape. (The camera
    # looking down lists every quarter of the two larger frames; there the equal infos say all.)
    assert any_none(host_lists(oracle, shape, DEFAULT))
    if cam_name != "down":
        assert any_none(want)


# ---- 2. frames after a move: a fresh renderer's and the oracle's ------------------------------

CHAIN = ["default", "inside", "down", "default"]


@pytest.mark.parametrize("variant,tables,symbol", [
    (N.KERNEL_AUTO, None, "vcrt_trace_cull_flat"),
    (N.KERNEL_SMEM, None, "vcrt_trace_smem"),
    (N.KERNEL_CULL_LANE, None, "vcrt_trace_cull_lane"),
    (N.KERNEL_CULL_FLAT, None, "vcrt_trace_cull_flat"),
    (N.KERNEL_CULL_FLAT, "global", "vcrt_trace_cull_flat_global"),
])
def test_chain_of_moves(oracle, monkeypatch, variant, tables, symbol):
    if tables:
        monkeypatch.setenv("VCRT_CULL_LANE_TABLES", tables)
    shape = "final44"
    frames = []
    with vc.Renderer(desc_of(shape, kernel_variant=variant), scene_of(oracle, shape)) as r:
        for k, cam_name in enumerate(CHAIN):
            if k > 0:
                r.set_camera(**CAMERAS[cam_name])
                assert r.camera_stats()["on_device"] == 1
            frames.append(draw(r))
    for cam_name, (got, st) in zip(CHAIN, frames):
        want, want_st = fresh(oracle, shape, cam_name, kernel_variant=variant)
        assert_same(got, want, f"{cam_name} against a fresh renderer")
        assert st["segments"] == want_st["segments"]
        assert st["kernel"] == want_st["kernel"]
        assert st["kernel"].startswith(symbol)
        assert_oracle(oracle, shape, cam_name, got, st)
    assert_same(frames[3][0], frames[0][0], "back at the first camera")
    assert (frames[1][0].view(np.uint32) != frames[0][0].view(np.uint32)).any()


@pytest.mark.parametrize("shape,cam_name,symbol", [
    ("final100r1", "orbit", "vcrt_trace_cull_flat"),
    ("final100r1", "down", "vcrt_trace_cull_flat"),
    ("stress96", "inside", "vcrt_trace_cull_flat_boxes"),
    ("stress96", "orbit", "vcrt_trace_cull_flat_boxes"),
])
def test_move_at_the_other_shapes(oracle, shape, cam_name, symbol):
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        first = draw(r)
        r.set_camera(**CAMERAS[cam_name])
        got, st = draw(r)
    want, want_st = fresh(oracle, shape, cam_name)
    assert_same(got, want, f"{shape} {cam_name} against a fresh renderer")
    assert (st["segments"], st["kernel"]) == (want_st["segments"], want_st["kernel"])
    assert st["kernel"].startswith(symbol)
    assert_oracle(oracle, shape, cam_name, got, st)
    assert_oracle(oracle, shape, "default", *first)


# ---- 3. the host builders behind the same call -------------------------------------------------

def test_host_switch(oracle, monkeypatch):
    shape = "final44"
    monkeypatch.setenv("VCRT_CAMERA_LISTS", "host")
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        r.set_camera(**INSIDE)
        lists, cs = r.camera_lists(), r.camera_stats()
        got, st = draw(r)
    assert cs["on_device"] == 0 and cs["lists_ms"] == 0.0 and cs["quarters"] == 72
    assert_lists_equal(lists, host_lists(oracle, shape, INSIDE), "host switch")
    monkeypatch.delenv("VCRT_CAMERA_LISTS")
    want, want_st = fresh(oracle, shape, "inside")
    assert_same(got, want, "host switch against a fresh renderer")
    assert (st["segments"], st["kernel"]) == (want_st["segments"], want_st["kernel"])


# ---- 4. progressive ----------------------------------------------------------------------------

def test_progressive_restarts(oracle):
    shape = "final44"
    kw = dict(samples_per_pixel=4, progressive=True)
    with vc.Renderer(desc_of(shape, **kw), scene_of(oracle, shape)) as r:
        draw(r)
        _, s2 = draw(r)
        r.set_camera(**INSIDE)
        got, st = draw(r)
    assert s2["accumulated_spp"] == 8 and st["accumulated_spp"] == 4
    want, want_st = fresh(oracle, shape, "inside", **kw)
    assert_same(got, want, "first progressive frame after a move")
    assert st["segments"] == want_st["segments"]


# ---- 5. the thin lens --------------------------------------------------------------------------

def test_lens(oracle):
    shape, sc = "final44", scene_of(oracle, "final44")
    with vc.Renderer(desc_of(shape, lens_radius=0.1), sc) as r:
        draw(r)
        r.set_camera(**INSIDE)
        lists, cs = r.camera_lists(), r.camera_stats()
        got, st = draw(r)
    assert all(len(v) == 0 for v in lists.values())
    assert (cs["on_device"], cs["quarters"]) == (0, 0)
    want, segs = L.reference_frame(oracle, sc, desc_of(shape, INSIDE, lens_radius=0.1))
    assert_same(got, want, "lens frame after a move")
    assert st["segments"] == segs
    assert st["kernel"].startswith("vcrt_trace_cull_flat_lens")


# ---- 6. a scene after the camera ---------------------------------------------------------------

def test_scene_after_camera(oracle):
    shape = "final44"
    three = R.scene_of(oracle, "three")
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        r.set_camera(**INSIDE)
        r.set_scene(three)
        assert len(r.camera_lists()["group_info"]) == 0   # no tables: no lists
        got3, st3 = draw(r)
        r.set_scene(scene_of(oracle, shape))
        lists = r.camera_lists()
        gotf, stf = draw(r)
    with vc.Renderer(desc_of(shape, INSIDE), three) as r:
        want3, want_st3 = draw(r)
    assert_same(got3, want3, "three spheres after the move")
    assert (st3["segments"], st3["kernel"]) == (want_st3["segments"], want_st3["kernel"])
    wantf, want_stf = fresh(oracle, shape, "inside")
    assert_same(gotf, wantf, "final scene after the move")
    assert (stf["segments"], stf["kernel"]) == (want_stf["segments"], want_stf["kernel"])
    assert_lists_equal(lists, host_lists(oracle, shape, INSIDE), "set_scene after the move")


# ---- 7. edge cameras (valid inputs: vcrt_begin takes them too) --------------------------------

@pytest.mark.parametrize("name,cam", [
    ("lookfrom_is_lookat", dict(lookfrom=(1, 1, 1), lookat=(1, 1, 1), vfov=20)),
    ("far_away", dict(lookfrom=(3e30, 0, 0), lookat=(0, 0, 0), vfov=20)),
])
@pytest.mark.parametrize("shape", ["final44", "stress96"])
def test_edge_cameras(oracle, shape, name, cam):
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        r.set_camera(**cam)
        lists, cs = r.camera_lists(), r.camera_stats()
        got, st = draw(r)
    assert cs["on_device"] == 1 and (cs["group_ids"], cs["pair_records"]) == (0, 0)
    assert (lists["group_info"] == NONE).all() and (lists["sphere_info"] == NONE).all()
    assert len(lists["group_info"]) == SHAPES[shape][2]
    assert_lists_equal(lists, host_lists(oracle, shape, cam), f"{shape} {name}")
    want, want_st = fresh(oracle, shape, name, cam)
    assert_same(got, want, f"{shape} {name} against a fresh renderer")
    assert (st["segments"], st["kernel"]) == (want_st["segments"], want_st["kernel"])


# ---- 8. queries do not depend on the camera ----------------------------------------------------

def test_queries_unaffected(oracle):
    shape = "final44"
    O, D = R.ray_batch(oracle)[:2]
    ok = R.finite_rays(O, D)
    O, D = O[ok][:2048], D[ok][:2048]
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        rad0, hit0 = r.trace_rays(O, D, 6, hits=True)
        occ0 = r.occluded(O, D, 5.0)
        r.set_camera(**DOWN)
        rad1, hit1 = r.trace_rays(O, D, 6, hits=True)
        occ1 = r.occluded(O, D, 5.0)
    assert len(rad0) == len(O) and occ0.any() and not occ0.all()
    assert_same(rad1, rad0, "trace_rays after a move")
    assert hit0.tobytes() == hit1.tobytes()
    assert np.array_equal(occ0, occ1)


# ---- 9. the command line -----------------------------------------------------------------------

def test_cli_orbit(oracle, tmp_path):
    from tests.test_gpu_configs import read_pfm
    shape, deg = "final44", 30.0
    d = SHAPES[shape][1]
    th = 1 * deg * math.pi / 180.0
    lf, la = DEFAULT["lookfrom"], DEFAULT["lookat"]
    dx, dz = float(lf[0]) - la[0], float(lf[2]) - la[2]
    cam = dict(lookfrom=(float(np.float32(la[0] + dx * math.cos(th) + dz * math.sin(th))), lf[1],
                         float(np.float32(la[2] - dx * math.sin(th) + dz * math.cos(th)))),
               lookat=la, vfov=20)
    want, want_st = fresh(oracle, shape, "cli_orbit", cam)
    out = tmp_path / "orbit.pfm"
    cmd = [os.path.join(N.BIN_DIR, "vcrt_render"), "--scene", "final", "--width", str(d["width"]),
           "--height", str(d["height"]), "--spp", str(d["samples_per_pixel"]), "--depth",
           str(d["max_depth"]), "--frames", "2", "--orbit", str(deg), "--out", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip().endswith(f"{want_st['segments']} segments")
    assert_same(read_pfm(out), want[..., :3], "vcrt_render --orbit")
    first, _ = fresh(oracle, shape, "default")
    assert (read_pfm(out).view(np.uint32) != first[..., :3].view(np.uint32)).any()
