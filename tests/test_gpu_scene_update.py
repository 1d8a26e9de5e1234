"""Moving spheres on the GPU (vcrt_update_spheres): the tables the refit kernels leave on the
device equal the host restatement of the refit byte for byte, and every frame and ray query after
an update equals a fresh renderer's and the oracle's bit for bit -- for each frame kernel, the
device variant, the host switch, the fallbacks, progressive frames, the thin lens and the camera.

Shapes: tests/test_gpu_camera_move.py's. Moves: tests/scene_update_ref.py's."""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import lens_ref as L
from tests import ray_query_ref as R
from tests import scene_update_ref as U
from tests.test_cull_cpu import INSIDE
from tests.test_gpu_camera_move import (DEFAULT, SHAPES, assert_lists_equal, desc_of, draw,
                                        scene_of)
from tests.test_gpu_lens import assert_same

pytestmark = pytest.mark.gpu
N = vc._native
S = vc.scene
SYMBOL = {"final44": "vcrt_trace_cull_flat", "final100r1": "vcrt_trace_cull_flat",
          "stress96": "vcrt_trace_cull_flat_boxes"}

_moved, _want, _fresh, _oracle = {}, {}, {}, {}


def moved_scene(oracle, shape, move):
    key = (SHAPES[shape][0], move)
    if key not in _moved:
        _moved[key] = U.MOVES[move](scene_of(oracle, shape))
    return _moved[key]


def want_tables(oracle, shape, move):
    """The host restatement of the refit; computed once per scene and move."""
    key = (SHAPES[shape][0], move)
    if key not in _want:
        _want[key] = U.tables(scene_of(oracle, shape), moved_scene(oracle, shape, move))
    return _want[key]


def device_tables(r):
    return {name: r.scene_table(name) for name in N.SCENE_TABLES}


def fresh(oracle, shape, move, cam=None, **kw):
    """(frame, stats) of a new renderer on the moved scene; cached."""
    key = (shape, move, tuple(sorted((cam or {}).items())), tuple(sorted(kw.items())))
    if key not in _fresh:
        with vc.Renderer(desc_of(shape, cam, **kw), moved_scene(oracle, shape, move)) as r:
            _fresh[key] = draw(r)
    return _fresh[key]


def assert_oracle(oracle, shape, move, got, st):
    """The oracle's frame of the moved scene (the whole frame, also for a shard)."""
    key = (shape, move, st["accumulate_quantum"])
    d = SHAPES[shape][1]
    if key not in _oracle:
        cfg = oracle.config(d["width"], d["height"], d["samples_per_pixel"], d["max_depth"],
                            **oracle.partition(st), **DEFAULT)
        _oracle[key] = oracle.render(cfg, moved_scene(oracle, shape, move))
    want, segs = _oracle[key]
    world, rank = d.get("world_size", 1), d.get("rank", 0)
    if world == 1:
        assert_same(got, want, f"{shape} {move} against the oracle")
        assert st["segments"] == segs
    else:
        m = vc.tile_pixel_map(d["width"], d["height"], world)
        mine = m[..., 0] == rank
        assert_same(got.reshape(-1, 4)[m[..., 1][mine]], want[mine],
                    f"{shape} {move} rank {rank} against the oracle")


def assert_fresh(oracle, shape, move, got, st, cam=None, **kw):
    want, want_st = fresh(oracle, shape, move, cam, **kw)
    assert_same(got, want, f"{shape} {move} against a fresh renderer")
    assert st["segments"] == want_st["segments"]


# ---- 1. the refitted tables are the host's ------------------------------------------------

@pytest.mark.parametrize("move", U.REFIT_MOVES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tables_equal_the_host_refit(oracle, shape, move):
    base, moved = scene_of(oracle, shape), moved_scene(oracle, shape, move)
    with vc.Renderer(desc_of(shape), base) as r:
        before = device_tables(r)
        r.update_spheres(moved)
        got, lists, us = device_tables(r), r.camera_lists(), r.scene_update_stats()
        _, st = draw(r)
    print(f"{shape} {move}: {us}")
    U.assert_tables_equal(before, want_tables(oracle, shape, "identity"), f"{shape} set_scene")
    U.assert_tables_equal(got, want_tables(oracle, shape, move), f"{shape} {move}")
    assert (us["on_device"], us["rebuilt"]) == (1, 0)
    sc = got["scalars"]
    assert us["groups"] == sc["nbig"] + sc["ngroups"] and us["refit_ms"] > 0.0
    if move == "identity":
        U.assert_tables_equal(got, before, f"{shape} identity against the tables before")
    else:
        assert any(not isinstance(got[k], dict) and got[k].tobytes() != before[k].tobytes()
                   for k in got if got[k] is not None)
    want_lists = S.refit_camera_lists(base, moved, desc_of(shape))
    assert_lists_equal(lists, want_lists, f"{shape} {move} lists")
    assert len(lists["group_info"]) == SHAPES[shape][2]
    # the kernel follows the kept grouping's size, whatever a regrouping would choose
    assert st["kernel"].startswith(SYMBOL[shape])


# ---- 2. frames after updates --------------------------------------------------------------

CHAIN = ["identity", "drift", "bounce", "resize", "swap", "identity"]


@pytest.mark.parametrize("variant,tables,symbol", [
    (N.KERNEL_AUTO, None, "vcrt_trace_cull_flat"),
    (N.KERNEL_SMEM, None, "vcrt_trace_smem"),
    (N.KERNEL_CULL_LANE, None, "vcrt_trace_cull_lane"),
    (N.KERNEL_CULL_FLAT, None, "vcrt_trace_cull_flat"),
    (N.KERNEL_CULL_FLAT, "global", "vcrt_trace_cull_flat_global"),
])
def test_chain_of_updates(oracle, monkeypatch, variant, tables, symbol):
    if tables:
        monkeypatch.setenv("VCRT_CULL_LANE_TABLES", tables)
    shape = "final44"
    frames = []
    with vc.Renderer(desc_of(shape, kernel_variant=variant), scene_of(oracle, shape)) as r:
        for k, move in enumerate(CHAIN):
            if k > 0:
                r.update_spheres(moved_scene(oracle, shape, move))
                us = r.scene_update_stats()
                assert (us["on_device"], us["rebuilt"]) == (1, 0)
            frames.append(draw(r))
    for move, (got, st) in zip(CHAIN, frames):
        assert_fresh(oracle, shape, move, got, st, kernel_variant=variant)
        assert st["kernel"].startswith(symbol)
        assert_oracle(oracle, shape, move, got, st)
    assert_same(frames[-1][0], frames[0][0], "back at the first scene")
    for a, b in zip(frames, frames[1:]):
        assert (a[0].view(np.uint32) != b[0].view(np.uint32)).any()


@pytest.mark.parametrize("shape,move", [("final100r1", "bounce"), ("stress96", "drift")])
def test_update_at_the_other_shapes(oracle, shape, move):
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        r.update_spheres(moved_scene(oracle, shape, move))
        got, st = draw(r)
    assert_fresh(oracle, shape, move, got, st)
    assert st["kernel"].startswith(SYMBOL[shape])
    assert_oracle(oracle, shape, move, got, st)


# ---- 3. the device variant ------------------------------------------------------------------

def test_device_variant(oracle, monkeypatch):
    import torch
    shape, move = "final44", "drift"
    moved = moved_scene(oracle, shape, move)
    flat = np.ascontiguousarray(moved).view(np.float32).reshape(-1, 10)
    t = torch.from_numpy(flat.copy()).to("cuda:0")
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        with pytest.raises(ValueError):
            r.update_spheres(t[:, :9])
        r.update_spheres(t)
        tables, us = device_tables(r), r.scene_update_stats()
        got, st = draw(r)
        # h_spheres is true: the host list builders of a camera move read it
        monkeypatch.setenv("VCRT_CAMERA_LISTS", "host")
        r.set_camera(**INSIDE)
        assert r.camera_stats()["on_device"] == 0
        got_in, st_in = draw(r)
    monkeypatch.delenv("VCRT_CAMERA_LISTS")
    assert (us["on_device"], us["rebuilt"]) == (1, 0)
    U.assert_tables_equal(tables, want_tables(oracle, shape, move), "device variant")
    assert_fresh(oracle, shape, move, got, st)
    assert_fresh(oracle, shape, move, got_in, st_in, cam=INSIDE)


# ---- 4. the host switch ---------------------------------------------------------------------

def test_host_switch(oracle, monkeypatch):
    shape, move = "final44", "resize"
    monkeypatch.setenv("VCRT_SCENE_UPDATE", "host")
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        r.update_spheres(moved_scene(oracle, shape, move))
        tables, us = device_tables(r), r.scene_update_stats()
        got, st = draw(r)
    assert (us["on_device"], us["rebuilt"], us["refit_ms"]) == (0, 0, 0.0)
    U.assert_tables_equal(tables, want_tables(oracle, shape, move), "host switch")
    assert_fresh(oracle, shape, move, got, st)


# ---- 5. fallbacks ---------------------------------------------------------------------------

def test_unbounded_rebuilds_and_a_bounded_update_refits_again(oracle):
    shape = "final44"
    base = scene_of(oracle, shape)
    fresh(oracle, shape, "unbounded")  # (a new renderer would retire the one below)
    with vc.Renderer(desc_of(shape), base) as r:
        r.update_spheres(moved_scene(oracle, shape, "unbounded"))
        us = r.scene_update_stats()
        got, st = draw(r)
        assert (us["on_device"], us["rebuilt"]) == (0, 1)
        assert r.scene_table("groups") is None
        assert_fresh(oracle, shape, "unbounded", got, st)
        assert st["kernel"].startswith("vcrt_trace_smem")
        # no tables now: the next update rebuilds them; the one after refits
        r.update_spheres(base)
        assert r.scene_update_stats()["rebuilt"] == 1
        r.update_spheres(moved_scene(oracle, shape, "drift"))
        us = r.scene_update_stats()
        assert (us["on_device"], us["rebuilt"]) == (1, 0)
        U.assert_tables_equal(device_tables(r), want_tables(oracle, shape, "drift"), "refit again")
        got, st = draw(r)
    assert_fresh(oracle, shape, "drift", got, st)


def test_device_variant_unbounded_rebuilds(oracle):
    import torch
    shape = "final44"
    moved = moved_scene(oracle, shape, "unbounded")
    t = torch.from_numpy(np.ascontiguousarray(moved).view(np.float32).reshape(-1, 10).copy())
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        r.update_spheres(t.to("cuda:0"))
        us = r.scene_update_stats()
        got, st = draw(r)
    assert (us["on_device"], us["rebuilt"]) == (0, 1)
    assert_fresh(oracle, shape, "unbounded", got, st)


def test_small_scene_and_wrong_count(oracle):
    shape = "final44"
    three = R.scene_of(oracle, "three")
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        first, _ = draw(r)
        with pytest.raises(N.VcrtError) as e:
            r.update_spheres(three)
        assert e.value.code == N.VK_ERROR_FORMAT_NOT_SUPPORTED
        again, _ = draw(r)
        assert_same(again, first, "the frame after a refused update")
        r.set_scene(three)
        moved = three.copy()
        moved["center"][:, 0] += np.float32(0.25)
        r.update_spheres(moved)
        assert r.scene_update_stats()["rebuilt"] == 1
        got, st = draw(r)
    with vc.Renderer(desc_of(shape), moved) as r:
        want, want_st = draw(r)
    assert_same(got, want, "four spheres moved")
    assert st["segments"] == want_st["segments"]


# ---- 6. interplay ---------------------------------------------------------------------------

def test_progressive_restarts(oracle):
    shape, move = "final44", "drift"
    kw = dict(samples_per_pixel=4, progressive=True)
    with vc.Renderer(desc_of(shape, **kw), scene_of(oracle, shape)) as r:
        draw(r)
        _, s2 = draw(r)
        r.update_spheres(moved_scene(oracle, shape, move))
        got, st = draw(r)
    assert s2["accumulated_spp"] == 8 and st["accumulated_spp"] == 4
    assert_fresh(oracle, shape, move, got, st, **kw)


def test_lens(oracle):
    shape, move = "final44", "drift"
    moved = moved_scene(oracle, shape, move)
    with vc.Renderer(desc_of(shape, lens_radius=0.1), scene_of(oracle, shape)) as r:
        draw(r)
        r.update_spheres(moved)
        lists, us = r.camera_lists(), r.scene_update_stats()
        got, st = draw(r)
    assert all(len(v) == 0 for v in lists.values())
    assert (us["on_device"], us["rebuilt"], us["lists_ms"]) == (1, 0, 0.0)
    want, segs = L.reference_frame(oracle, moved, desc_of(shape, lens_radius=0.1))
    assert_same(got, want, "lens frame after an update")
    assert st["segments"] == segs


def test_camera_and_update_in_either_order(oracle):
    shape, move = "final44", "swap"
    moved = moved_scene(oracle, shape, move)
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        r.update_spheres(moved)
        r.set_camera(**INSIDE)
        a, sa = draw(r)
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        r.set_camera(**INSIDE)
        r.update_spheres(moved)
        lists = r.camera_lists()
        b, sb = draw(r)
    assert_fresh(oracle, shape, move, a, sa, cam=INSIDE)
    assert_fresh(oracle, shape, move, b, sb, cam=INSIDE)
    assert_lists_equal(lists, S.refit_camera_lists(scene_of(oracle, shape), moved,
                                                   desc_of(shape, INSIDE)), "update after move")


def test_queries_after_an_update(oracle):
    shape, move = "final44", "drift"
    O, D = R.ray_batch(oracle)[:2]
    ok = R.finite_rays(O, D)
    O, D = O[ok][:2048], D[ok][:2048]
    moved = moved_scene(oracle, shape, move)
    with vc.Renderer(desc_of(shape), scene_of(oracle, shape)) as r:
        rad0 = r.trace_rays(O, D, 6)
        r.update_spheres(moved)
        rad1, hit1 = r.trace_rays(O, D, 6, hits=True)
        occ1 = r.occluded(O, D, 5.0)
    with vc.Renderer(desc_of(shape), moved) as r:
        rad2, hit2 = r.trace_rays(O, D, 6, hits=True)
        occ2 = r.occluded(O, D, 5.0)
    assert_same(rad1, rad2, "trace_rays after an update")
    assert hit1.tobytes() == hit2.tobytes() and np.array_equal(occ1, occ2)
    assert occ1.any() and not occ1.all()
    assert (rad0.view(np.uint32) != rad1.view(np.uint32)).any()


def test_set_scene_after_updates(oracle):
    shape = "final44"
    base = scene_of(oracle, shape)
    with vc.Renderer(desc_of(shape), base) as r:
        r.update_spheres(moved_scene(oracle, shape, "swap"))
        r.update_spheres(moved_scene(oracle, shape, "bounce"))
        r.set_scene(base)
        tables = device_tables(r)
        got, st = draw(r)
    U.assert_tables_equal(tables, want_tables(oracle, shape, "identity"), "set_scene after updates")
    assert_fresh(oracle, shape, "identity", got, st)
