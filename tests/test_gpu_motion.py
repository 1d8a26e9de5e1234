"""The reprojection map on the GPU (vcrt_draw_motion, Renderer.draw_motion): bit parity of both
planes with tests/motion_ref on scenes that take each of the kernel's routes, for a static view,
an orbit, an orbit with moved spheres and a previous camera that looks away, one GPU and a shard's
packed tiles; independence of the route and of a lens; agreement with the ray queries; the state
changes; no effect on frames; the forms of the call and the calls it refuses."""
import ctypes
import math

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import features_ref as FR
from tests import motion_ref as M
from tests import ray_query_ref as R

pytestmark = pytest.mark.gpu
N = vc._native
F = np.float32

W, H = 44, 20  # both edges partial: 6 x 3 tiles
PLANES = ("motion", "surface")
SENTINEL = F(-77.5)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def desc_of(**kw):
    base = dict(width=W, height=H, samples_per_pixel=4, max_depth=3, device=0)
    base.update(kw)
    return vc.RenderDesc(**base)


def orbit(desc, degrees):
    """desc's camera turned about the y axis through lookat (in double, rounded to float)."""
    th = math.radians(degrees)
    dx, dz = desc.lookfrom[0] - desc.lookat[0], desc.lookfrom[2] - desc.lookat[2]
    return desc.with_camera(lookfrom=(
        float(F(desc.lookat[0] + dx * math.cos(th) + dz * math.sin(th))), desc.lookfrom[1],
        float(F(desc.lookat[2] - dx * math.sin(th) + dz * math.cos(th)))))


def shifted(scene):
    """Every sphere but the ground moved by 0.05 in x and -0.05 in z."""
    out = scene.copy()
    i = np.flatnonzero(np.abs(scene["radius"]) < 100)
    out["center"][i, 0] += F(0.05)
    out["center"][i, 2] -= F(0.05)
    return out


def previous(kind, desc, scene):
    """(prev_desc, prev_scene) of a case; None: the current one."""
    if kind == "same":
        return None, None
    if kind == "orbit":
        return orbit(desc, 3.0), None
    if kind == "orbit-moved":
        return orbit(desc, 3.0), shifted(scene)
    if kind == "away":
        away = tuple(2 * a - b for a, b in zip(desc.lookfrom, desc.lookat))
        return desc.with_camera(lookat=away), None
    raise KeyError(kind)


def same(got, want, what=""):
    for k in PLANES:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, f"{what}: {k} differs at {bad[:6].tolist()} ({len(bad)} words)"


def draw_packed(r, prev_desc, prev_scene):
    """vcrt_draw_motion into sentinel-filled planes of the rank-local layout (the C ABI itself:
    the Python method hands out fresh arrays)."""
    elems, tiles = r.local_layout()
    out = {k: np.full((tiles, 64, 4), SENTINEL, F) for k in PLANES}
    st = N.vcrt_motion_stats()
    cam = None if prev_desc is None else ctypes.byref(prev_desc.to_c().camera)
    arr = None if prev_scene is None else np.ascontiguousarray(prev_scene)
    N.check("vcrt_draw_motion", N.lib().vcrt_draw_motion(
        cam, None if arr is None else arr.ctypes.data, 0 if arr is None else len(arr),
        out["motion"].ctypes.data, out["surface"].ctypes.data, ctypes.byref(st)))
    return out, st


@pytest.mark.parametrize("kind", ["same", "orbit", "orbit-moved", "away"])
@pytest.mark.parametrize("scene", ["three", "final", "stress4096"])
def test_parity_with_the_reference(oracle, scene, kind):
    sc = R.scene_of(oracle, scene)
    desc = desc_of()
    pd, ps = previous(kind, desc, sc)
    want = M.frame_motion(oracle, sc, desc, pd, ps)
    with vc.Renderer(desc, sc) as r:
        got = r.draw_motion(prev_camera=pd, prev_spheres=ps, stats=True)
    st = got.pop("stats")
    same(got, want, f"{scene} {kind} world 1")
    assert st["rays"] == W * H and st["kernel"] == "vcrt_frame_motion"
    assert st["hit_rays"] == want["hit"] and 0 < st["hit_rays"] < st["rays"]
    assert st["projected"] == want["projected"] and st["identity"] == want["identity"]
    assert st["group_tests"] > 0 and st["kernel_ms"] > 0 and st["host_ms"] >= st["kernel_ms"]
    if kind == "same":
        assert st["identity"] == st["rays"] == st["projected"]  # a static view: all identity
        y, x = np.mgrid[0:H, 0:W]
        assert np.array_equal(got["motion"][..., 0], x) and np.array_equal(got["motion"][..., 1], y)
    elif kind == "away":
        assert st["projected"] < st["rays"] and st["identity"] == 0
        assert (got["motion"][..., 3] == 0).any()
    else:
        assert st["identity"] == 0 and st["projected"] > st["rays"] // 2
    if scene == "three":
        assert st["listed_rays"] == 0 and st["bound_tests"] == 0  # four spheres have no tables
    elif scene == "final":
        assert 0 < st["listed_rays"] <= st["rays"]
    # rank 1 of 3: packed tiles, the slots outside the frame untouched
    with vc.Renderer(desc_of(world_size=3, rank=1), sc) as r:
        got3, st3 = draw_packed(r, pd, ps)
    want3 = {k: FR.packed(want[k], W, H, 3, 1, SENTINEL) for k in PLANES}
    same(got3, want3, f"{scene} {kind} rank 1 of 3")
    valid = int((want3["surface"][..., 0] != SENTINEL).sum())
    assert 0 < valid < want3["surface"][..., 0].size and st3.rays == valid


@pytest.mark.parametrize("scene", ["final", "stress4096"])
def test_route_independence(oracle, scene, monkeypatch):
    sc = R.scene_of(oracle, scene)
    pd, ps = previous("orbit-moved", desc_of(), sc)
    with vc.Renderer(desc_of(), sc) as r:
        lists = r.draw_motion(pd, ps, stats=True)
    monkeypatch.setenv("VCRT_FEATURE_LISTS", "0")
    with vc.Renderer(desc_of(), sc) as r:
        scans = r.draw_motion(pd, ps, stats=True)
    same(scans, lists, scene)
    assert lists["stats"]["listed_rays"] > 0 and scans["stats"]["listed_rays"] == 0
    assert scans["stats"]["bound_tests"] > lists["stats"]["bound_tests"]


@pytest.mark.parametrize("kind", ["same", "orbit-moved"])
def test_a_lens_renderer_gives_the_pinholes_planes(oracle, kind):
    sc = R.scene_of(oracle, "final")
    pd, ps = previous(kind, desc_of(), sc)
    with vc.Renderer(desc_of(), sc) as r:
        pin = r.draw_motion(pd, ps)
    with vc.Renderer(desc_of(lens_radius=0.1), sc) as r:
        lens = r.draw_motion(pd, ps, stats=True)
    same(lens, pin, kind)
    assert lens["stats"]["listed_rays"] == 0  # a lens renderer has no lists


@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_host_and_device_forms_agree(oracle, world, rank):
    import torch
    sc = R.scene_of(oracle, "final")
    pd, ps = previous("orbit-moved", desc_of(), sc)
    with vc.Renderer(desc_of(world_size=world, rank=rank), sc) as r:
        host = r.draw_motion(pd, ps)
        dev = r.draw_motion(pd, ps, device=True, stats=True)
        # the caller's own 40-byte records on the device
        t = torch.from_numpy(np.ascontiguousarray(ps).view(F).reshape(-1, 10).copy()).cuda()
        rec = r.draw_motion(pd, t)
        mine = int((vc.tile_pixel_map(W, H, world)[..., 0] == rank).sum())
        assert dev["stats"]["rays"] == mine
        for k in PLANES:
            assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda
            assert np.array_equal(bits(dev[k].cpu().numpy()), bits(host[k])), k
            assert np.array_equal(bits(rec[k].cpu().numpy()), bits(host[k])), k
        # either plane alone
        lib = N.lib()
        only = torch.full_like(dev["motion"], -1.0)
        assert lib.vcrt_draw_motion_device(None, None, 0, only.data_ptr(), None, None) == 0
        again = torch.full_like(dev["surface"], -1.0)
        assert lib.vcrt_draw_motion_device(None, None, 0, None, again.data_ptr(), None) == 0
        if world == 1:
            assert np.array_equal(bits(again.cpu().numpy()), bits(host["surface"]))
            assert (only[..., 3] >= 1).all()


def test_agreement_with_the_ray_queries(oracle):
    desc = desc_of()
    o, d = M.centre_rays(oracle, desc)
    D = np.ascontiguousarray(d.reshape(-1, 3))
    O = np.ascontiguousarray(np.broadcast_to(o, D.shape))
    with vc.Renderer(desc, "final") as r:
        got = r.draw_motion()
        _, hits = r.trace_rays(O, D, max_depth=1, hits=True)
    assert np.array_equal((got["surface"][..., 0].ravel() - 2).astype(np.int32), hits["sphere"])
    t = np.where(hits["sphere"] >= 0, hits["t"], F(0))
    assert np.array_equal(bits(got["surface"][..., 1].ravel()), bits(t))
    assert not got["surface"][..., 2:].any()


def test_after_set_camera_and_update_spheres(oracle):
    """The editor's loop: the view and the spheres move, the old state is passed in."""
    sc = R.scene_of(oracle, "final")
    old_desc, old_sc = desc_of(), sc
    new_desc, new_sc = orbit(old_desc, -3.0), shifted(sc)
    want = M.frame_motion(oracle, new_sc, new_desc, old_desc, old_sc)
    with vc.Renderer(old_desc, old_sc) as r:
        first = r.draw_motion()
        r.set_camera(lookfrom=new_desc.lookfrom)
        r.update_spheres(new_sc)
        got = r.draw_motion(prev_camera=old_desc, prev_spheres=old_sc, stats=True)
        still = r.draw_motion(stats=True)
    same(got, want, "after set_camera and update_spheres")
    assert got["stats"]["identity"] == 0 and got["stats"]["listed_rays"] > 0
    assert still["stats"]["identity"] == W * H
    assert not np.array_equal(bits(first["surface"]), bits(got["surface"]))
    # only the ground stayed: with the same camera its pixels and the sky's are identity
    with vc.Renderer(new_desc, new_sc) as r:
        part = r.draw_motion(prev_spheres=old_sc, stats=True)
    want = M.frame_motion(oracle, new_sc, new_desc, None, old_sc)
    same(part, want, "the same camera, moved spheres")
    assert 0 < part["stats"]["identity"] == want["identity"] < W * H


@pytest.mark.parametrize("progressive", [False, True])
def test_frames_are_left_alone(oracle, progressive):
    desc = desc_of(progressive=progressive, max_depth=8)
    pd, ps = previous("orbit-moved", desc, R.scene_of(oracle, "final"))
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        a, sa = r.read_framebuffer(), r.stats()
        r.draw_next_frame()
        b, sb = r.read_framebuffer(), r.stats()
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        r.draw_motion(pd, ps)
        assert np.array_equal(bits(r.read_framebuffer()), bits(a))  # the framebuffer untouched
        s = r.stats()
        assert (s["segments"], s["frames"], s["kernel"]) == (sa["segments"], 1, sa["kernel"])
        r.draw_next_frame()
        assert np.array_equal(bits(r.read_framebuffer()), bits(b))
        s = r.stats()
        assert (s["segments"], s["accumulated_spp"]) == (sb["segments"], sb["accumulated_spp"])
    if progressive:
        assert not np.array_equal(bits(a), bits(b))


def test_refused_calls(oracle):
    import torch
    lib = N.lib()
    INIT, FORMAT = N.VK_ERROR_INITIALIZATION_FAILED, N.VK_ERROR_FORMAT_NOT_SUPPORTED
    sc = np.ascontiguousarray(R.scene_of(oracle, "final"))
    with vc.Renderer(desc_of(), sc) as r:
        plane = np.zeros((H, W, 4), F)
        p = plane.ctypes.data
        for fn in (lib.vcrt_draw_motion, lib.vcrt_draw_motion_device):
            assert fn(None, None, 0, None, None, None) == INIT           # no plane
            assert fn(None, sc.ctypes.data, len(sc) - 1, p, None, None) == FORMAT  # another count
            assert fn(None, sc.ctypes.data, 0, p, None, None) == FORMAT
        dev = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        d = dev.data_ptr()
        assert lib.vcrt_draw_motion_device(None, None, 0, d + 4, None, None) == INIT
        assert lib.vcrt_draw_motion_device(None, None, 0, None, d + 8, None) == INIT
        rec = torch.zeros((len(sc) * 10 + 1,), dtype=torch.float32, device="cuda")
        assert lib.vcrt_draw_motion_device(None, rec.data_ptr() + 2, len(sc), d, None,
                                           None) == INIT
        with pytest.raises(ValueError):
            r.draw_motion(prev_spheres=np.zeros((3, 9), F))
        with pytest.raises(ValueError):
            r.draw_motion(prev_camera=dict(fov=1))
        with pytest.raises(vc.VcrtError):
            r.draw_motion(prev_spheres=sc[:-1])
    assert lib.vcrt_draw_motion(None, None, 0, p, None, None) == INIT   # after vcrt_end
