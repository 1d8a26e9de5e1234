"""Feature buffers on the GPU (vcrt_draw_features, Renderer.draw_features): bit parity with
tests/features_ref on every valid pixel, on scenes that take each of the kernel's three routes,
pinhole and lens, one GPU and a shard's packed tiles; independence of the route; agreement with
the frame's own rays and with the ray queries; no effect on frames; the state changes; the forms
of the call; the command-line tool."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import features_ref as FR
from tests import ray_query_ref as R

pytestmark = pytest.mark.gpu
N = vc._native

W, H = 44, 20  # both edges partial: 6 x 3 tiles
PLANES = ("albedo", "normal_depth", "sphere")
SENTINEL = {"albedo": np.float32(-77.5), "normal_depth": np.float32(-77.5),
            "sphere": np.int32(-77)}
# (samples, first, lens radius)
CASES = [(1, 0, 0.0), (5, 7, 0.0), (16, 0, 0.0), (5, 7, 0.1), (16, 0, 0.1), (1, 7, 0.1)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def desc_of(radius=0.0, **kw):
    base = dict(width=W, height=H, samples_per_pixel=4, max_depth=3, device=0,
                lens_radius=radius)
    base.update(kw)
    return vc.RenderDesc(**base)


def same(got, want, what=""):
    for k in PLANES:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, f"{what}: {k} differs at {bad[:6].tolist()} ({len(bad)} words)"


def draw_packed(r, first, n):
    """vcrt_draw_features into sentinel-filled planes of the rank-local layout (the C ABI itself:
    the Python method hands out fresh arrays)."""
    elems, tiles = r.local_layout()
    out = {"albedo": np.full((tiles, 64, 4), SENTINEL["albedo"], np.float32),
           "normal_depth": np.full((tiles, 64, 4), SENTINEL["normal_depth"], np.float32),
           "sphere": np.full((tiles, 64), SENTINEL["sphere"], np.int32)}
    st = N.vcrt_feature_stats()
    N.check("vcrt_draw_features", N.lib().vcrt_draw_features(
        first, n, out["albedo"].ctypes.data, out["normal_depth"].ctypes.data,
        out["sphere"].ctypes.data, ctypes.byref(st)))
    return out, st


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-first{c[1]}-lens{c[2]}")
@pytest.mark.parametrize("scene", ["final", "mixed", "three", "stress4096"])
def test_parity_with_the_reference(oracle, scene, case):
    n, first, radius = case
    sc = R.scene_of(oracle, scene)
    desc = desc_of(radius)
    want = FR.frame_features(oracle, sc, desc, first, n)
    with vc.Renderer(desc, sc) as r:
        got = r.draw_features(samples=n, first=first, stats=True)
    st = got.pop("stats")
    same(got, want, f"{scene} world 1")
    assert st["rays"] == W * H * n and st["kernel"] == "vcrt_frame_features"
    assert st["group_tests"] > 0 and st["kernel_ms"] > 0 and st["host_ms"] >= st["kernel_ms"]
    if radius > 0 or scene == "three":
        assert st["listed_rays"] == 0  # a lens shares no origin; four spheres have no tables
    elif scene == "final":
        assert 0 < st["listed_rays"] <= st["rays"]
    if scene == "three":
        assert st["bound_tests"] == 0  # the linear scan only
    if scene == "stress4096" and radius == 0:  # quarters without a list take the culled scan
        assert st["listed_rays"] < st["rays"] and st["bound_tests"] > 0
    # rank 1 of 3: packed tiles, the slots outside the frame untouched
    with vc.Renderer(desc_of(radius, world_size=3, rank=1), sc) as r:
        got3, st3 = draw_packed(r, first, n)
    want3 = {k: FR.packed(want[k], W, H, 3, 1, SENTINEL[k]) for k in PLANES}
    same(got3, want3, f"{scene} rank 1 of 3")
    valid = int((want3["sphere"] != SENTINEL["sphere"]).sum())
    assert 0 < valid < want3["sphere"].size and st3.rays == valid * n


@pytest.mark.parametrize("scene", ["final", "stress4096"])
def test_route_independence(oracle, scene, monkeypatch):
    sc = R.scene_of(oracle, scene)
    with vc.Renderer(desc_of(), sc) as r:
        lists = r.draw_features(samples=5, first=7, stats=True)
    monkeypatch.setenv("VCRT_FEATURE_LISTS", "0")
    with vc.Renderer(desc_of(), sc) as r:
        scans = r.draw_features(samples=5, first=7, stats=True)
    same(scans, lists, scene)
    assert lists["stats"]["listed_rays"] > 0 and scans["stats"]["listed_rays"] == 0
    assert scans["stats"]["bound_tests"] > lists["stats"]["bound_tests"]


@pytest.mark.parametrize("radius", [0.0, 0.1])
def test_the_rays_are_the_frames(oracle, radius):
    """No host ray model: on a black Lambertian copy of the final scene a depth-1 frame is the
    direct sequential sum of 0 for a hit and the sky for a miss -- the albedo plane's rgb."""
    black = R.scene_of(oracle, "final").copy()
    black["colour"] = 0
    black["texture"][:, 0] = 1
    desc = desc_of(radius, samples_per_pixel=8, max_depth=1, accumulate_quantum=8)
    with vc.Renderer(desc, black) as r:
        r.draw_next_frame()
        frame = r.read_framebuffer()
        got = r.draw_features(samples=8)
    assert np.array_equal(bits(got["albedo"][..., :3]), bits(frame[..., :3]))
    assert got["albedo"][..., :3].any() and (got["albedo"][..., 3] > 0).any()


def test_agreement_with_the_ray_queries(oracle):
    desc = desc_of()
    y, x = np.mgrid[0:H, 0:W]
    o, d = vc.frame_rays(desc, np.stack([x.ravel(), y.ravel()], axis=1), 0, 1)
    with vc.Renderer(desc, "final") as r:
        got = r.draw_features(samples=1)
        _, hits = r.trace_rays(o[:, 0], d[:, 0], max_depth=1, hits=True)
    assert np.array_equal(got["sphere"].ravel(), hits["sphere"])
    t = np.where(hits["sphere"] >= 0, hits["t"], np.float32(0))
    want = np.concatenate([hits["normal"], t[:, None]], axis=1).astype(np.float32)
    assert np.array_equal(bits(got["normal_depth"].reshape(-1, 4)), bits(want))
    assert np.array_equal(got["albedo"][..., 3].ravel() == 1, hits["sphere"] >= 0)


@pytest.mark.parametrize("progressive", [False, True])
def test_frames_are_left_alone(progressive):
    desc = desc_of(progressive=progressive, max_depth=8)
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        a, sa = r.read_framebuffer(), r.stats()
        r.draw_next_frame()
        b, sb = r.read_framebuffer(), r.stats()
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        r.draw_features(first=7, samples=5)
        assert np.array_equal(bits(r.read_framebuffer()), bits(a))  # the framebuffer untouched
        s = r.stats()
        assert (s["segments"], s["frames"], s["kernel"]) == (sa["segments"], 1, sa["kernel"])
        r.draw_next_frame()
        assert np.array_equal(bits(r.read_framebuffer()), bits(b))
        s = r.stats()
        assert (s["segments"], s["accumulated_spp"]) == (sb["segments"], sb["accumulated_spp"])
    if progressive:
        assert not np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("radius", [0.0, 0.1])
def test_set_camera_then_features(radius):
    move = dict(lookfrom=(-6.5, 3.25, 9.0), lookat=(0.5, 0.75, -1.0), vfov=33.0)
    with vc.Renderer(desc_of(radius).with_camera(**move), "final") as r:
        want = r.draw_features(samples=5, first=7)
    with vc.Renderer(desc_of(radius), "final") as r:
        before = r.draw_features(samples=5, first=7)
        r.set_camera(**move)
        got = r.draw_features(samples=5, first=7)
    same(got, want, "after set_camera")
    assert not np.array_equal(before["sphere"], got["sphere"])


def test_update_spheres_then_features(oracle):
    moved = R.scene_of(oracle, "final").copy()
    moved["center"][:, 1] += np.float32(0.125)
    moved["center"][::3, 0] -= np.float32(0.25)
    moved["colour"][::2] = (0.25, 0.5, 0.125)
    with vc.Renderer(desc_of(), moved) as r:
        want = r.draw_features(samples=5, stats=True)
    with vc.Renderer(desc_of(), "final") as r:
        before = r.draw_features(samples=5)
        r.update_spheres(moved)
        got = r.draw_features(samples=5, stats=True)
        r.set_scene("three")
        small = r.draw_features(samples=5)
    same(got, want, "after update_spheres")
    assert got["stats"]["listed_rays"] > 0
    assert not np.array_equal(bits(before["albedo"]), bits(got["albedo"]))
    assert small["sphere"].max() <= 3  # the new scene's four spheres


@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_host_and_device_forms_agree(world, rank):
    import torch
    with vc.Renderer(desc_of(world_size=world, rank=rank), "final") as r:
        host = r.draw_features(samples=5)
        dev = r.draw_features(samples=5, device=True, stats=True)
        mine = int((vc.tile_pixel_map(W, H, world)[..., 0] == rank).sum())
        assert dev["stats"]["rays"] == 5 * mine
        for k in PLANES:
            assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda
            assert np.array_equal(bits(dev[k].cpu().numpy()), bits(host[k])), k
        # a misaligned device plane is refused before anything runs
        p = dev["albedo"].data_ptr()
        assert N.lib().vcrt_draw_features_device(0, 1, p + 4, None, None, None) == \
            N.VK_ERROR_INITIALIZATION_FAILED


def test_any_subset_of_outputs():
    with vc.Renderer(desc_of(), "final") as r:
        full = r.draw_features(samples=5)
        for on in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)):
            kw = dict(zip(("albedo", "normal", "sphere"), map(bool, on)))
            got = r.draw_features(samples=5, **kw)
            assert sorted(got) == sorted(k for k, o in zip(PLANES, on) if o)
            for k in got:
                assert np.array_equal(bits(got[k]), bits(full[k])), (on, k)
        again = r.draw_features()  # the description's spp
        assert again["albedo"].shape == (H, W, 4) and again["sphere"].shape == (H, W)


def test_cli_writes_the_guides(tmp_path):
    prefix = tmp_path / "guide"
    cmd = [os.path.join(N.BIN_DIR, "vcrt_render"), "--width", str(W), "--height", str(H), "--spp",
           "2", "--depth", "3", "--features", str(prefix), "--feature-samples", "3"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    head = f"P6\n{W} {H}\n255\n".encode()
    images = []
    for name in ("albedo", "normal"):
        data = open(f"{prefix}_{name}.ppm", "rb").read()
        assert data.startswith(head) and len(data) == len(head) + 3 * W * H, name
        images.append(np.frombuffer(data[len(head):], np.uint8))
    assert len(np.unique(images[0])) > 8 and len(np.unique(images[1])) > 8
    assert images[1][:3].tolist() == [128, 128, 128]  # the top-left pixel is sky: normal 0
