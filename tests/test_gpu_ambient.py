"""The ambient visibility buffer on the GPU (vcrt_draw_occlusion, Renderer.draw_occlusion): bit
parity with tests/ambient_ref on every valid pixel, on scenes that take each of the kernel's
routes, pinhole and lens, one GPU and a shard's packed tiles; agreement with the project's own
ray and occlusion queries and with draw_features' coverage; independence of the route and of
kernel_variant; reach at min_t; no effect on frames; the state changes; the forms of the call; the
command-line tool."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import ambient_ref as AR
from tests import ray_query_ref as R

pytestmark = pytest.mark.gpu
N = vc._native

W, H = 44, 20  # both edges partial: 6 x 3 tiles, listed, unlisted and edge tiles
SENTINEL = np.float32(-77.5)
# (n, first, m, reach, lens radius); reach None: the default, the reference's infinity 1e5
CASES = [(2, 0, 4, None, 0.0), (3, 7, 5, 2.0, 0.1), (1, 0, 1, float("inf"), 0.0)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def desc_of(radius=0.0, **kw):
    base = dict(width=W, height=H, samples_per_pixel=4, max_depth=3, device=0,
                lens_radius=radius)
    base.update(kw)
    return vc.RenderDesc(**base)


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: differs at {bad[:6].tolist()} ({len(bad)} words)"


def draw_packed(r, first, n, m, reach):
    """vcrt_draw_occlusion into a sentinel-filled plane of the rank-local layout (the C ABI
    itself: the Python method hands out a fresh array)."""
    elems, tiles = r.local_layout()
    out = np.full((tiles, 64, 4), SENTINEL, np.float32)
    st = N.vcrt_occlusion_buffer_stats()
    N.check("vcrt_draw_occlusion", N.lib().vcrt_draw_occlusion(
        first, n, m, reach, out.ctypes.data, ctypes.byref(st)))
    return out, st


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-first{c[1]}-m{c[2]}-lens{c[4]}")
@pytest.mark.parametrize("scene", ["final", "mixed", "three", "stress4096"])
def test_parity_with_the_reference(oracle, scene, case):
    n, first, m, reach, radius = case
    T = 1e5 if reach is None else reach
    sc = R.scene_of(oracle, scene)
    desc = desc_of(radius)
    want = AR.frame_occlusion(oracle, sc, desc, first, n, m, T)
    with vc.Renderer(desc, sc) as r:
        got, st = r.draw_occlusion(samples=n, first=first, rays=m, reach=reach, stats=True)
    print(scene, case, {k: st[k] for k in ("hit_rays", "secondary_rays", "occluded")},
          {k: want[k] for k in ("hit_rays", "secondary_rays", "occluded")})
    same(got, want["visibility"], f"{scene} world 1")
    assert st["rays"] == W * H * n and st["kernel"] == "vcrt_frame_occlusion"
    assert st["hit_rays"] == want["hit_rays"]
    assert st["secondary_rays"] == want["secondary_rays"]
    assert st["occluded"] == want["occluded"]
    assert st["group_tests"] > 0 and st["kernel_ms"] > 0 and st["host_ms"] >= st["kernel_ms"]
    if radius > 0 or scene == "three":
        assert st["listed_rays"] == 0  # a lens shares no origin; four spheres have no tables
    elif scene == "final":
        assert 0 < st["listed_rays"] <= st["rays"]
    if scene == "three":
        assert st["bound_tests"] == 0  # the linear scans only
    else:
        assert st["bound_tests"] > 0   # the secondary rays take the culled scan
    # rank 1 of 3: packed tiles, the slots outside the frame untouched
    with vc.Renderer(desc_of(radius, world_size=3, rank=1), sc) as r:
        got3, st3 = draw_packed(r, first, n, m, T)
    want3 = AR.packed(want["visibility"], W, H, 3, 1, SENTINEL)
    same(got3, want3, f"{scene} rank 1 of 3")
    valid = int((want3[..., 0] != SENTINEL).sum())
    assert 0 < valid < want3[..., 0].size and st3.rays == valid * n
    mine = vc.tile_pixel_map(W, H, 3)[..., 0] == 1
    C = want["C"][mine].sum()
    assert st3.hit_rays == C and st3.secondary_rays == C * m
    assert st3.occluded == want["blocked"][mine].sum()


@pytest.mark.parametrize("radius", [0.0, 0.1])
def test_agreement_with_the_queries(radius):
    """The same buffer the long way round: the frame's rays through trace_rays, the secondary
    rays built here in fp32 and put through occluded -- the project's own kernels, no reference."""
    n, first, m, reach = 3, 7, 5, 2.0
    desc = desc_of(radius)
    y, x = np.mgrid[0:H, 0:W]
    o, d = vc.frame_rays(desc, np.stack([x.ravel(), y.ravel()], axis=1), first, n)
    O, D = o.reshape(-1, 3), d.reshape(-1, 3)
    u = vc.ambient_dirs(first * m, n * m).reshape(n, m, 3)
    F = np.float32
    with vc.Renderer(desc, "final") as r:
        got = r.draw_occlusion(samples=n, first=first, rays=m, reach=reach)
        feat = r.draw_features(samples=n, first=first, normal=False, sphere=False)
        _, hits = r.trace_rays(O, D, max_depth=1, hits=True)
        hit = hits["sphere"] >= 0
        nrm, t = hits["normal"], hits["t"]
        P = (O + (t[:, None] * D).astype(F)).astype(F)
        dn = ((D[:, 0] * nrm[:, 0] + D[:, 1] * nrm[:, 1]).astype(F) + D[:, 2] * nrm[:, 2])
        Nn = np.where((dn > 0)[:, None], -nrm, nrm).astype(F)
        d2 = (Nn[:, None, :] + u[np.arange(len(O)) % n]).astype(F)
        occ = r.occluded(np.repeat(P[hit], m, axis=0), d2[hit].reshape(-1, 3), tmax=reach)
    blocked = np.zeros(len(O), np.int64)
    blocked[hit] = occ.reshape(-1, m).sum(axis=1)
    blocked = blocked.reshape(H * W, n).sum(axis=1)
    C = hit.reshape(H * W, n).sum(axis=1)
    want_v = ((n * m - blocked).astype(F) / F(n * m)).astype(F)
    assert 0 < blocked.sum() < hit.sum() * m
    assert np.array_equal(bits(got[..., 0].ravel()), bits(want_v))
    assert np.array_equal(bits(got[..., 3].ravel()), bits((C.astype(F) / F(n)).astype(F)))
    assert np.array_equal(bits(got[..., 3]), bits(feat["albedo"][..., 3]))


@pytest.mark.parametrize("scene", ["final", "stress4096"])
def test_route_independence(oracle, scene, monkeypatch):
    sc = R.scene_of(oracle, scene)
    with vc.Renderer(desc_of(), sc) as r:
        lists, st = r.draw_occlusion(samples=3, first=7, rays=5, reach=2.0, stats=True)
    for variant in (vc.KERNEL_SMEM, vc.KERNEL_CULL_FLAT):
        with vc.Renderer(desc_of(kernel_variant=variant), sc) as r:
            same(r.draw_occlusion(samples=3, first=7, rays=5, reach=2.0), lists,
                 f"{scene} variant {variant}")
    monkeypatch.setenv("VCRT_FEATURE_LISTS", "0")
    with vc.Renderer(desc_of(), sc) as r:
        scans, st0 = r.draw_occlusion(samples=3, first=7, rays=5, reach=2.0, stats=True)
    same(scans, lists, scene)
    assert st["listed_rays"] > 0 and st0["listed_rays"] == 0
    assert st0["bound_tests"] > st["bound_tests"]
    assert (st0["hit_rays"], st0["occluded"]) == (st["hit_rays"], st["occluded"])


@pytest.mark.parametrize("reach", [0.001, 0.0, -1.0, float("-inf")])
def test_reach_at_min_t_leaves_everything_open(reach):
    with vc.Renderer(desc_of(), "final") as r:
        got, st = r.draw_occlusion(samples=2, rays=4, reach=reach, stats=True)
        cover = r.draw_features(samples=2, normal=False, sphere=False)["albedo"][..., 3]
    assert np.all(got[..., :3] == 1) and st["occluded"] == 0
    assert st["hit_rays"] > 0 and st["secondary_rays"] == 4 * st["hit_rays"]
    assert np.array_equal(bits(got[..., 3]), bits(cover))


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
        r.draw_occlusion(first=7, samples=3, rays=5)
        assert np.array_equal(bits(r.read_framebuffer()), bits(a))  # the framebuffer untouched
        s = r.stats()
        assert (s["segments"], s["frames"], s["kernel"]) == (sa["segments"], 1, sa["kernel"])
        r.draw_next_frame()
        assert np.array_equal(bits(r.read_framebuffer()), bits(b))
        s = r.stats()
        assert (s["segments"], s["accumulated_spp"]) == (sb["segments"], sb["accumulated_spp"])
    if progressive:
        assert not np.array_equal(bits(a), bits(b))


def test_state_changes(oracle):
    move = dict(lookfrom=(-6.5, 3.25, 9.0), lookat=(0.5, 0.75, -1.0), vfov=33.0)
    moved = R.scene_of(oracle, "final").copy()
    moved["center"][:, 1] += np.float32(0.125)
    moved["center"][::3, 0] -= np.float32(0.25)
    kw = dict(samples=3, first=7, rays=5, reach=2.0)
    with vc.Renderer(desc_of().with_camera(**move), "final") as r:
        want_camera = r.draw_occlusion(**kw)
    with vc.Renderer(desc_of().with_camera(**move), moved) as r:
        want_both = r.draw_occlusion(**kw)
    with vc.Renderer(desc_of(), "final") as r:
        before = r.draw_occlusion(**kw)
        r.set_camera(**move)
        after_camera = r.draw_occlusion(**kw)
        r.update_spheres(moved)
        after_both = r.draw_occlusion(**kw)
    same(after_camera, want_camera, "after set_camera")
    same(after_both, want_both, "after update_spheres")
    assert not np.array_equal(bits(before), bits(after_camera))
    assert not np.array_equal(bits(after_camera), bits(after_both))


@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_host_and_device_forms_agree(world, rank):
    import torch
    with vc.Renderer(desc_of(world_size=world, rank=rank), "final") as r:
        host = r.draw_occlusion(samples=3, rays=5)
        dev, st = r.draw_occlusion(samples=3, rays=5, device=True, stats=True)
        mine = int((vc.tile_pixel_map(W, H, world)[..., 0] == rank).sum())
        assert st["rays"] == 3 * mine
        assert isinstance(dev, torch.Tensor) and dev.is_cuda
        assert np.array_equal(bits(dev.cpu().numpy()), bits(host))
        assert 0 < st["occluded"] < st["secondary_rays"]
        # a misaligned device plane is refused before anything runs
        assert N.lib().vcrt_draw_occlusion_device(0, 1, 1, 1e5, dev.data_ptr() + 4, None) == \
            N.VK_ERROR_INITIALIZATION_FAILED


def test_cli_writes_the_buffer(oracle, tmp_path):
    prefix = tmp_path / "guide"
    cmd = [os.path.join(N.BIN_DIR, "vcrt_render"), "--width", str(W), "--height", str(H), "--spp",
           "2", "--depth", "3", "--ao", str(prefix), "--ao-rays", "5", "--feature-samples", "3"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    head = f"P6\n{W} {H}\n255\n".encode()
    data = open(f"{prefix}_ao.ppm", "rb").read()
    assert data.startswith(head) and len(data) == len(head) + 3 * W * H
    image = np.frombuffer(data[len(head):], np.uint8).reshape(H, W, 3)
    with vc.Renderer(desc_of(samples_per_pixel=2), "final") as r:
        plane = r.draw_occlusion(samples=3, rays=5)
    assert np.array_equal(image, oracle.encode_srgb8(plane)[..., :3])
    assert len(np.unique(image)) > 4
