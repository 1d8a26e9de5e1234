"""Adaptive sampling on the GPU (vcrt_draw_samples, vcrt_sample_counts; Renderer.draw_samples,
Renderer.sample_counts): bit parity of sums and mean with tests/adaptive_ref on scenes that take
each of the tracer's routes, pinhole and lens, one GPU and a shard's packed tiles; the relation to
the frame; accumulation; independence of the schedule and of the route; no effect on frames; the
state changes; the count rule; the forms of the call; the command-line tool."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import adaptive_ref as AR
from tests import ray_query_ref as R

pytestmark = pytest.mark.gpu
N = vc._native
F = np.float32

W, H = 44, 20  # both edges partial: 6 x 3 tiles
SENTINEL = F(-77.5)
COUNT_SENTINEL = np.uint16(999)  # outside the frame: never read


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def desc_of(radius=0.0, **kw):
    base = dict(width=W, height=H, samples_per_pixel=4, max_depth=3, device=0,
                lens_radius=radius)
    base.update(kw)
    return vc.RenderDesc(**base)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: differs at {bad[:6].tolist()} ({len(bad)} words)"


def count_planes():
    """name -> (counts [H, W] uint16, max_count): the issue's five planes."""
    rng = np.random.default_rng(20261021)
    zero = np.zeros((H, W), np.uint16)
    rand = rng.integers(0, 12, (H, W)).astype(np.uint16)   # 0 .. 11, clamped at 9
    assert int(np.minimum(rand, 9).sum()) % 64 != 0 and (rand > 9).any() and (rand == 0).any()
    one = zero.copy()
    one[11, 21] = 256
    tile = np.full((H, W), 2, np.uint16)
    tile[8:16, 16:24] = 0   # one whole tile
    tile[8:16, 24:32] = 5   # its neighbour
    return {"zero": (zero, 4), "uniform4": (np.full((H, W), 4, np.uint16), 4),
            "random": (rand, 9), "one256": (one, 256), "tile": (tile, 8)}


PLANES = count_planes()


def draw_packed(r, counts, first, max_count):
    """vcrt_draw_samples on rank-local packed planes filled with sentinels (the C ABI itself)."""
    elems, tiles = r.local_layout()
    sums = np.full((tiles, 64, 4), SENTINEL, F)
    mean = np.full((tiles, 64, 4), SENTINEL, F)
    st = N.vcrt_sample_stats()
    N.check("vcrt_draw_samples", N.lib().vcrt_draw_samples(
        first, max_count, counts.ctypes.data, 0, sums.ctypes.data, mean.ctypes.data,
        ctypes.byref(st)))
    return sums, mean, st


@pytest.mark.parametrize("first", [0, 7])
@pytest.mark.parametrize("radius", [0.0, 0.1], ids=["pinhole", "lens"])
@pytest.mark.parametrize("scene", ["final", "mixed", "three", "stress4096"])
def test_parity_with_the_reference(oracle, scene, radius, first):
    sc = R.scene_of(oracle, scene)
    desc = desc_of(radius)
    wants = {k: AR.draw_samples(oracle, sc, desc, c, first, m) for k, (c, m) in PLANES.items()}
    with vc.Renderer(desc, sc) as r:
        for name, (counts, max_count) in PLANES.items():
            want_sums, want_mean, want_st = wants[name]
            got = r.draw_samples(counts, first=first, max_count=max_count, stats=True)
            what = f"{scene} {name}"
            same(got["sums"], want_sums, what + " sums")
            same(got["mean"], want_mean, what + " mean")
            st = got["stats"]
            for k in ("samples", "pixels", "items", "segments"):
                assert st[k] == want_st[k], (what, k, st[k], want_st[k])
            assert st["kernel"] == "vcrt_trace_samples"
            if name == "zero":
                assert st["items"] == 0 and not got["sums"].any()
                continue
            assert st["kernel_ms"] > 0 and st["host_ms"] >= st["kernel_ms"]
            if radius > 0 or scene == "three":
                assert st["listed_rays"] == 0  # a lens shares no origin; four spheres: no tables
            elif scene == "final" and name != "one256":
                assert 0 < st["listed_rays"] <= st["samples"]
            if scene == "three":
                assert st["bound_tests"] == 0  # the linear scan only
    # rank 1 of 3: packed tiles, the slots outside the frame neither read nor written
    with vc.Renderer(desc_of(radius, world_size=3, rank=1), sc) as r:
        for name in ("random", "tile"):
            counts, max_count = PLANES[name]
            want_sums, want_mean, _ = wants[name]
            packed_counts = AR.packed(counts, W, H, 3, 1, COUNT_SENTINEL)
            sums, mean, st = draw_packed(r, packed_counts, first, max_count)
            same(sums, AR.packed(want_sums, W, H, 3, 1, SENTINEL), f"{scene} {name} rank 1 sums")
            same(mean, AR.packed(want_mean, W, H, 3, 1, SENTINEL), f"{scene} {name} rank 1 mean")
            mine = packed_counts != COUNT_SENTINEL
            n = np.minimum(packed_counts[mine].astype(np.int64), max_count)
            assert 0 < mine.sum() < mine.size
            assert (st.samples, st.pixels, st.items) == (
                int(n.sum()), int((n > 0).sum()), int(((n + 3) // 4).sum()))


@pytest.mark.parametrize("radius", [0.0, 0.1], ids=["pinhole", "lens"])
def test_the_frame_relation(radius):
    """Uniform 4 from index 0 is the frame of spp 4 with one quantum of 4: the sequential sum
    divided once."""
    desc = desc_of(radius, samples_per_pixel=4, accumulate_quantum=4, max_depth=8)
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        frame = r.read_framebuffer()
        got = r.draw_samples(np.full((H, W), 4, np.uint16), first=0, max_count=4)
    same(got["mean"][..., :3], frame[..., :3], "mean against the framebuffer")
    assert (got["sums"][..., 3] == 4).all() and (got["mean"][..., 3] == 1).all()
    assert len(np.unique(bits(frame[..., :3]))) > 100


def test_accumulate(oracle):
    sc = R.scene_of(oracle, "final")
    desc = desc_of()
    c1, m1 = PLANES["random"]
    c2 = np.roll(PLANES["tile"][0], 3, axis=1)
    c2[:, :5] = 0
    m2 = 8
    one = AR.draw_samples(oracle, sc, desc, c1, 0, m1)
    two = AR.draw_samples(oracle, sc, desc, c2, m1, m2, sums=one[0])
    with vc.Renderer(desc, sc) as r:
        a = r.draw_samples(c1, first=0, max_count=m1)
        same(a["sums"], one[0], "round one")
        kept = a["sums"].copy()
        b = r.draw_samples(c2, first=m1, max_count=m2, sums=a["sums"])
        assert b["sums"] is a["sums"]  # in place
        same(b["sums"], two[0], "round two sums")
        same(b["mean"], two[1], "round two mean")
        idle = c2 == 0
        assert idle.any() and np.array_equal(bits(b["sums"][idle]), bits(kept[idle]))
        assert not np.array_equal(bits(b["sums"][~idle]), bits(kept[~idle]))
        # accumulate == 0 overwrites whatever the plane held
        junk = np.full((H, W, 4), SENTINEL, F)
        c = r.draw_samples(c1, first=0, max_count=m1, sums=junk, accumulate=False)
        same(c["sums"], one[0], "overwritten")
        # pixels that never had a sample: the mean is (0, 0, 0, 1)
        never = (c1 == 0) & (c2 == 0)
        if never.any():
            assert np.array_equal(b["mean"][never], np.tile(F([0, 0, 0, 1]), (never.sum(), 1)))


@pytest.mark.parametrize("scene", ["final", "stress4096"])
def test_schedule_and_route_independence(oracle, scene, monkeypatch):
    sc = R.scene_of(oracle, scene)
    counts, max_count = PLANES["random"]

    def run(**kw):
        with vc.Renderer(desc_of(**kw), sc) as r:
            return r.draw_samples(counts, first=7, max_count=max_count, stats=True)

    base = run()
    for what, kw in (("SMEM", dict(kernel_variant=vc.KERNEL_SMEM)),
                     ("one block per CU", dict(blocks_per_cu=1)),
                     ("three blocks per CU", dict(blocks_per_cu=3))):
        got = run(**kw)
        same(got["sums"], base["sums"], f"{scene} {what}")
        same(got["mean"], base["mean"], f"{scene} {what}")
    monkeypatch.setenv("VCRT_FEATURE_LISTS", "0")
    scans = run()
    same(scans["sums"], base["sums"], f"{scene} without the lists")
    assert base["stats"]["listed_rays"] > 0 and scans["stats"]["listed_rays"] == 0
    assert scans["stats"]["segments"] == base["stats"]["segments"]


@pytest.mark.parametrize("progressive", [False, True])
def test_frames_are_left_alone(progressive):
    desc = desc_of(progressive=progressive, max_depth=8)
    counts, max_count = PLANES["random"]
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        a, sa = r.read_framebuffer(), r.stats()
        r.draw_next_frame()
        b, sb = r.read_framebuffer(), r.stats()
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        r.draw_samples(counts, first=7, max_count=max_count)
        assert np.array_equal(bits(r.read_framebuffer()), bits(a))  # the framebuffer untouched
        s = r.stats()
        assert (s["segments"], s["frames"], s["kernel"]) == (sa["segments"], 1, sa["kernel"])
        r.draw_next_frame()
        assert np.array_equal(bits(r.read_framebuffer()), bits(b))
        s = r.stats()
        assert (s["segments"], s["accumulated_spp"]) == (sb["segments"], sb["accumulated_spp"])


@pytest.mark.parametrize("radius", [0.0, 0.1], ids=["pinhole", "lens"])
def test_state_changes(oracle, radius):
    counts, max_count = PLANES["random"]
    move = dict(lookfrom=(-6.5, 3.25, 9.0), lookat=(0.5, 0.75, -1.0), vfov=33.0)
    moved = R.scene_of(oracle, "final").copy()
    moved["center"][:, 1] += F(0.125)
    moved["center"][::3, 0] -= F(0.25)
    moved["colour"][::2] = (0.25, 0.5, 0.125)
    with vc.Renderer(desc_of(radius).with_camera(**move), "final") as r:
        want_cam = r.draw_samples(counts, first=7, max_count=max_count)
    with vc.Renderer(desc_of(radius).with_camera(**move), moved) as r:
        want_both = r.draw_samples(counts, first=7, max_count=max_count)
    with vc.Renderer(desc_of(radius), "final") as r:
        before = r.draw_samples(counts, first=7, max_count=max_count)
        r.set_camera(**move)
        got = r.draw_samples(counts, first=7, max_count=max_count)
        same(got["sums"], want_cam["sums"], "after set_camera")
        r.update_spheres(moved)
        got = r.draw_samples(counts, first=7, max_count=max_count)
        same(got["sums"], want_both["sums"], "after update_spheres")
        same(got["mean"], want_both["mean"], "after update_spheres")
    assert not np.array_equal(bits(before["sums"]), bits(want_cam["sums"]))
    assert not np.array_equal(bits(want_cam["sums"]), bits(want_both["sums"]))


def test_sample_counts_on_the_gpu(oracle):
    import torch
    from tests.test_adaptive_cpu import edge_plane
    v = np.concatenate([edge_plane(0.05, 256), edge_plane(0.3, 9)])
    with vc.Renderer(desc_of(), "three") as r:
        for target, lo, hi in ((0.05, 1, 256), (0.3, 0, 9), (0.1, 0, 64)):
            want, total = vc.sample_counts_host(v, target, lo, hi, stats=True)
            got, st = r.sample_counts(v, target, lo, hi, stats=True)
            assert got.dtype == np.uint16 and np.array_equal(got, want), (target, lo, hi)
            assert st["total"] == total and st["kernel"] == "vcrt_sample_counts_pass"
            dev = r.sample_counts(torch.from_numpy(v).cuda(), target, lo, hi)
            assert dev.is_cuda and dev.dtype == torch.uint16
            assert np.array_equal(dev.cpu().numpy(), want), (target, lo, hi)


def test_variance_to_counts_to_samples(oracle):
    """One end-to-end step: a frame's moments -> variance -> sample_counts -> draw_samples."""
    sc = R.scene_of(oracle, "final")
    desc = desc_of()
    with vc.Renderer(desc, sc) as r:
        r.draw_next_frame()
        frame = r.read_framebuffer()
        mo = r.draw_motion()
        out, hist = r.reproject_moments(frame, mo["motion"], None, surface=mo["surface"])
        var = r.variance(hist)
        counts, st = r.sample_counts(var, 0.05, 0, 11, stats=True)
        got = r.draw_samples(counts, first=4, max_count=11, stats=True)
    assert np.array_equal(counts, AR.sample_counts(var, 0.05, 0, 11)[0])
    assert 0 < st["total"] == got["stats"]["samples"] and len(np.unique(counts)) > 3
    want_sums, want_mean, _ = AR.draw_samples(oracle, sc, desc, counts, 4, 11)
    same(got["sums"], want_sums, "sums")
    same(got["mean"], want_mean, "mean")


@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_the_forms_of_the_call_agree(world, rank):
    import torch
    full, max_count = PLANES["random"]
    with vc.Renderer(desc_of(world_size=world, rank=rank), "final") as r:
        elems, tiles = r.local_layout()
        counts = full if world == 1 else AR.packed(full, W, H, world, rank, np.uint16(0))
        host = r.draw_samples(counts, first=7, max_count=max_count)
        dc = torch.from_numpy(counts.astype(np.int16)).cuda()
        dev = r.draw_samples(dc, first=7, max_count=max_count, stats=True)
        for k in ("sums", "mean"):
            assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda
            same(dev[k].cpu().numpy(), host[k], k)
        # device pointers through the C ABI itself, accumulating into the tensor
        st = N.vcrt_sample_stats()
        N.check("vcrt_draw_samples_device", N.lib().vcrt_draw_samples_device(
            7 + max_count, max_count, dc.data_ptr(), 1, dev["sums"].data_ptr(), None,
            ctypes.byref(st)))
        again = r.draw_samples(counts, first=7 + max_count, max_count=max_count,
                               sums=host["sums"])
        same(dev["sums"].cpu().numpy(), again["sums"], "two rounds on the device")
        assert st.samples == dev["stats"]["samples"] > 0
        # refused before anything runs
        p, q = dev["sums"].data_ptr(), dc.data_ptr()
        lib = N.lib()
        INIT, FORMAT = N.VK_ERROR_INITIALIZATION_FAILED, N.VK_ERROR_FORMAT_NOT_SUPPORTED
        assert lib.vcrt_draw_samples_device(0, 4, q, 0, p + 4, None, None) == INIT
        assert lib.vcrt_draw_samples_device(0, 4, q + 1, 0, p, None, None) == INIT
        assert lib.vcrt_draw_samples_device(0, 4, q, 0, p, p + 8, None) == INIT
        assert lib.vcrt_draw_samples_device(0, 4, q, 0, p, p, None) == INIT
        assert lib.vcrt_draw_samples_device(0, 4, None, 0, p, None, None) == INIT
        assert lib.vcrt_draw_samples_device(0, 4, q, 0, None, None, None) == INIT
        assert lib.vcrt_draw_samples_device(0, 257, q, 0, p, None, None) == FORMAT
        assert lib.vcrt_draw_samples_device(0, 0, q, 0, p, None, None) == FORMAT
        assert lib.vcrt_draw_samples_device((1 << 19) - 3, 4, q, 0, p, None, None) == FORMAT
        v = torch.zeros(8, device="cuda")
        c = torch.zeros(8, dtype=torch.int16, device="cuda")
        pr = N.vcrt_sample_count_params(ctypes.sizeof(N.vcrt_sample_count_params), 0.1, 0, 4)
        assert lib.vcrt_sample_counts_device(v.data_ptr() + 2, 4, ctypes.byref(pr), c.data_ptr(),
                                             None) == INIT
        assert lib.vcrt_sample_counts_device(v.data_ptr(), 4, ctypes.byref(pr), c.data_ptr() + 1,
                                             None) == INIT
        for bad in (dict(counts=counts[:-1]), dict(counts=counts.astype(F)),
                    dict(counts=counts, max_count=257), dict(counts=counts, first=-1),
                    dict(counts=counts, sums=np.zeros((3, 4), F)),
                    dict(counts=counts, sums=dev["sums"]), dict(counts=counts, accumulate=True)):
            with pytest.raises(ValueError):
                r.draw_samples(**bad)


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = map(int, f.readline().split())
        assert f.readline() == b"-1.0\n"
        return np.frombuffer(f.read(), F).reshape(h, w, 3)[::-1]


def lum(c):
    y = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]).astype(F)
    return (y + F(0.0722) * c[..., 2]).astype(F)


def test_cli_runs_the_adaptive_loop(tmp_path):
    path = tmp_path / "adaptive.pfm"
    n0, target, most = 3, 0.02, 9
    cmd = [os.path.join(N.BIN_DIR, "vcrt_render"), "--width", str(W), "--height", str(H), "--spp",
           "1", "--depth", "3", "--adaptive", f"{n0},{target},{most}", "--adaptive-out", str(path)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    with vc.Renderer(desc_of(samples_per_pixel=1), "final") as r:
        uniform = np.full((H, W), n0, np.uint16)
        a = r.draw_samples(uniform, first=0, max_count=n0)
        b = r.draw_samples(uniform, first=n0, max_count=n0, sums=a["sums"])
        d = (lum(b["mean"]) - lum(a["mean"])).astype(F)
        var = ((d * d).astype(F) * F(2 * n0)).astype(F)
        counts, st = r.sample_counts(var, target, 0, most, stats=True)
        c = r.draw_samples(counts, first=2 * n0, max_count=most, sums=b["sums"])
    assert 0 < st["total"] < most * W * H and f"{st['total']} adaptive samples" in res.stdout
    same(read_pfm(str(path)), np.ascontiguousarray(c["mean"][..., :3]), "the PFM")
    # the options go together
    res = subprocess.run(cmd[:-2], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2
