"""The denoiser on the GPU (vcrt_denoise, vcrt_denoise_device, Renderer.denoise): bit parity with
tests/denoise_ref at every shape, parameter set and guide combination, through the host and the
device form, with the LDS passes and without them; the renderer's own frame and guides, after a
camera move too; a sharded frame put through assemble_tiles; no effect on frames; the refused
calls; the statistics; the command-line tool."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import denoise_ref as D

pytestmark = pytest.mark.gpu
N = vc._native

W, H = 44, 20


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: differs at {bad[:6].tolist()} ({len(bad)} words)"


def read_pfm(path):
    """PFM (linear rgb float32, little-endian, rows bottom to top) -> float32 [H, W, 3]."""
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(b"\n", 3)
    assert parts[0] == b"PF" and float(parts[2]) < 0  # colour, little-endian
    w, h = (int(v) for v in parts[1].split())
    img = np.frombuffer(parts[3], dtype="<f4", count=w * h * 3).reshape(h, w, 3)
    return img[::-1].copy()


def host_renderer():
    """Any renderer: the calls are functions of the caller's planes and need only its device,
    stream and code object (four spheres, 16 x 16: the cheapest vcrt_begin)."""
    return vc.Renderer(vc.RenderDesc(width=16, height=16, samples_per_pixel=1, max_depth=2,
                                     device=0), "three")


def frame_desc(**kw):
    base = dict(width=W, height=H, samples_per_pixel=4, max_depth=6, device=0)
    base.update(kw)
    return vc.RenderDesc(**base)


@pytest.mark.parametrize("name", list(D.PARAM_SETS))
@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_with_the_reference(shape, name, monkeypatch):
    import torch
    w, h = shape
    params = D.PARAM_SETS[name]
    colour, albedo, nd = D.planes(w, h)
    t = [torch.from_numpy(p.copy()).cuda() for p in (colour, albedo, nd)]
    guides = dict(albedo=albedo, normal_depth=nd)
    with host_renderer() as r:
        for demodulate in (0, 1):
            want = D.reference(w, h, name, demodulate)
            for lds in ("2", "0", "1"):  # both kernels, the direct one alone, one LDS pass
                monkeypatch.setenv("VCRT_DENOISE_LDS", lds)
                got, st = r.denoise(colour, guides, stats=True, demodulate=demodulate, **params)
                same(got, want, f"{w}x{h} {name} demodulate {demodulate} host form, LDS {lds}")
                assert st["passes"] == params["levels"]
                assert st["lds_passes"] == min(int(lds), params["levels"])
                dev = r.denoise(t[0], dict(albedo=t[1], normal_depth=t[2]),
                                demodulate=demodulate, **params)
                assert isinstance(dev, torch.Tensor) and dev.is_cuda
                same(dev.cpu().numpy(), want, f"{w}x{h} {name} device form, LDS {lds}")
            monkeypatch.delenv("VCRT_DENOISE_LDS")
            same(r.denoise(colour, guides, demodulate=demodulate, **params), want, "the default")
            # each NULL-guide combination; demodulate and sigma_albedo > 0 with no albedo is no
            # error: those terms are off
            for with_albedo, with_guides in ((False, True), (True, False), (False, False)):
                g = dict(albedo=albedo if with_albedo else None,
                         normal_depth=nd if with_guides else None)
                same(r.denoise(colour, g, demodulate=demodulate, **params),
                     D.reference(w, h, name, demodulate, with_albedo, with_guides),
                     f"{w}x{h} {name} albedo {with_albedo} guides {with_guides}")
        # the inputs are left as they were
        for a, b in zip(t, (colour, albedo, nd)):
            same(a.cpu().numpy(), b, "an input plane")


def test_the_renderers_own_frame_and_guides():
    with vc.Renderer(frame_desc(), "final") as r:
        r.draw_next_frame()
        got, st = r.denoise(stats=True)
        frame, g = r.read_framebuffer(), r.draw_features(samples=4)
        want = D.denoise(frame, g["albedo"], g["normal_depth"], **D.DEFAULTS)
        same(got, want, "denoise()")
        assert not np.array_equal(bits(got[..., :3]), bits(frame[..., :3]))
        same(got[..., 3], frame[..., 3], "alpha")
        # the statistics
        assert st["kernel"] == "vcrt_denoise_pass" and st["passes"] == D.DEFAULTS["levels"]
        assert 0 <= st["lds_passes"] <= 2 and len(st["pass_ms"]) == st["passes"]
        assert st["kernel_ms"] > 0 and all(ms >= 0 for ms in st["pass_ms"])
        assert st["host_ms"] >= st["kernel_ms"]
        # the same through the device defaults: the framebuffer filtered where it lies
        dev = r.denoise(device=True, levels=3)
        same(dev.cpu().numpy(), D.denoise(frame, g["albedo"], g["normal_depth"],
                                          **dict(D.DEFAULTS, levels=3)), "denoise(device=True)")
        same(r.read_framebuffer(), frame, "the framebuffer")
        # after a camera move it sees the new frame and the new guides
        r.set_camera(lookfrom=(-6.5, 3.25, 9.0), lookat=(0.5, 0.75, -1.0), vfov=33.0)
        r.draw_next_frame()
        moved = r.denoise()
        frame2, g2 = r.read_framebuffer(), r.draw_features(samples=4)
        same(moved, D.denoise(frame2, g2["albedo"], g2["normal_depth"], **D.DEFAULTS), "moved")
        assert not np.array_equal(bits(moved), bits(got))
        assert not np.array_equal(bits(g2["albedo"]), bits(g["albedo"]))


@pytest.mark.parametrize("progressive", [False, True])
def test_frames_are_left_alone(progressive):
    desc = frame_desc(progressive=progressive)
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        a, sa = r.read_framebuffer(), r.stats()
        r.draw_next_frame()
        b, sb = r.read_framebuffer(), r.stats()
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        before = r.stats()
        r.denoise()
        r.denoise(device=True, levels=8)
        same(r.read_framebuffer(), a, "the framebuffer after a denoise")
        assert r.stats() == before  # vcrt_stats, every field
        assert (before["segments"], before["frames"], before["kernel"]) == \
            (sa["segments"], 1, sa["kernel"])
        r.draw_next_frame()
        same(r.read_framebuffer(), b, "the next frame")
        s = r.stats()
        assert (s["segments"], s["accumulated_spp"], s["frames"]) == \
            (sb["segments"], sb["accumulated_spp"], 2)
    if progressive:
        assert not np.array_equal(bits(a), bits(b))


def test_a_sharded_frame_through_assemble_tiles():
    """World 3 rendered rank by rank on one GPU: the ranks' packed frames and guide planes,
    concatenated rank-major and padded to tiles_per_rank, rebuilt by assemble_tiles and denoised,
    give the one-GPU result bit for bit."""
    import torch
    from vulkancomputeraytracing_amd import distributed as DI
    world = 3
    with vc.Renderer(frame_desc(), "final") as r:
        r.draw_next_frame()
        want = r.denoise()
    pad = DI.tiles_per_rank(W, H, world)
    names = ("frame", "albedo", "normal_depth")
    gathered = {k: torch.zeros((world, pad * 64, 4), dtype=torch.float32, device="cuda:0")
                for k in names}
    for rank in range(world):
        with vc.Renderer(frame_desc(world_size=world, rank=rank), "final") as r:
            with pytest.raises(ValueError, match="assemble_tiles"):
                r.denoise()
            r.draw_next_frame()
            g = r.draw_features(samples=4, sphere=False)
            packed = dict(frame=r.read_framebuffer(), albedo=g["albedo"],
                          normal_depth=g["normal_depth"])
            for k in names:
                flat = torch.from_numpy(packed[k].reshape(-1, 4))
                gathered[k][rank, :len(flat)] = flat.cuda()
            if rank == world - 1:
                planes = {k: torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
                          for k in names}
                torch.cuda.synchronize()
                for k in names:
                    r.assemble_tiles(gathered[k].data_ptr(), planes[k].data_ptr(), pad)
                got = r.denoise(planes["frame"], planes)
    same(got.cpu().numpy(), want, "world 3 assembled")


def test_refused_calls():
    import torch
    lib = N.lib()
    INIT, FORMAT = N.VK_ERROR_INITIALIZATION_FAILED, N.VK_ERROR_FORMAT_NOT_SUPPORTED
    a = torch.rand((8, 8, 4), device="cuda:0")
    b, c, out = a.clone(), a.clone(), torch.full_like(a, -7.0)
    with host_renderer() as r:
        for alias in (a, b, c):  # out equal to an input
            assert lib.vcrt_denoise_device(a.data_ptr(), b.data_ptr(), c.data_ptr(), 8, 8, None,
                                           alias.data_ptr(), None) == INIT
        for k in range(4):  # a misaligned plane
            p = [a.data_ptr(), b.data_ptr(), c.data_ptr(), out.data_ptr()]
            p[k] += 4
            assert lib.vcrt_denoise_device(p[0], p[1], p[2], 4, 4, None, p[3], None) == INIT
        assert lib.vcrt_denoise_device(None, b.data_ptr(), c.data_ptr(), 8, 8, None,
                                       out.data_ptr(), None) == INIT
        bad = N.vcrt_denoise_params()
        lib.vcrt_default_denoise_params(ctypes.byref(bad))
        bad.levels = 9
        assert lib.vcrt_denoise_device(a.data_ptr(), b.data_ptr(), c.data_ptr(), 8, 8,
                                       ctypes.byref(bad), out.data_ptr(), None) == FORMAT
        assert lib.vcrt_denoise_device(a.data_ptr(), b.data_ptr(), c.data_ptr(), 0, 8, None,
                                       out.data_ptr(), None) == FORMAT
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())  # nothing ran
        with pytest.raises(ValueError):
            r.denoise(a, dict(albedo=b.cpu().numpy()))
        with pytest.raises(ValueError):
            r.denoise(a, dict(albedo=b[:4]))
        with pytest.raises(vc.VcrtError):
            r.denoise(a, dict(albedo=b), sigma_depth=-1.0)
        # and a valid call after all that
        got = r.denoise(a, dict(albedo=b, normal_depth=c))
        same(got.cpu().numpy(), D.denoise(a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy(),
                                          **D.DEFAULTS), "after the refused calls")
    # after vcrt_end the GPU forms are refused again
    assert lib.vcrt_denoise_device(a.data_ptr(), b.data_ptr(), c.data_ptr(), 8, 8, None,
                                   out.data_ptr(), None) == INIT


@pytest.mark.parametrize("suffix", ["pfm", "ppm"])
def test_cli_writes_the_denoised_frame(oracle, tmp_path, suffix):
    path = tmp_path / f"clean.{suffix}"
    cmd = [os.path.join(N.BIN_DIR, "vcrt_render"), "--width", str(W), "--height", str(H), "--spp",
           "4", "--depth", "6", "--denoise", str(path), "--denoise-levels", "3"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    with vc.Renderer(frame_desc(), "final") as r:
        r.draw_next_frame()
        want = r.denoise(levels=3)
    if suffix == "pfm":
        same(read_pfm(str(path)), np.ascontiguousarray(want[..., :3]), "the PFM")
    else:
        head = f"P6\n{W} {H}\n255\n".encode()
        data = open(path, "rb").read()
        assert data.startswith(head) and len(data) == len(head) + 3 * W * H
        image = np.frombuffer(data[len(head):], np.uint8).reshape(H, W, 3)
        assert np.array_equal(image, oracle.encode_srgb8(want)[..., :3])
        assert len(np.unique(image)) > 16
