"""Temporal accumulation on the GPU (vcrt_reproject, vcrt_reproject_device, Renderer.reproject):
bit parity with tests/reproject_ref on the CPU tests' generated planes through the host and the
device form; a draw / motion / reproject sequence across an orbit against the reference chain; a
sharded frame put through assemble_tiles; the static case; the command-line tool; the refused
calls."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import motion_ref as M
from tests import ray_query_ref as R
from tests import reproject_ref as P

pytestmark = pytest.mark.gpu
N = vc._native
F = np.float32

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
    base = dict(width=W, height=H, samples_per_pixel=4, max_depth=3, device=0)
    base.update(kw)
    return vc.RenderDesc(**base)


def orbit(desc, degrees):
    """desc's camera turned about the y axis through lookat, as vcrt_render --orbit turns it."""
    th = math.radians(degrees)
    dx, dz = desc.lookfrom[0] - desc.lookat[0], desc.lookfrom[2] - desc.lookat[2]
    return desc.with_camera(lookfrom=(
        float(F(desc.lookat[0] + dx * math.cos(th) + dz * math.sin(th))), desc.lookfrom[1],
        float(F(desc.lookat[2] - dx * math.sin(th) + dz * math.cos(th)))))


@pytest.mark.parametrize("name", list(P.PARAM_SETS))
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_with_the_reference(shape, name):
    import torch
    w, h = shape
    params = P.PARAM_SETS[name]
    colour, motion, hcol, hsurf, hlen = pl = P.planes(w, h)
    want, want_len, took = P.reference(w, h, name)
    hist = dict(colour=hcol, surface=hsurf, length=hlen)
    t = [torch.from_numpy(p.copy()).cuda() for p in pl]
    with host_renderer() as r:
        got, h2, st = r.reproject(colour, motion, hist, surface=hsurf, stats=True, **params)
        same(got, want, f"{w}x{h} {name} host form")
        same(h2["length"], want_len, f"{w}x{h} {name} host form, length")
        assert h2["colour"] is got and h2["surface"] is hsurf
        assert st["accepted_pixels"] == int(took.sum()) and st["kernel"] == "vcrt_reproject_pass"
        assert st["kernel_ms"] > 0 and st["host_ms"] >= st["kernel_ms"]
        dev, hd = r.reproject(t[0], t[1], dict(colour=t[2], surface=t[3], length=t[4]), **params)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and hd["length"].is_cuda
        same(dev.cpu().numpy(), want, f"{w}x{h} {name} device form")
        same(hd["length"].cpu().numpy(), want_len, f"{w}x{h} {name} device form, length")
        # the inputs are left as they were
        for a, b in zip(t, pl):
            same(a.cpu().numpy(), b, "an input plane")


def reference_chain(oracle, scene, descs, params):
    """The sequence on the host: the oracle's frames, the restated maps, the restated blend.
    A list of (out, length, accepted, motion, surface) per frame."""
    sc = R.scene_of(oracle, scene)
    steps = []
    for i, d in enumerate(descs):
        frame, _ = oracle.render(oracle.config(d.width, d.height, d.samples_per_pixel,
                                               d.max_depth, d.lookfrom, d.lookat, d.vup, d.vfov),
                                 sc)
        m = M.frame_motion(oracle, sc, d, descs[i - 1] if i else None)
        if i == 0:
            out, length = frame.copy(), np.ones((d.height, d.width), F)
            took = np.zeros((d.height, d.width), bool)
        else:
            out, length, took = P.reproject(frame, m["motion"], steps[-1][0], steps[-1][4],
                                            steps[-1][1], **params)
        steps.append((out, length, took, m["motion"], m["surface"]))
    return steps


def test_a_sequence_across_an_orbit(oracle):
    """draw -> motion -> reproject over three views 3 degrees apart, on the GPU through the host
    and the device forms, against the reference chain."""
    import torch
    descs = [orbit(frame_desc(), 3.0 * k) for k in range(3)]
    # a depth tolerance of 0.02: there the float32 reference accepts 86.7 % of the pixels after
    # one step and 29 % of them on all four taps, so both branches of every test are at work
    # (at the default 0.1 only the silhouettes reject: 98 % accept)
    params = dict(alpha=0.2, max_history=32.0, depth_tolerance=0.02)
    steps = reference_chain(oracle, "three", descs, params)
    # the history branch must be at work in the reference itself, both ways
    for out, length, took, motion, _ in steps[1:]:
        share = took.mean()
        print(f"accepted {share:.3f}")
        assert share >= 0.5 and 1 - share >= 0.05
    assert (steps[2][1] == 3).any()  # a pixel with three frames behind it
    with vc.Renderer(descs[0], "three") as r:
        hist, hist_dev = None, None
        for k, d in enumerate(descs):
            if k:
                r.set_camera(lookfrom=d.lookfrom)
            r.draw_next_frame()
            frame = r.read_framebuffer()
            mo = r.draw_motion(prev_camera=descs[k - 1] if k else None)
            same(mo["motion"], steps[k][3], f"frame {k} motion")
            out, hist, st = r.reproject(frame, mo["motion"], hist, surface=mo["surface"],
                                        stats=True, **params)
            same(out, steps[k][0], f"frame {k}")
            same(hist["length"], steps[k][1], f"frame {k} length")
            assert st["accepted_pixels"] == int(steps[k][2].sum())
            # the same on the device: no host round trip
            md = r.draw_motion(prev_camera=descs[k - 1] if k else None, device=True)
            fb = torch.from_numpy(frame).cuda()
            out_dev, hist_dev = r.reproject(fb, md["motion"], hist_dev, surface=md["surface"],
                                            **params)
            same(out_dev.cpu().numpy(), steps[k][0], f"frame {k} device form")


def test_a_sharded_frame_through_assemble_tiles(oracle):
    """World 3 rendered rank by rank on one GPU: the ranks' packed frames and motion planes,
    concatenated rank-major and padded to tiles_per_rank, rebuilt by assemble_tiles, give the
    one-GPU planes and the one-GPU result bit for bit."""
    import torch
    from vulkancomputeraytracing_amd import distributed as DI
    world = 3
    prev = orbit(frame_desc(), 3.0)
    with vc.Renderer(frame_desc(), "final") as r:
        r.draw_next_frame()
        frame = r.read_framebuffer()
        one = r.draw_motion(prev_camera=prev)
    hcol, hsurf, hlen = P.planes(W, H)[2], one["surface"], np.full((H, W), 3, F)
    want, want_len, took = P.reproject(frame, one["motion"], hcol, hsurf, hlen, **P.DEFAULTS)
    assert 0.3 < took.mean() < 1
    pad = DI.tiles_per_rank(W, H, world)
    names = ("frame", "motion", "surface")
    gathered = {k: torch.zeros((world, pad * 64, 4), dtype=torch.float32, device="cuda:0")
                for k in names}
    for rank in range(world):
        with vc.Renderer(frame_desc(world_size=world, rank=rank), "final") as r:
            r.draw_next_frame()
            mo = r.draw_motion(prev_camera=prev)
            packed = dict(frame=r.read_framebuffer(), motion=mo["motion"], surface=mo["surface"])
            for k in names:
                flat = torch.from_numpy(packed[k].reshape(-1, 4))
                gathered[k][rank, :len(flat)] = flat.cuda()
            if rank == world - 1:
                planes = {k: torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
                          for k in names}
                torch.cuda.synchronize()
                for k in names:
                    r.assemble_tiles(gathered[k].data_ptr(), planes[k].data_ptr(), pad)
                hist = dict(colour=torch.from_numpy(hcol.copy()).cuda(), surface=planes["surface"],
                            length=torch.from_numpy(hlen).cuda())
                got, h2 = r.reproject(planes["frame"], planes["motion"], hist, **P.DEFAULTS)
    same(planes["motion"].cpu().numpy(), one["motion"], "world 3 assembled motion")
    same(planes["surface"].cpu().numpy(), one["surface"], "world 3 assembled surface")
    same(got.cpu().numpy(), want, "world 3 assembled")
    same(h2["length"].cpu().numpy(), want_len, "world 3 assembled, length")


def test_a_static_view_is_the_running_average():
    """Five progressive frames' worth of new samples under identity motion: every pixel takes one
    tap of weight 1, so the k-th output is hcol + (c - hcol) / k computed in that order."""
    desc = frame_desc()
    with vc.Renderer(desc, "final") as r:
        mo = r.draw_motion(stats=True)
        assert mo["stats"]["identity"] == W * H
        hist, mean = None, None
        for k in range(1, 6):
            r.draw_next_frame()
            c = r.read_framebuffer()
            # (a static renderer redraws the same samples; scale them so the frames differ)
            c = (c * F(1 + 0.125 * k)).astype(F)
            out, hist = r.reproject(c, mo["motion"], hist, surface=mo["surface"],
                                    alpha=2.0 ** -20, max_history=64, depth_tolerance=0.1)
            if mean is None:
                mean = c.copy()
            else:
                a = F(1) / F(k)
                mean[..., :3] = mean[..., :3] + (a * (c[..., :3] - mean[..., :3]).astype(F)
                                                 ).astype(F)
                mean[..., 3] = c[..., 3]
            same(out, mean, f"frame {k}")
            assert (hist["length"] == k).all()


def test_cli_writes_the_accumulated_frame(tmp_path):
    path = tmp_path / "out.pfm"
    clean = tmp_path / "clean.pfm"
    cmd = [os.path.join(N.BIN_DIR, "vcrt_render"), "--width", str(W), "--height", str(H), "--spp",
           "4", "--depth", "3", "--scene", "three", "--orbit", "3", "--frames", "3", "--temporal",
           str(path), "--denoise", str(clean), "--denoise-levels", "3"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    descs = [orbit(frame_desc(), 3.0 * k) for k in range(3)]
    with vc.Renderer(descs[0], "three") as r:
        hist = None
        for k, d in enumerate(descs):
            if k:
                r.set_camera(lookfrom=d.lookfrom)
            r.draw_next_frame()
            mo = r.draw_motion(prev_camera=descs[k - 1] if k else None)
            out, hist = r.reproject(r.read_framebuffer(), mo["motion"], hist,
                                    surface=mo["surface"])
        last = r.read_framebuffer()
        # --denoise composes: the accumulated frame, filtered under the last view's guides
        want_clean = r.denoise(out, r.draw_features(samples=4, sphere=False), levels=3)
    same(read_pfm(str(path)), np.ascontiguousarray(out[..., :3]), "the PFM")
    assert not np.array_equal(bits(out[..., :3]), bits(last[..., :3]))
    same(read_pfm(str(clean)), np.ascontiguousarray(want_clean[..., :3]), "the denoised PFM")


def test_refused_calls():
    import torch
    lib = N.lib()
    INIT, FORMAT = N.VK_ERROR_INITIALIZATION_FAILED, N.VK_ERROR_FORMAT_NOT_SUPPORTED
    planes = [torch.rand((8, 8, 4), device="cuda:0") for _ in range(4)]
    planes.append(torch.ones((8, 8), device="cuda:0"))
    out, length = torch.full((8, 8, 4), -7.0, device="cuda:0"), torch.full((8, 8), -7.0,
                                                                          device="cuda:0")
    ptr = [p.data_ptr() for p in planes]
    o, ol = out.data_ptr(), length.data_ptr()
    with host_renderer() as r:
        for k in range(5):
            assert lib.vcrt_reproject_device(*ptr, 8, 8, None, ptr[k], ol, None) == INIT
            assert lib.vcrt_reproject_device(*ptr, 8, 8, None, o, ptr[k], None) == INIT
            q = list(ptr)
            q[k] = None
            assert lib.vcrt_reproject_device(*q, 8, 8, None, o, ol, None) == INIT
            q = list(ptr)
            q[k] += 4 if k < 4 else 2  # a misaligned plane
            assert lib.vcrt_reproject_device(*q, 4, 4, None, o, ol, None) == INIT
        assert lib.vcrt_reproject_device(*ptr, 4, 4, None, o + 8, ol, None) == INIT
        assert lib.vcrt_reproject_device(*ptr, 4, 4, None, o, ol + 1, None) == INIT
        bad = N.vcrt_reproject_params()
        lib.vcrt_default_reproject_params(ctypes.byref(bad))
        bad.alpha = 0.0
        assert lib.vcrt_reproject_device(*ptr, 8, 8, ctypes.byref(bad), o, ol, None) == FORMAT
        assert lib.vcrt_reproject_device(*ptr, 0, 8, None, o, ol, None) == FORMAT
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((length == -7.0).all())  # nothing ran
        hist = dict(colour=planes[2], surface=planes[3], length=planes[4])
        with pytest.raises(ValueError):
            r.reproject(planes[0], planes[1].cpu().numpy(), hist)
        with pytest.raises(ValueError):
            r.reproject(planes[0], planes[1][:4], hist)
        with pytest.raises(ValueError):
            r.reproject(planes[0], planes[1], dict(colour=planes[2]))
        with pytest.raises(vc.VcrtError):
            r.reproject(planes[0], planes[1], hist, max_history=0)
        # and a valid call after all that
        got, h2 = r.reproject(planes[0], planes[1], hist)
        want, want_len, _ = P.reproject(*(p.cpu().numpy() for p in planes), **P.DEFAULTS)
        same(got.cpu().numpy(), want, "after the refused calls")
        same(h2["length"].cpu().numpy(), want_len, "after the refused calls, length")
    # after vcrt_end the GPU forms are refused again
    assert lib.vcrt_reproject_device(*ptr, 8, 8, None, o, ol, None) == INIT
