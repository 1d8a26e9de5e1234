"""The ambient visibility buffer without a GPU (vcrt_draw_occlusion, vcrt_ambient_dirs): the
symbols and bindings, the host-only direction table against tests/ambient_ref bit for bit, the
argument errors of the C ABI and the Python layer (all before vcrt_begin), the stats struct's
layout, and the conditions on tests/ambient_ref that keep the GPU parity test from passing
vacuously."""
import ctypes
import os
import re

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import ambient_ref as AR
from tests import ray_query_ref as R

N = vc._native
W, H = 44, 20
FORMAT = -11  # VK_ERROR_FORMAT_NOT_SUPPORTED
# (n, first, m, reach, lens radius): the GPU parity test's cases (reach None: the default, 1e5)
CASES = [(2, 0, 4, None, 0.0), (3, 7, 5, 2.0, 0.1), (1, 0, 1, float("inf"), 0.0)]
SCENES = ("final", "mixed", "three", "stress4096")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_symbols_and_bindings():
    lib = N.lib()
    for name in ("vcrt_draw_occlusion", "vcrt_draw_occlusion_device", "vcrt_ambient_dirs"):
        assert name in N.SIGNATURES and getattr(lib, name) is not None
    assert callable(vc.Renderer.draw_occlusion) and callable(vc.ambient_dirs)
    header = open(os.path.join(os.path.dirname(N.HERE), "include", "Renderer.hpp")).read()
    assert "DrawOcclusion(" in header


def test_stats_layout():
    """include/vcrt.h: seven u64, two doubles, char[48]."""
    S = N.vcrt_occlusion_buffer_stats
    names = ["rays", "hit_rays", "secondary_rays", "occluded", "listed_rays", "group_tests",
             "bound_tests", "kernel_ms", "host_ms", "kernel"]
    assert ctypes.sizeof(S) == 7 * 8 + 2 * 8 + 48
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == \
        [(f, 8 * i) for i, f in enumerate(names)]
    header = open(os.path.join(os.path.dirname(N.HERE), "include", "vcrt.h")).read()
    body = re.search(r"typedef struct vcrt_occlusion_buffer_stats \{(.*?)\} "
                     r"vcrt_occlusion_buffer_stats;", header, re.S).group(1)
    assert re.findall(r"^\s*(?:uint64_t|double|char)\s+(\w+)", body, re.M) == names


@pytest.mark.parametrize("first,count", [(0, 4096), ((1 << 22) - 64, 64), ((1 << 19) * 7, 33)])
def test_ambient_dirs_equal_the_reference(oracle, first, count):
    got = vc.ambient_dirs(first, count)
    want = AR.ambient_dirs(oracle, first, count)
    assert got.shape == want.shape == (count, 3) and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))
    len2 = (got.astype(np.float64) ** 2).sum(axis=1)
    assert np.abs(len2 - 1).max() <= 1e-6
    # a table, not a constant (rand repeats a value now and then: not every row is distinct)
    assert len(np.unique(got, axis=0)) > count // 2
    # a subrange gives the same rows
    assert np.array_equal(bits(vc.ambient_dirs(first + 5, 7)), bits(want[5:12]))


def test_ambient_dirs_errors():
    lib = N.lib()
    out = np.zeros((4, 3), np.float32)
    p = out.ctypes.data
    assert lib.vcrt_ambient_dirs(0, 4, p) == 4
    assert lib.vcrt_ambient_dirs(0, 0, None) == 0
    assert lib.vcrt_ambient_dirs((1 << 22) - 4, 4, p) == 4
    assert lib.vcrt_ambient_dirs((1 << 22) - 3, 4, p) == FORMAT
    assert lib.vcrt_ambient_dirs(0xFFFFFFFF, 2, p) == FORMAT      # no 32-bit wrap
    assert lib.vcrt_ambient_dirs(0, 4, None) == N.VK_ERROR_INITIALIZATION_FAILED
    for first, count in ((-1, 1), (0, -1), ((1 << 22), 1), ("x", 1)):
        with pytest.raises(ValueError):
            vc.ambient_dirs(first, count)


@pytest.mark.parametrize("entry", ["vcrt_draw_occlusion", "vcrt_draw_occlusion_device"])
def test_errors_without_a_renderer(entry):
    """Nothing here touches the GPU: no renderer has begun."""
    lib = N.lib()
    lib.vcrt_end()
    f = getattr(lib, entry)
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    st = N.vcrt_occlusion_buffer_stats()
    init = N.VK_ERROR_INITIALIZATION_FAILED
    assert f(0, 4, 8, 1e5, p, ctypes.byref(st)) == init          # before begin
    assert f(0, 4, 8, 1e5, None, None) == init                   # no plane
    assert f(0, 4, 8, float("nan"), p, None) == init             # reach NaN
    assert f(0, 4, 8, float("inf"), p, None) == init             # (+inf is taken: before begin)
    # the ranges, whatever else is wrong
    assert f(0, 0, 8, 1e5, p, None) == FORMAT                    # n >= 1
    assert f(0, 4, 0, 1e5, p, None) == FORMAT                    # m >= 1
    assert f(0, 1, 257, 1e5, p, None) == FORMAT                  # m <= 256
    assert f(0, 1, 256, 1e5, p, None) == init
    assert f(0, 17, 256, 1e5, p, None) == FORMAT                 # n m <= 4096
    assert f(0, 16, 256, 1e5, p, None) == init
    assert f(0, 4097, 1, 1e5, p, None) == FORMAT
    assert f((1 << 19) - 4, 5, 1, 1e5, p, None) == FORMAT        # first + n <= 2^19
    assert f((1 << 19) - 4, 4, 1, 1e5, p, None) == init
    assert f(0xFFFFFFFF, 2, 1, 1e5, p, None) == FORMAT           # no 32-bit wrap
    assert f((1 << 19) - 4, 4, 9, 1e5, p, None) == FORMAT        # (first + n) m <= 2^22
    assert f((1 << 19) - 4, 4, 8, 1e5, p, None) == init
    assert f(0, 0, 8, float("nan"), None, None) == FORMAT        # the ranges come first
    assert not buf.any()


def test_python_argument_errors():
    r = object.__new__(vc.Renderer)
    r.desc = vc.RenderDesc(width=W, height=H)
    for kw in (dict(samples=0), dict(first=-1), dict(samples=1 << 19, first=1), dict(rays=0),
               dict(rays=257), dict(rays="many"), dict(samples=513, rays=8),
               dict(samples=4, first=(1 << 19) - 4, rays=9), dict(reach=float("nan")),
               dict(reach="far")):
        with pytest.raises(ValueError):
            r.draw_occlusion(**kw)
    with pytest.raises(vc.VcrtError):  # valid arguments reach the (closed) renderer
        r.draw_occlusion(samples=2, reach=float("inf"))


@pytest.mark.parametrize("scene", SCENES)
def test_the_reference_is_not_vacuous(oracle, scene):
    """The first two parity cases on every scene: hit samples (1364 .. 2185 of 1760 .. 2640
    rays), occluded and open secondary rays (483 .. 3868 of 5456 .. 10925), at least 125 partly
    open pixels, and no d' at the culled scans' guard: the smallest |d'|^2 is 5.6e-5 (stress4096,
    the second case), 58 times the guard's 2^-20, so every wave takes the scan its scene has."""
    sc = R.scene_of(oracle, scene)
    for n, first, m, reach, radius in CASES[:2]:
        desc = vc.RenderDesc(width=W, height=H, samples_per_pixel=4, max_depth=3,
                             lens_radius=radius)
        ref = AR.frame_occlusion(oracle, sc, desc, first, n, m, 1e5 if reach is None else reach)
        rays = W * H * n
        assert 0.5 * rays < ref["hit_rays"] < rays, (scene, ref["hit_rays"])
        assert ref["secondary_rays"] == ref["hit_rays"] * m
        assert 400 < ref["occluded"] < 0.5 * ref["secondary_rays"], (scene, ref["occluded"])
        assert ref["min_d2"] >= 2.0 ** -15, (scene, ref["min_d2"])
        v = ref["visibility"]
        assert np.array_equal(bits(v[..., 0]), bits(v[..., 1]))
        assert np.array_equal(bits(v[..., 0]), bits(v[..., 2]))
        assert v[..., :3].min() >= 0 and v.max() <= 1
        assert int(((v[..., 0] > 0) & (v[..., 0] < 1)).sum()) >= 125, scene
        # a pixel whose samples all missed is fully open with no coverage
        sky = ref["C"] == 0
        assert np.all(v[sky] == (1, 1, 1, 0))


def test_reference_on_a_hand_made_case(oracle):
    """A unit sphere and the camera inside a big shell: every sample hits, and every secondary
    ray ends on the shell (from the shell itself the chord along normal + unit vector has t =
    the radius, whatever the vector), so nothing is open; with reach = min_t everything is."""
    from tests.oracle_py import SPHERE_DTYPE
    sc = np.zeros(2, dtype=SPHERE_DTYPE)
    sc[0]["center"], sc[0]["radius"] = (0, 0, 0), 1.0
    sc[1]["center"], sc[1]["radius"] = (0, 0, 0), 50.0          # the camera sits inside the lid
    for s in sc:
        s["colour"], s["texture"] = (0.5, 0.5, 0.5), (1, 1.0, 0)
    desc = vc.RenderDesc(width=W, height=H, samples_per_pixel=1)
    shut = AR.frame_occlusion(oracle, sc, desc, 0, 2, 4, 1e5)
    assert shut["hit_rays"] == W * H * 2 and shut["occluded"] == shut["secondary_rays"]
    assert not shut["visibility"][..., :3].any() and np.all(shut["visibility"][..., 3] == 1)
    near = AR.frame_occlusion(oracle, sc, desc, 0, 2, 4, 0.001)
    assert near["occluded"] == 0 and np.all(near["visibility"] == 1)
