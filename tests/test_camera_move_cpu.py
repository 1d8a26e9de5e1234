"""The moving camera without a GPU: the C ABI's new symbols and their bindings, the calls'
answers before vcrt_begin, Renderer.set_camera's merge of partial arguments, and the command
line's --orbit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc

N = vc._native

NEW_SYMBOLS = ("vcrt_set_camera", "vcrt_get_camera_stats", "vcrt_camera_lists_read")


def test_symbols_and_bindings_exist():
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in N.SIGNATURES, name
    for name in ("set_camera", "camera_lists", "camera_stats"):
        assert callable(getattr(vc.Renderer, name)), name
    # the struct as include/vcrt.h lays it out: 2 doubles, 2 int32, 3 uint64
    assert ctypes.sizeof(N.vcrt_camera_stats) == 48
    assert [f for f, _ in N.vcrt_camera_stats._fields_] == [
        "host_ms", "lists_ms", "on_device", "reserved", "quarters", "group_ids", "pair_records"]
    text = open(os.path.join(os.path.dirname(N.HERE), "include", "Renderer.hpp")).read()
    assert "VkResult SetRenderCamera(IN const vcrt_camera* camera);" in text


def test_calls_before_begin():
    lib = N.lib()
    lib.vcrt_end()
    cam = vc.RenderDesc().to_c().camera
    assert lib.vcrt_set_camera(ctypes.byref(cam)) == N.VK_ERROR_INITIALIZATION_FAILED
    assert lib.vcrt_set_camera(None) == N.VK_ERROR_INITIALIZATION_FAILED
    st = N.vcrt_camera_stats()
    assert lib.vcrt_get_camera_stats(ctypes.byref(st)) == N.VK_ERROR_INITIALIZATION_FAILED
    nids, npairs = ctypes.c_int32(7), ctypes.c_int32(7)
    assert lib.vcrt_camera_lists_read(None, None, 0, None, 0, None, 0, ctypes.byref(nids),
                                      ctypes.byref(npairs)) == N.VK_ERROR_INITIALIZATION_FAILED
    assert lib.vcrt_camera_lists_read(None, None, 0, None, 0, None, 0, None,
                                      None) == N.VK_ERROR_INITIALIZATION_FAILED


def test_with_camera_merges_partial_arguments():
    d = vc.RenderDesc(width=44, height=20, vfov=25.0)
    e = d.with_camera(lookfrom=(1, 2, 3))
    assert e.lookfrom == (1.0, 2.0, 3.0) and e.lookat == d.lookat and e.vup == d.vup
    assert e.vfov == 25.0 and (e.width, e.height) == (44, 20)
    assert d.lookfrom == (13.0, 2.0, 3.0)  # a copy: the original is untouched
    f = e.with_camera(lookat=np.array([0, 0.5, 0]), vfov=30)
    assert f.lookfrom == (1.0, 2.0, 3.0) and f.lookat == (0.0, 0.5, 0.0) and f.vfov == 30.0
    assert d.with_camera() == d
    with pytest.raises(ValueError):
        d.with_camera(vup=(0, 1))


class _FakeLib:
    """Stands in for libvcrt in Renderer.set_camera: records the camera it is handed."""

    def __init__(self, code):
        self.code, self.seen = code, []

    def vcrt_set_camera(self, ref):
        c = ref._obj
        self.seen.append((tuple(c.lookfrom), tuple(c.lookat), tuple(c.vup), c.vfov))
        return self.code


def _unopened_renderer(desc, lib):
    r = vc.Renderer.__new__(vc.Renderer)   # no vcrt_begin: nothing here touches a GPU
    r.desc, r._c_desc = desc, desc.to_c()
    r._L = lambda: lib
    return r


def test_renderer_set_camera_merges_into_desc():
    lib = _FakeLib(N.VK_SUCCESS)
    r = _unopened_renderer(vc.RenderDesc(width=44, height=20), lib)
    r.set_camera(lookfrom=(2, 0.3, 1.5), vfov=60)
    assert r.desc.lookfrom == (2.0, 0.3, 1.5) and r.desc.vfov == 60.0
    assert r.desc.lookat == (0.0, 0.0, 0.0) and r.desc.vup == (0.0, 1.0, 0.0)
    f32 = lambda v: tuple(float(np.float32(x)) for x in v)
    assert lib.seen[-1] == (f32((2, 0.3, 1.5)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0)
    r.set_camera(lookat=(-6, 0.2, -2))
    assert r.desc.lookfrom == (2.0, 0.3, 1.5) and r.desc.lookat == (-6.0, 0.2, -2.0)
    assert lib.seen[-1][0] == f32((2, 0.3, 1.5)) and lib.seen[-1][1] == f32((-6, 0.2, -2))
    assert tuple(r._c_desc.camera.lookat) == f32((-6, 0.2, -2))


def test_renderer_set_camera_keeps_desc_on_error():
    lib = _FakeLib(N.VK_ERROR_INITIALIZATION_FAILED)
    d = vc.RenderDesc(width=44, height=20)
    r = _unopened_renderer(d, lib)
    with pytest.raises(vc.VcrtError):
        r.set_camera(lookfrom=(1, 1, 1))
    assert r.desc == d


def test_closed_renderer_rejects_camera_calls():
    r = vc.Renderer.__new__(vc.Renderer)
    r.desc, r._open = vc.RenderDesc(), False
    for call in (lambda: r.set_camera(vfov=30), r.camera_stats, r.camera_lists):
        with pytest.raises(vc.VcrtError) as e:
            call()
        assert e.value.code == N.VK_ERROR_INITIALIZATION_FAILED


def test_cli_help_lists_orbit():
    res = subprocess.run([os.path.join(N.BIN_DIR, "vcrt_render"), "--help"],
                         capture_output=True, text=True, timeout=60)
    assert "--orbit DEG" in res.stdout + res.stderr
