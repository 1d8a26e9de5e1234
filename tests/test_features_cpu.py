"""Feature buffers without a GPU (vcrt_draw_features, vcrt_frame_rays): the host-only ray
definition against tests/lens_ref bit for bit, the argument errors of the C ABI and the Python
layer, the stats struct's layout, and tests/features_ref checked on hand-made cases."""
import ctypes

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import features_ref as FR
from tests import lens_ref as L
from tests.oracle_py import SPHERE_DTYPE

N = vc._native
W, H = 44, 20
OTHER_CAMERA = dict(lookfrom=(-6.5, 3.25, 9.0), lookat=(0.5, 0.75, -1.0), vup=(0.1, 1.0, 0.05),
                    vfov=33.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def all_pixels():
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x.ravel(), y.ravel()], axis=1)


@pytest.mark.parametrize("camera", [{}, OTHER_CAMERA], ids=["reference", "other"])
@pytest.mark.parametrize("radius", [0.0, 0.1])
@pytest.mark.parametrize("first", [0, 7])
def test_frame_rays_equal_the_lens_reference(oracle, camera, radius, first):
    n = 5
    desc = vc.RenderDesc(width=W, height=H, samples_per_pixel=3, lens_radius=radius, **camera)
    want_o, want_d = L.frame_rays(oracle, desc, first, n)      # [n, 3], [H, W, n, 3]
    got_o, got_d = vc.frame_rays(desc, all_pixels(), first, n)  # [H * W, n, 3]
    assert got_o.shape == got_d.shape == (H * W, n, 3)
    assert np.array_equal(bits(got_d), bits(want_d.reshape(H * W, n, 3)))
    assert np.array_equal(bits(got_o), bits(np.broadcast_to(want_o, (H * W, n, 3))))
    if radius == 0:  # the pinhole: every ray starts at the camera centre
        assert np.all(got_o == got_o[0, 0])
    else:
        assert len(np.unique(got_o[0], axis=0)) == n
    # a subset in another order gives the same rays
    sel = np.array([[W - 1, H - 1], [0, 0], [17, 3]])
    sub_o, sub_d = vc.frame_rays(desc, sel, first, n)
    assert np.array_equal(bits(sub_d), bits(want_d[sel[:, 1], sel[:, 0]]))


def test_frame_rays_errors():
    lib = N.lib()
    d = vc.RenderDesc(width=W, height=H).to_c()
    xy = np.array([[0, 0]], np.int32)
    o = np.zeros((1, 1, 3), np.float32)

    def call(desc, pxy, npix, first, n):
        return lib.vcrt_frame_rays(ctypes.byref(desc) if desc is not None else None, pxy, npix,
                                   first, n, o.ctypes.data, o.ctypes.data)
    assert call(d, xy.ctypes.data, 1, 0, 1) == 1
    assert call(d, xy.ctypes.data, 0, 0, 1) == 0
    assert call(None, xy.ctypes.data, 1, 0, 1) == N.VK_ERROR_INITIALIZATION_FAILED
    assert call(d, None, 1, 0, 1) == N.VK_ERROR_INITIALIZATION_FAILED
    assert call(d, xy.ctypes.data, -1, 0, 1) == N.VK_ERROR_INITIALIZATION_FAILED
    assert call(d, xy.ctypes.data, 1, 0, 0) == -11            # FORMAT_NOT_SUPPORTED
    assert call(d, xy.ctypes.data, 1, (1 << 19) - 1, 2) == -11
    assert call(d, xy.ctypes.data, 1, (1 << 19) - 1, 1) == 1
    assert call(d, xy.ctypes.data, 1, 0xFFFFFFFF, 2) == -11    # no 32-bit wrap
    outside = np.array([[W, 0]], np.int32)
    assert call(d, outside.ctypes.data, 1, 0, 1) == N.VK_ERROR_INITIALIZATION_FAILED
    bad = vc.RenderDesc(width=0, height=H).to_c()
    assert call(bad, xy.ctypes.data, 1, 0, 1) == N.VK_ERROR_INITIALIZATION_FAILED


@pytest.mark.parametrize("entry", ["vcrt_draw_features", "vcrt_draw_features_device"])
def test_draw_features_errors_without_a_renderer(entry):
    """Nothing here touches the GPU: no renderer has begun."""
    lib = N.lib()
    lib.vcrt_end()
    f = getattr(lib, entry)
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    st = N.vcrt_feature_stats()
    assert f(0, 4, p, p, p, ctypes.byref(st)) == N.VK_ERROR_INITIALIZATION_FAILED  # before begin
    assert f(0, 4, None, None, None, None) == N.VK_ERROR_INITIALIZATION_FAILED
    assert f(0, 0, p, None, None, None) == -11
    assert f(1 << 19, 1, p, None, None, None) == -11
    assert f((1 << 19) - 4, 5, None, None, p, None) == -11
    assert f(0xFFFFFFFF, 2, None, p, None, None) == -11
    assert f((1 << 19) - 4, 4, p, None, None, None) == N.VK_ERROR_INITIALIZATION_FAILED
    assert not buf.any()


def test_python_argument_errors():
    desc = vc.RenderDesc(width=W, height=H)
    for first, n in ((0, 0), (-1, 1), (1 << 19, 1), (0, (1 << 19) + 1), ("x", 1)):
        with pytest.raises(ValueError):
            vc.frame_rays(desc, [[0, 0]], first, n)
    for xy in ([0, 0], [[0, 0, 0]], [[W, 0]], [[0, H]], [[-1, 0]], "pixels"):
        with pytest.raises(ValueError):
            vc.frame_rays(desc, xy, 0, 1)
    # draw_features validates before it asks for the library's state
    r = object.__new__(vc.Renderer)
    r.desc = desc
    for kw in (dict(samples=0), dict(first=-1), dict(samples=1 << 19, first=1),
               dict(albedo=False, normal=False, sphere=False)):
        with pytest.raises(ValueError):
            r.draw_features(**kw)
    with pytest.raises(vc.VcrtError):  # valid arguments reach the (closed) renderer
        r.draw_features(samples=2)


def test_feature_stats_layout():
    """include/vcrt.h: four u64, two doubles, char[48]."""
    S = N.vcrt_feature_stats
    assert ctypes.sizeof(S) == 4 * 8 + 2 * 8 + 48
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [
        ("rays", 0), ("listed_rays", 8), ("group_tests", 16), ("bound_tests", 24),
        ("kernel_ms", 32), ("host_ms", 40), ("kernel", 48)]
    import os
    import re
    header = open(os.path.join(os.path.dirname(N.HERE), "include", "vcrt.h")).read()
    body = re.search(r"typedef struct vcrt_feature_stats \{(.*?)\} vcrt_feature_stats;", header,
                     re.S).group(1)
    names = re.findall(r"^\s*(?:uint64_t|double|char)\s+(\w+)", body, re.M)
    assert names == [f for f, _ in S._fields_]


def _scene(rows):
    arr = np.zeros(len(rows), dtype=SPHERE_DTYPE)
    for i, (c, r, col, tex) in enumerate(rows):
        arr[i]["center"], arr[i]["radius"], arr[i]["colour"], arr[i]["texture"] = c, r, col, tex
    return arr


def test_reference_rows_on_hand_made_cases(oracle):
    unit = _scene([((0, 0, 0), 1.0, (0.25, 0.5, 0.75), (1, 0.5, 0)),
                   ((5, 0, 0), 1.0, (0.1, 0.2, 0.3), (3, 1.5, 0))])
    O = np.array([[0, 0, 3], [5, 0, 3], [0, 9, 3]], np.float32)
    D = np.array([[0, 0, -1], [0, 0, -2], [0, 1, -1]], np.float32)
    a, nrm, z, c, sphere = FR.sample_rows(oracle, unit, O, D)
    assert sphere.tolist() == [0, 1, -1] and c.tolist() == [1, 1, 0]
    # straight at a unit sphere from z = 3: t = 2, the normal (0, 0, 1)
    assert z[0] == 2 and nrm[0].tolist() == [0, 0, 1] and a[0].tolist() == [0.25, 0.5, 0.75]
    # t is in units of dir; glass reads 1, whatever its colour
    assert z[1] == 1 and nrm[1].tolist() == [0, 0, 1] and a[1].tolist() == [1, 1, 1]
    # the sky: ray_color at depth 1 of a miss, no normal, no depth
    sky, segs = oracle.ray_color(unit, O[2], D[2], 1)
    assert segs == 1 and np.array_equal(bits(a[2]), bits(sky))
    assert z[2] == 0 and not nrm[2].any()


def test_reference_pixel_whose_samples_all_miss(oracle):
    far = _scene([((0, -500, 0), 1.0, (0.5, 0.5, 0.5), (1, 1.0, 0))])
    desc = vc.RenderDesc(width=W, height=H, samples_per_pixel=1)
    ref = FR.frame_features(oracle, far, desc, 0, 1)
    assert np.all(ref["sphere"] == -1) and not ref["normal_depth"].any()
    assert not ref["albedo"][..., 3].any()
    o, d = L.frame_rays(oracle, desc, 0, 1)
    sky, _ = oracle.ray_color(far, o[0], d[3, 5, 0], 1)
    assert np.array_equal(bits(ref["albedo"][3, 5, :3]), bits(sky))
    # three samples: the sequential fp32 mean of the three skies
    ref3 = FR.frame_features(oracle, far, desc, 7, 3)
    o, d = L.frame_rays(oracle, desc, 7, 3)
    acc = np.zeros(3, np.float32)
    for k in range(3):
        acc = (acc + oracle.ray_color(far, o[k], d[19, 43, k], 1)[0]).astype(np.float32)
    assert np.array_equal(bits(ref3["albedo"][19, 43, :3]), bits(acc / np.float32(3)))


def test_reference_packing():
    plane = np.arange(H * W, dtype=np.int32).reshape(H, W)
    total = 0
    for rank in range(3):
        p = FR.packed(plane, W, H, 3, rank, -7)
        assert p.shape == (len(vc.tiles_for_rank(W, H, 3, rank)), 64)
        total += int((p != -7).sum())
    assert total == H * W
    p1 = FR.packed(plane, W, H, 3, 1, -7)
    t = vc.tiles_for_rank(W, H, 3, 1)[0]
    tx, ty = t % 6, t // 6
    assert p1[0, 8 * 2 + 3] == plane[8 * ty + 2, 8 * tx + 3]
