"""The denoiser's definition on the host (vcrt_denoise_host, csrc/denoise.cpp; no GPU): bit parity
with tests/denoise_ref at every shape, parameter set and guide combination; what the definition
promises of a constant image, of a depth step and of alpha; the argument errors, which read the
same without a renderer; and, on the CPU oracle's frames, that the defaults denoise."""
import ctypes
import json
import os

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import denoise_ref as D
from tests import features_ref as FR
from tests import ray_query_ref as R

N = vc._native
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: differs at {bad[:6].tolist()} ({len(bad)} words)"


@pytest.mark.parametrize("name", list(D.PARAM_SETS))
@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_reference(shape, name):
    w, h = shape
    colour, albedo, nd = D.planes(w, h)
    for demodulate in (0, 1):
        for with_albedo in (True, False):
            for with_guides in (True, False):
                want = D.reference(w, h, name, demodulate, with_albedo, with_guides)
                got = vc.denoise_host(colour, albedo if with_albedo else None,
                                      nd if with_guides else None, demodulate=demodulate,
                                      **D.PARAM_SETS[name])
                same(got, want, f"{w}x{h} {name} demodulate {demodulate} albedo {with_albedo} "
                                f"guides {with_guides}")
                assert np.isfinite(got).all()
        # a NULL plane and a zero sigma are the same "off"
        off = dict(D.PARAM_SETS[name], sigma_albedo=0, demodulate=0)
        same(vc.denoise_host(colour, None, nd, **off), vc.denoise_host(colour, albedo, nd, **off),
             "albedo off")
    if name != "none" and w * h > 6:
        blur = vc.denoise_host(colour, albedo, nd, demodulate=0,
                               **dict(D.PARAM_SETS["none"], levels=D.PARAM_SETS[name]["levels"]))
        weights_vary = not np.array_equal(bits(blur), bits(D.reference(w, h, name, 0)))
        assert weights_vary, "the edge-stopping term changed nothing: the planes test nothing"


@pytest.mark.parametrize("shape", [(44, 20), (3, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_constant_image_stays_constant(shape):
    """A weighted mean of equal values c: each w c is exact when c is a power of two (scaling
    commutes with rounding), so the sums are c wsum and the quotient is c, whatever the weights.
    For any other c every product and every one of at most 25 additions of positive terms rounds
    once, and so does the division: the relative error is below 27 x 2^-24."""
    w, h = shape
    _, albedo, nd = D.planes(w, h)
    colour = np.empty((h, w, 4), F)
    colour[...] = (0.5, 2.0, 0.125, 1.0)
    out = vc.denoise_host(colour, albedo, nd, demodulate=0, **D.PARAM_SETS["all"])
    same(out, colour, "powers of two")
    colour[...] = (0.3, 0.7, 1.9, 0.25)
    out = vc.denoise_host(colour, albedo, nd, demodulate=0, **D.PARAM_SETS["all"])
    rel = np.abs(out.astype(np.float64) - colour) / colour
    print("constant image, largest relative error", rel.max())
    assert rel.max() <= 27 * 2.0 ** -24
    same(out[..., 3], colour[..., 3], "alpha")


def test_no_leak_across_a_depth_step():
    """Sky (z = 0) beside a sphere (z = 5): rz = 5 / (5 + 2^-20), rz^2 k_depth = 100 rz^2 > 1, so
    every tap across the step has w = 0 and each half is a mean of its own colour alone."""
    w, h = 40, 12
    nd = np.zeros((h, w, 4), F)
    nd[:, 17:, :] = (0, 0, 1, 5)
    albedo = np.zeros((h, w, 4), F)
    albedo[:, :17] = (0.5, 0.7, 1.0, 0)
    albedo[:, 17:] = (0.8, 0.3, 0.2, 1)
    colour = np.zeros((h, w, 4), F)
    colour[:, :17, :3] = 1.0
    colour[:, 17:, :3] = 0.25
    colour[..., 3] = 1
    only_depth = dict(levels=5, sigma_normal=0, sigma_depth=0.1, sigma_albedo=0, sigma_colour=0)
    out = vc.denoise_host(colour, albedo, nd, demodulate=0, **only_depth)
    same(out, colour, "depth step")
    same(D.denoise(colour, albedo, nd, demodulate=0, **only_depth), colour, "the reference")
    # without the term the halves do mix
    blur = vc.denoise_host(colour, albedo, nd, demodulate=0, **dict(only_depth, sigma_depth=0))
    assert 0.25 < blur[5, 16, 0] < 1.0 and 0.25 < blur[5, 17, 0] < 1.0


def test_alpha_is_carried_through():
    colour, albedo, nd = D.planes(44, 20)
    for demodulate in (0, 1):
        out = vc.denoise_host(colour, albedo, nd, demodulate=demodulate, **D.PARAM_SETS["all"])
        same(out[..., 3], colour[..., 3], "alpha")
        assert not np.array_equal(bits(out[..., :3]), bits(colour[..., :3]))


def test_scales():
    assert vc.default_denoise_params() == pytest.approx(D.DEFAULTS)
    for s in (0.5, 0.1, 0.25, 3.0, 1e-3, 7.3):
        k = vc.denoise_scales(sigma_normal=s, sigma_depth=0, sigma_albedo=s, sigma_colour=s)
        assert bits(k).tolist() == [int(D.scale(v).view(np.uint32)) for v in (s, 0, s, s)]


def params_of(**kw):
    p = N.vcrt_denoise_params()
    N.lib().vcrt_default_denoise_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_errors_read_the_same_without_a_renderer():
    lib = N.lib()
    vc.EndRenderingOperation()  # no renderer, whatever ran before
    a = np.zeros((4, 4, 4), F)
    b, c, out = a.copy(), a.copy(), a.copy()
    FORMAT, INIT = N.VK_ERROR_FORMAT_NOT_SUPPORTED, N.VK_ERROR_INITIALIZATION_FAILED

    def calls(colour, albedo, nd, w, h, p, o):
        args = (colour, albedo, nd, w, h, None if p is None else ctypes.byref(p), o)
        return (lib.vcrt_denoise_host(*args), lib.vcrt_denoise(*args, None),
                lib.vcrt_denoise_device(*args, None))

    ptr = [x.ctypes.data for x in (a, b, c, out)]
    bad = [dict(levels=0), dict(levels=9), dict(levels=-1), dict(struct_size=4),
           dict(sigma_normal=float("nan")), dict(sigma_depth=-0.5),
           dict(sigma_albedo=float("inf")), dict(sigma_colour=float("-inf")),
           dict(sigma_normal=1e-30),                 # sigma^2 underflows: k is not finite
           dict(sigma_colour=1e-18, levels=8)]       # kl of the last pass overflows
    for kw in bad:
        assert calls(*ptr[:3], 4, 4, params_of(**kw), ptr[3]) == (FORMAT,) * 3, kw
    # the parameters come first: a bad block with NULL planes is still a format error
    assert calls(None, None, None, 4, 4, params_of(levels=0), None) == (FORMAT,) * 3
    for w, h in ((0, 4), (4, 0), (-1, 4), (65536, 1), (1, 65536), (65535, 1025)):
        assert calls(*ptr[:3], w, h, params_of(), ptr[3]) == (FORMAT,) * 3, (w, h)
    assert calls(None, ptr[1], ptr[2], 4, 4, params_of(), ptr[3]) == (INIT,) * 3
    assert calls(*ptr[:3], 4, 4, params_of(), None) == (INIT,) * 3
    for k in range(3):  # out equal to an input
        assert calls(*ptr[:3], 4, 4, params_of(), ptr[k]) == (INIT,) * 3
    # valid arguments: the host function runs (NULL params: the defaults; NULL guides and a
    # demodulate or sigma_albedo that asks for them: their terms are off, no error), the GPU
    # forms need vcrt_begin
    assert calls(*ptr[:3], 4, 4, params_of(), ptr[3]) == (N.VK_SUCCESS, INIT, INIT)
    assert calls(*ptr[:3], 4, 4, None, ptr[3]) == (N.VK_SUCCESS, INIT, INIT)
    assert calls(ptr[0], None, None, 4, 4, params_of(demodulate=1, sigma_albedo=0.5),
                 ptr[3]) == (N.VK_SUCCESS, INIT, INIT)
    # a misaligned device plane
    assert lib.vcrt_denoise_device(ptr[0] + 4, ptr[1], ptr[2], 2, 2, None, ptr[3], None) == INIT
    assert lib.vcrt_denoise_scales(ctypes.byref(params_of(levels=9)), ptr[3]) == FORMAT
    with pytest.raises(ValueError):
        vc.denoise_host(a, b[:2], c)
    with pytest.raises(ValueError):
        vc.denoise_host(a[..., :3])
    with pytest.raises(TypeError):
        vc.denoise_host(a, b, c, sigma=1)
    with pytest.raises(vc.VcrtError):
        vc.denoise_host(a, b, c, levels=0)


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    """The final scene at 64 x 36, depth 10: 4 spp, the same view at 256 spp (the C oracle) and the
    4-sample guides (features_ref)."""
    w, h, depth = 64, 36, 10
    sc = R.scene_of(oracle, "final")
    noisy, _ = oracle.render(oracle.config(w, h, 4, depth), sc)
    clean, _ = oracle.render(oracle.config(w, h, 256, depth), sc)
    g = FR.frame_features(oracle, sc, vc.RenderDesc(width=w, height=h, samples_per_pixel=4,
                                                    max_depth=depth), 0, 4)
    return noisy, clean, g


def mse(a, b):
    return float(((a[..., :3].astype(np.float64) - b[..., :3]) ** 2).mean())


def test_the_defaults_denoise(oracle_frames):
    """The condition the defaults were chosen under (profiles/denoise_defaults.json): the denoised
    4-spp frame is closer to the 256-spp frame than the 4-spp frame is."""
    noisy, clean, g = oracle_frames
    den = vc.denoise_host(noisy, g["albedo"], g["normal_depth"])
    same(den, D.denoise(noisy, g["albedo"], g["normal_depth"], **vc.default_denoise_params()),
         "the defaults on the oracle's frame")
    before, after = mse(noisy, clean), mse(den, clean)
    print(f"mse against 256 spp: noisy {before:.6g}, denoised {after:.6g}")
    assert after < before
    rec = json.load(open(os.path.join(ROOT, "profiles", "denoise_defaults.json")))
    assert rec["chosen"] == pytest.approx(vc.default_denoise_params())
