"""Variance-guided denoising's definitions on the host (vcrt_reproject_moments_host,
vcrt_variance_host, vcrt_denoise_variance_host, csrc/variance.cpp; no GPU): bit parity with
tests/variance_ref at every shape and parameter set; the moments call's out and out_length are
vcrt_reproject_host's words; what the definitions promise of a repeated frame and of a huge
variance; and the argument errors, which read the same without a renderer."""
import ctypes
import json
import os

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import denoise_ref as D
from tests import reproject_ref as P
from tests import variance_ref as V

N = vc._native
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: differs at {bad[:6].tolist()} ({len(bad)} words)"


def moments_host(p, name, with_albedo=True):
    return vc.reproject_moments_host(p["colour"], p["motion"], p["hcol"], p["hsurf"], p["hlen"],
                                     p["hmom"], albedo=p["albedo"] if with_albedo else None,
                                     **V.MOMENTS_SETS[name])


def test_the_planes_hold_what_they_should():
    """The generated planes of the largest shapes exercise every branch of the definitions."""
    for w, h in ((44, 20), (100, 37)):
        p = V.planes(w, h)
        assert (p["albedo"][..., :3] < V.EPS).any() and (p["albedo"][..., :3] == V.EPS).any()
        assert (p["surface"][..., 0] == 1).any() and (p["surface"][..., 0] > 1).any()  # sky, spheres
        n = p["moments"][..., 3]
        assert (n < 4).any() and (n == 4).any() and (n > 4).any()
        var = p["var"]
        assert (var == 0).any() and ((var > 0) & (var < 1e-10)).any() and (var > 1e5).any()
        assert (var < 0).any()
        _, _, mom, took = V.moments_reference(w, h, "long-history")
        assert 0.3 < took.mean() < 0.95
        assert (mom[..., 2] > 0).any() and (mom[..., 2] == 0).any()
        _, spatial = V.variance_reference(w, h, "svgf")
        assert 0.2 < spatial.mean() < 0.8
        # the spatial estimate: neighbours on the pixel's surface and off it
        key = p["surface"][..., 0]
        assert (key[:, 1:] != key[:, :-1]).any() and (key[:, 1:] == key[:, :-1]).any()
        assert (key[1:] != key[:-1]).any() and (key[1:] == key[:-1]).any()


@pytest.mark.parametrize("name", list(V.MOMENTS_SETS))
@pytest.mark.parametrize("shape", V.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_host_equals_the_reference(shape, name):
    w, h = shape
    p = V.planes(w, h)
    for with_albedo in (True, False):
        want, want_len, want_mom, _ = V.moments_reference(w, h, name, with_albedo)
        out, length, mom = moments_host(p, name, with_albedo)
        same(out, want, f"{w}x{h} {name}")
        same(length, want_len, f"{w}x{h} {name} length")
        same(mom, want_mom, f"{w}x{h} {name} moments albedo={with_albedo}")
        assert np.isfinite(mom).all() and (mom[..., 2] >= 0).all()
        same(mom[..., 3], length, "moments.w is the length")


@pytest.mark.parametrize("name", list(V.MOMENTS_SETS))
@pytest.mark.parametrize("shape", V.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_out_is_reprojects(shape, name):
    """out and out_length are vcrt_reproject_host's words for the same planes and parameters."""
    w, h = shape
    p = V.planes(w, h)
    out, length, _ = moments_host(p, name)
    want, want_len = vc.reproject_host(*P.planes(w, h), **P.PARAM_SETS[name])
    same(out, want, f"{w}x{h} {name}")
    same(length, want_len, f"{w}x{h} {name} length")


def test_without_albedo_the_moments_are_the_colours_luminance():
    w, h = 44, 20
    p = V.planes(w, h)
    zeros = np.zeros((h, w, 4), F)
    # no history: every pixel M1 = Y, M2 = Y * Y
    _, length, mom = vc.reproject_moments_host(p["colour"], p["motion"], zeros, zeros,
                                               np.zeros((h, w), F), zeros)
    y = V.lum(p["colour"])
    assert (length == 1).all()
    same(mom[..., 0], y, "M1")
    same(mom[..., 1], y * y, "M2")
    same(mom[..., 3], length, "N")
    # with an albedo it is the demodulated colour's
    _, _, mom = vc.reproject_moments_host(p["colour"], p["motion"], zeros, zeros,
                                          np.zeros((h, w), F), zeros, albedo=p["albedo"])
    same(mom[..., 0], V.lum(p["colour"][..., :3] / np.fmax(p["albedo"][..., :3], V.EPS)), "M1")


@pytest.mark.parametrize("name", list(V.VARIANCE_SETS))
@pytest.mark.parametrize("shape", V.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_variance_host_equals_the_reference(shape, name):
    w, h = shape
    p = V.planes(w, h)
    want, spatial = V.variance_reference(w, h, name)
    got = vc.variance_host(p["moments"], p["surface"], **V.VARIANCE_SETS[name])
    same(got, want, f"{w}x{h} {name}")
    assert np.isfinite(got).all() and (got >= 0).all()
    if name == "all-temporal":
        assert not spatial.any()
    if name == "all-spatial":
        assert spatial.all()


@pytest.mark.parametrize("name", list(V.DENOISE_SETS))
@pytest.mark.parametrize("shape", V.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_variance_host_equals_the_reference(shape, name):
    w, h = shape
    p = V.planes(w, h)
    for demodulate in (1, 0):
        want, want_var = V.denoise_reference(w, h, name, demodulate)
        out, out_var = vc.denoise_variance_host(p["colour"], p["var"], p["albedo"], p["nd"],
                                                demodulate=demodulate, **V.DENOISE_SETS[name])
        same(out, want, f"{w}x{h} {name} demodulate={demodulate}")
        same(out_var, want_var, f"{w}x{h} {name} variance")
        assert np.isfinite(out).all() and np.isfinite(out_var).all() and (out_var >= 0).all()
        same(out[..., 3], p["colour"][..., 3], "alpha")


@pytest.mark.parametrize("albedo,guides", [(False, False), (True, False), (False, True)])
def test_denoise_variance_host_without_a_guide_plane(albedo, guides):
    w, h = 44, 20
    p = V.planes(w, h)
    want, want_var = V.denoise_reference(w, h, "all", 1, albedo, guides)
    out, out_var = vc.denoise_variance_host(p["colour"], p["var"],
                                            p["albedo"] if albedo else None,
                                            p["nd"] if guides else None, **V.DENOISE_SETS["all"])
    same(out, want)
    same(out_var, want_var)


def identity_motion(w, h, key=2.0, z=3.0):
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w, 4), F)
    m[..., 0], m[..., 1], m[..., 2], m[..., 3] = x, y, z, key
    return m


def test_a_repeated_frame_has_variance_zero_and_is_left_alone():
    """A frame repeated under identity motion: one tap of weight 1, h1 = Y and h2 = Y2 exactly,
    so M1 = Y + am * 0 = Y, M2 = Y2 = fl(M1 * M1) and the variance is exactly 0 from the second
    call on. The denoiser then has g = 0 and kv = 1 / 2^-20 = 2^20: a tap whose luminance differs
    by 2^-10 or more has w = 0. Over a grey frame of multiples of 1/8 (luminance steps of ~1/8, and
    every product with a binomial weight exact) with no guide planes each pixel is averaged with
    equal neighbours only: out = frame to the bit, out_variance = 0."""
    w, h = 44, 20
    rng = np.random.default_rng(11)
    c = np.zeros((h, w, 4), F)
    c[..., :3] = (rng.integers(2, 17, (h, w)) / 8.0).astype(F)[..., None]
    c[..., 3] = rng.random((h, w)).astype(F)
    m = identity_motion(w, h)
    surf = np.zeros((h, w, 4), F)
    surf[..., 0], surf[..., 1] = 2.0, 3.0
    zeros = np.zeros((h, w, 4), F)
    out, length, mom = vc.reproject_moments_host(c, m, zeros, surf, np.zeros((h, w), F), zeros)
    for k in range(2, 5):
        out, length, mom = vc.reproject_moments_host(c, m, out, surf, length, mom, alpha=0.2,
                                                     alpha_moments=0.3, max_history=3.0)
        same(out, c, f"call {k}")
        assert (length == min(k, 3)).all()
        assert (mom[..., 2] == 0).all()
        var = vc.variance_host(mom, surf, min_history=2.0, alpha=0.2)
        assert (bits(var) == 0).all(), f"call {k}: the variance is +0"
    den, den_var = vc.denoise_variance_host(c, var, levels=5, sigma_colour=4.0)
    same(den, c, "the denoised repeated frame")
    assert (den_var == 0).all()


@pytest.mark.parametrize("demodulate", [1, 0])
def test_a_huge_variance_switches_the_colour_term_off(demodulate):
    """variance = 1e30 everywhere: g ~ 1e30 (and no smaller than 1e30 / 25^5 at the last pass),
    kv <= 1e-21, so tl = dy^2 kv < 2^-25 for any luminance the planes hold: X + tl = X where
    X > 0 (or e = 1 - tl = 1 where X = 0) -- the weights, and so the rgb, are those of
    vcrt_denoise_host with sigma_colour = 0."""
    w, h = 44, 20
    colour, albedo, nd = D.planes(w, h)
    pr = dict(V.DENOISE_SETS["all"], demodulate=demodulate)
    out, out_var = vc.denoise_variance_host(colour, np.full((h, w), 1e30, F), albedo, nd, **pr)
    want = vc.denoise_host(colour, albedo, nd, **dict(pr, sigma_colour=0.0))
    same(out[..., :3], want[..., :3])
    same(out[..., 3], colour[..., 3])
    assert (out_var > 1e22).all() and (out_var <= 1e30).all()


def test_defaults():
    assert set(vc.default_reproject_moments_params()) == {"alpha", "max_history",
                                                          "depth_tolerance", "alpha_moments"}
    assert set(vc.default_variance_params()) == {"min_history", "alpha"}
    dv, dd = vc.default_denoise_variance_params(), vc.default_denoise_params()
    assert {k: v for k, v in dv.items() if k != "sigma_colour"} == \
           {k: v for k, v in dd.items() if k != "sigma_colour"}
    # the variance pass is told the alpha the moments pass runs with
    assert vc.default_variance_params()["alpha"] == vc.default_reproject_moments_params()["alpha"]
    # the grid search's choice (tools/variance_defaults.py), scored beside today's chain
    rec = json.load(open(os.path.join(ROOT, "profiles", "variance_defaults.json")))
    chosen = rec["chosen"]
    assert vc.default_reproject_moments_params()["alpha"] == pytest.approx(chosen["alpha"])
    assert vc.default_reproject_moments_params()["alpha_moments"] == \
        pytest.approx(chosen["alpha_moments"])
    assert vc.default_variance_params() == pytest.approx(
        dict(min_history=chosen["min_history"], alpha=chosen["alpha"]))
    assert dv["sigma_colour"] == pytest.approx(chosen["sigma_colour"])
    assert rec["mse_chosen"] == min(p["mse"] for p in rec["points"])
    assert rec["new_chain_scores_lower"] == (rec["mse_chosen"] < rec["today"]["mse"])
    assert rec["today"]["reproject"] == pytest.approx(vc.default_reproject_params())
    assert rec["today"]["denoise"] == pytest.approx(vc.default_denoise_params())
    # the existing defaults are untouched
    assert vc.default_reproject_params() == pytest.approx(P.DEFAULTS)
    assert dd == pytest.approx(D.DEFAULTS)


def moments_params(**kw):
    p = N.vcrt_reproject_moments_params()
    N.lib().vcrt_default_reproject_moments_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def variance_params(**kw):
    p = N.vcrt_variance_params()
    N.lib().vcrt_default_variance_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def denoise_params(**kw):
    p = N.vcrt_denoise_params()
    N.lib().vcrt_default_denoise_variance_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


FORMAT, INIT, OK = (N.VK_ERROR_FORMAT_NOT_SUPPORTED, N.VK_ERROR_INITIALIZATION_FAILED,
                    N.VK_SUCCESS)
NAN = float("nan")


def ref(p):
    return None if p is None else ctypes.byref(p)


def test_moments_errors_read_the_same_without_a_renderer():
    lib = N.lib()
    vc.EndRenderingOperation()  # no renderer, whatever ran before
    pl = [np.zeros((4, 4, 4), F) for _ in range(4)] + [np.zeros((4, 4), F)] + \
         [np.zeros((4, 4, 4), F) for _ in range(2)]
    outs = [np.full((4, 4, 4), -1, F), np.full((4, 4), -1, F), np.full((4, 4, 4), -1, F)]
    ptr = [x.ctypes.data for x in pl]
    o = [x.ctypes.data for x in outs]

    def calls(planes, w, h, p, o3):
        args = (*planes, w, h, ref(p), *o3)
        return (lib.vcrt_reproject_moments_host(*args), lib.vcrt_reproject_moments(*args, None),
                lib.vcrt_reproject_moments_device(*args, None))

    bad = [dict(struct_size=16), dict(alpha=0.0), dict(alpha=NAN), dict(max_history=0.5),
           dict(max_history=65536.0), dict(depth_tolerance=-1e-3), dict(alpha_moments=0.0),
           dict(alpha_moments=-0.5), dict(alpha_moments=1.5), dict(alpha_moments=NAN)]
    for kw in bad:
        assert calls(ptr, 4, 4, moments_params(**kw), o) == (FORMAT,) * 3, kw
    assert calls([None] * 7, 4, 4, moments_params(alpha_moments=0.0), [None] * 3) == (FORMAT,) * 3
    for w, h in ((0, 4), (4, 0), (65536, 1), (65535, 1025)):
        assert calls(ptr, w, h, moments_params(), o) == (FORMAT,) * 3, (w, h)
    for k in range(7):
        if k != 5:  # a NULL input; the albedo may be NULL
            assert calls(ptr[:k] + [None] + ptr[k + 1:], 4, 4, None, o) == (INIT,) * 3, k
        for j in range(3):  # an output equal to an input
            assert calls(ptr, 4, 4, None, o[:j] + [ptr[k]] + o[j + 1:]) == (INIT,) * 3, (k, j)
    for j in range(3):  # a NULL output; two outputs equal
        assert calls(ptr, 4, 4, None, o[:j] + [None] + o[j + 1:]) == (INIT,) * 3
    assert calls(ptr, 4, 4, None, [o[0], o[1], o[0]]) == (INIT,) * 3
    assert calls(ptr, 4, 4, None, [o[0], o[0], o[2]]) == (INIT,) * 3
    assert all((x == -1).all() for x in outs), "a refused call wrote to an output plane"
    assert calls(ptr, 4, 4, None, o) == (OK, INIT, INIT)
    assert calls(ptr[:5] + [None] + ptr[6:], 4, 4, moments_params(), o) == (OK, INIT, INIT)
    # a misaligned device plane
    for k in (0, 5, 6):
        shifted = ptr[:k] + [ptr[k] + 4] + ptr[k + 1:]
        assert lib.vcrt_reproject_moments_device(*shifted, 2, 2, None, *o, None) == INIT
    assert lib.vcrt_reproject_moments_device(*ptr, 2, 2, None, o[0], o[1], o[2] + 8, None) == INIT
    assert lib.vcrt_reproject_moments_device(*ptr, 2, 2, None, o[0], o[1] + 2, o[2], None) == INIT
    a = pl[0]
    with pytest.raises(ValueError):
        vc.reproject_moments_host(a, a[:2], a, a, pl[4], a)
    with pytest.raises(ValueError):
        vc.reproject_moments_host(a, a, a, a, a, a)  # the length plane has no channels
    with pytest.raises(ValueError):
        vc.reproject_moments_host(a, a, a, a, pl[4], None)
    with pytest.raises(TypeError):
        vc.reproject_moments_host(a, a, a, a, pl[4], a, sigma=1)
    with pytest.raises(vc.VcrtError):
        vc.reproject_moments_host(a, a, a, a, pl[4], a, alpha_moments=0)


def test_variance_errors_read_the_same_without_a_renderer():
    lib = N.lib()
    vc.EndRenderingOperation()
    mom, surf = np.zeros((4, 4, 4), F), np.zeros((4, 4, 4), F)
    out = np.full((4, 4), -1, F)
    m, s, o = mom.ctypes.data, surf.ctypes.data, out.ctypes.data

    def calls(m, s, w, h, p, o):
        args = (m, s, w, h, ref(p), o)
        return (lib.vcrt_variance_host(*args), lib.vcrt_variance(*args, None),
                lib.vcrt_variance_device(*args, None))

    bad = [dict(struct_size=8), dict(min_history=0.5), dict(min_history=65536.0),
           dict(min_history=NAN), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=NAN)]
    for kw in bad:
        assert calls(m, s, 4, 4, variance_params(**kw), o) == (FORMAT,) * 3, kw
    assert calls(None, None, 4, 4, variance_params(alpha=0.0), None) == (FORMAT,) * 3
    for w, h in ((0, 4), (4, 0), (65536, 1), (65535, 1025)):
        assert calls(m, s, w, h, None, o) == (FORMAT,) * 3
    for args in ((None, s, o), (m, None, o), (m, s, None), (m, s, m), (m, s, s)):
        assert calls(args[0], args[1], 4, 4, None, args[2]) == (INIT,) * 3, args
    assert (out == -1).all()
    assert calls(m, s, 4, 4, None, o) == (OK, INIT, INIT)
    assert calls(m, s, 4, 4, variance_params(min_history=1.0, alpha=1.0), o) == (OK, INIT, INIT)
    assert lib.vcrt_variance_device(m + 4, s, 2, 2, None, o, None) == INIT
    assert lib.vcrt_variance_device(m, s + 8, 2, 2, None, o, None) == INIT
    assert lib.vcrt_variance_device(m, s, 2, 2, None, o + 2, None) == INIT
    with pytest.raises(ValueError):
        vc.variance_host(mom, surf[:2])
    with pytest.raises(TypeError):
        vc.variance_host(mom, surf, sigma=1)
    with pytest.raises(vc.VcrtError):
        vc.variance_host(mom, surf, min_history=0)


def test_denoise_variance_errors_read_the_same_without_a_renderer():
    lib = N.lib()
    vc.EndRenderingOperation()
    pl = [np.zeros((4, 4, 4), F) for _ in range(3)] + [np.zeros((4, 4), F)]
    out, out_var = np.full((4, 4, 4), -1, F), np.full((4, 4), -1, F)
    ptr = [x.ctypes.data for x in pl]
    o, ov = out.ctypes.data, out_var.ctypes.data

    def calls(planes, w, h, p, o, ov):
        args = (*planes, w, h, ref(p), o, ov)
        return (lib.vcrt_denoise_variance_host(*args), lib.vcrt_denoise_variance(*args, None),
                lib.vcrt_denoise_variance_device(*args, None))

    # the parameter errors are vcrt_denoise's
    bad = [dict(struct_size=4), dict(levels=0), dict(levels=9), dict(sigma_normal=-1.0),
           dict(sigma_depth=NAN), dict(sigma_albedo=float("inf")), dict(sigma_colour=-0.5),
           dict(sigma_colour=1e-30)]
    for kw in bad:
        assert calls(ptr, 4, 4, denoise_params(**kw), o, ov) == (FORMAT,) * 3, kw
    assert calls([None] * 4, 4, 4, denoise_params(levels=0), None, None) == (FORMAT,) * 3
    for w, h in ((0, 4), (4, 0), (65536, 1), (65535, 1025)):
        assert calls(ptr, w, h, None, o, ov) == (FORMAT,) * 3
    assert calls([None] + ptr[1:], 4, 4, None, o, ov) == (INIT,) * 3       # a NULL colour
    assert calls(ptr[:3] + [None], 4, 4, None, o, ov) == (INIT,) * 3       # a NULL variance
    assert calls(ptr, 4, 4, None, None, ov) == (INIT,) * 3                 # a NULL out
    for k in range(4):  # an output equal to an input, or to the other output
        assert calls(ptr, 4, 4, None, ptr[k], ov) == (INIT,) * 3, k
        assert calls(ptr, 4, 4, None, o, ptr[k]) == (INIT,) * 3, k
    assert calls(ptr, 4, 4, None, o, o) == (INIT,) * 3
    assert (out == -1).all() and (out_var == -1).all()
    # the guides and out_variance may be NULL
    assert calls(ptr, 4, 4, None, o, ov) == (OK, INIT, INIT)
    assert calls([ptr[0], None, None, ptr[3]], 4, 4, denoise_params(), o, None) == (OK, INIT, INIT)
    for k in range(4):
        shifted = ptr[:k] + [ptr[k] + (2 if k == 3 else 4)] + ptr[k + 1:]
        assert lib.vcrt_denoise_variance_device(*shifted, 2, 2, None, o, ov, None) == INIT
    assert lib.vcrt_denoise_variance_device(*ptr, 2, 2, None, o + 4, ov, None) == INIT
    assert lib.vcrt_denoise_variance_device(*ptr, 2, 2, None, o, ov + 2, None) == INIT
    a = pl[0]
    with pytest.raises(ValueError):
        vc.denoise_variance_host(a, a)  # the variance plane has no channels
    with pytest.raises(ValueError):
        vc.denoise_variance_host(a, None)
    with pytest.raises(TypeError):
        vc.denoise_variance_host(a, pl[3], alpha=1)
    with pytest.raises(vc.VcrtError):
        vc.denoise_variance_host(a, pl[3], levels=0)


def test_cli_flag_parsing():
    """--variance is a flag (the one option without a value) and needs --temporal and --denoise:
    the tool says so before it touches a GPU."""
    import subprocess
    exe = os.path.join(N.BIN_DIR, "vcrt_render")
    res = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "[--variance]" in res.stdout + res.stderr
    for args in (["--variance"], ["--variance", "--temporal", "t.pfm"],
                 ["--denoise", "d.pfm", "--variance"], ["--width", "8", "--variance"]):
        res = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert res.returncode == 2, args
        assert "--variance needs --temporal and --denoise" in res.stderr, args
    # a flag takes no value: what follows it is parsed as the next option
    res = subprocess.run([exe, "--variance", "1", "--temporal", "t.pfm", "--denoise", "d.pfm"],
                         capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and "--variance needs" not in res.stderr
