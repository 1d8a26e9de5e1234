"""Temporal accumulation's definition on the host (vcrt_reproject_host, csrc/reproject.cpp; no
GPU): bit parity with tests/reproject_ref at every shape and parameter set over planes that hold
every special case the definition names; what the definition promises of identity motion and of
alpha = 1; and the argument errors, which read the same without a renderer."""
import ctypes
import json
import os

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import reproject_ref as P

N = vc._native
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: differs at {bad[:6].tolist()} ({len(bad)} words)"


def test_the_planes_hold_what_they_should():
    """The generated planes of the largest shapes exercise every branch of the definition."""
    for w, h in ((44, 20), (100, 37)):
        colour, motion, hcol, hsurf, hlen = P.planes(w, h)
        mx, my, mw = motion[..., 0], motion[..., 1], motion[..., 3]
        with np.errstate(invalid="ignore"):
            assert (mx <= -1).any() and (mx >= w).any() and (my <= -1).any() and (my >= h).any()
            assert ((mx > -1) & (mx < 0)).any() and ((mx > w - 1) & (mx < w)).any()
            assert ((my > -1) & (my < 0)).any() and ((my > h - 1) & (my < h)).any()
            assert ((mx == np.floor(mx)) & (mw >= 1)).any()
        for v in (np.nan, np.inf, -np.inf, 1e30):
            assert (bits(motion[..., :2]) == bits(np.asarray([v], F))[0]).any(), v
        assert (mw == 0).any() and np.isnan(mw).any()
        assert (hlen == 0).any() and (hlen == 32).any()
        taps = []
        _, length, took = P.reproject(colour, motion, hcol, hsurf, hlen, taps=taps,
                                      **P.PARAM_SETS["long-history"])
        assert 0.3 < took.mean() < 0.95
        assert (length == 32).any()  # a length at the cap
        inside = np.stack([t[0] for t in taps])
        key_ok = np.stack([t[1] for t in taps])
        len_ok = np.stack([t[2] for t in taps])
        depth_ok = np.stack([t[3] for t in taps])
        assert (inside.sum(axis=0) == 4).any() and (inside.sum(axis=0) == 1).any()
        # a key mismatch on some of a pixel's taps, not all
        assert ((inside & key_ok).any(axis=0) & (inside & ~key_ok).any(axis=0)).any()
        assert (inside & key_ok & ~len_ok).any()            # zero-length history
        assert (inside & key_ok & len_ok & ~depth_ok).any()  # a depth rejection
        assert (~took & inside.any(axis=0)).any()            # every tap of a valid pixel refused


@pytest.mark.parametrize("name", list(P.PARAM_SETS))
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_reference(shape, name):
    w, h = shape
    want, want_len, _ = P.reference(w, h, name)
    out, length = vc.reproject_host(*P.planes(w, h), **P.PARAM_SETS[name])
    same(out, want, f"{w}x{h} {name}")
    same(length, want_len, f"{w}x{h} {name} length")
    assert np.isfinite(out).all() and np.isfinite(length).all()
    same(out[..., 3], P.planes(w, h)[0][..., 3], "alpha")


def identity_motion(w, h, key=2.0, z=3.0):
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w, 4), F)
    m[..., 0], m[..., 1], m[..., 2], m[..., 3] = x, y, z, key
    return m


@pytest.mark.parametrize("shape", [(44, 20), (3, 2), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_motion_averages_exactly(shape):
    """Identity motion over one surface: a single tap of weight 1, so hcol = history and
    L = history_length exactly (x * 1 / 1), N = min(L + 1, cap); with alpha at its floor the k-th
    output is hcol + (c - hcol) / N in that order, and the length min(k, cap)."""
    w, h = shape
    rng = np.random.default_rng(7)
    m = identity_motion(w, h)
    surf = np.zeros((h, w, 4), F)
    surf[..., 0], surf[..., 1] = 2.0, 3.0
    cap = 4.0
    hist, length = None, None
    for k in range(1, 8):
        c = rng.uniform(0, 2, (h, w, 4)).astype(F)
        if hist is None:
            hist, length = c, np.ones((h, w), F)
            continue
        out, length = vc.reproject_host(c, m, hist, surf, length, alpha=2.0 ** -20,
                                        max_history=cap, depth_tolerance=0.1)
        n = F(min(k, cap))
        a = np.maximum(F(2.0 ** -20), F(1) / n)
        want = c.copy()
        want[..., :3] = hist[..., :3] + (a * (c[..., :3] - hist[..., :3]).astype(F)).astype(F)
        same(out, want, f"frame {k}")
        assert (length == n).all()
        hist = out


def test_alpha_one_gives_the_new_frame():
    """a = max(1, 1 / N) = 1: out = fl(hcol + fl(c - hcol)). The two roundings leave
    |out - c| <= 2^-24 (|c - hcol| + |c|) (1 + 2^-24), at most 2^-22 (1 + 2^-24) for planes in
    [0, 2]; where hcol lies within a factor two of c the subtraction is exact (Sterbenz) and so is
    the sum: out = c to the bit. The length still counts."""
    w, h = 44, 20
    colour, motion, hcol, hsurf, hlen = P.planes(w, h)
    out, length = vc.reproject_host(colour, motion, hcol, hsurf, hlen, alpha=1.0,
                                    max_history=9.0, depth_tolerance=0.0)
    ref, ref_len, took = P.reproject(colour, motion, hcol, hsurf, hlen, 1.0, 9.0, 0.0)
    same(out, ref)
    same(length, ref_len)
    err = np.abs(out.astype(np.float64) - colour).max()
    print("alpha = 1, largest |out - colour|", err)
    assert err <= 2.0 ** -22 * (1 + 2.0 ** -24)
    assert took.any() and (length[took] > 1).any() and (length[~took] == 1).all()
    # identity motion, one tap of weight 1: hcol is the history; within a factor two of c
    rng = np.random.default_rng(3)
    c = rng.uniform(1.0, 2.0, (h, w, 4)).astype(F)
    hist = rng.uniform(1.0, 2.0, (h, w, 4)).astype(F)
    surf = np.zeros((h, w, 4), F)
    surf[..., 0], surf[..., 1] = 2.0, 3.0
    out, length = vc.reproject_host(c, identity_motion(w, h), hist, surf, np.full((h, w), 5, F),
                                    alpha=1.0, max_history=9.0, depth_tolerance=0.1)
    same(out, c, "alpha = 1 over a history within a factor two")
    assert (length == 6).all()


def params_of(**kw):
    p = N.vcrt_reproject_params()
    N.lib().vcrt_default_reproject_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults():
    """The defaults are the grid search's choice (tools/reproject_defaults.py), which beat the
    unaccumulated frame."""
    assert vc.default_reproject_params() == pytest.approx(P.DEFAULTS)
    rec = json.load(open(os.path.join(ROOT, "profiles", "reproject_defaults.json")))
    assert rec["chosen"] == pytest.approx(vc.default_reproject_params())
    assert rec["mse_chosen"] < rec["mse_unaccumulated"]
    assert rec["fixed"]["max_history"] >= 8


def test_errors_read_the_same_without_a_renderer():
    lib = N.lib()
    vc.EndRenderingOperation()  # no renderer, whatever ran before
    pl = [np.zeros((4, 4, 4), F) for _ in range(4)] + [np.zeros((4, 4), F)]
    out, length = np.zeros((4, 4, 4), F), np.zeros((4, 4), F)
    FORMAT, INIT = N.VK_ERROR_FORMAT_NOT_SUPPORTED, N.VK_ERROR_INITIALIZATION_FAILED

    def calls(planes, w, h, p, o, ol):
        args = (*planes, w, h, None if p is None else ctypes.byref(p), o, ol)
        return (lib.vcrt_reproject_host(*args), lib.vcrt_reproject(*args, None),
                lib.vcrt_reproject_device(*args, None))

    ptr = [x.ctypes.data for x in pl]
    o, ol = out.ctypes.data, length.ctypes.data
    nan = float("nan")
    bad = [dict(struct_size=4), dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.5),
           dict(alpha=nan), dict(max_history=0.5), dict(max_history=65536.0),
           dict(max_history=nan), dict(max_history=float("inf")), dict(depth_tolerance=-1e-3),
           dict(depth_tolerance=nan)]
    for kw in bad:
        assert calls(ptr, 4, 4, params_of(**kw), o, ol) == (FORMAT,) * 3, kw
    # the parameters come first: a bad block with NULL planes is still a format error
    assert calls([None] * 5, 4, 4, params_of(alpha=0.0), None, None) == (FORMAT,) * 3
    for w, h in ((0, 4), (4, 0), (-1, 4), (65536, 1), (1, 65536), (65535, 1025)):
        assert calls(ptr, w, h, params_of(), o, ol) == (FORMAT,) * 3, (w, h)
    for k in range(5):  # a NULL input; out or out_length equal to an input
        assert calls(ptr[:k] + [None] + ptr[k + 1:], 4, 4, params_of(), o, ol) == (INIT,) * 3
        assert calls(ptr, 4, 4, params_of(), ptr[k], ol) == (INIT,) * 3
        assert calls(ptr, 4, 4, params_of(), o, ptr[k]) == (INIT,) * 3
    assert calls(ptr, 4, 4, params_of(), None, ol) == (INIT,) * 3
    assert calls(ptr, 4, 4, params_of(), o, None) == (INIT,) * 3
    assert calls(ptr, 4, 4, params_of(), o, o) == (INIT,) * 3
    # valid arguments: the host function runs (NULL params: the defaults), the GPU forms need
    # vcrt_begin
    assert calls(ptr, 4, 4, params_of(), o, ol) == (N.VK_SUCCESS, INIT, INIT)
    assert calls(ptr, 4, 4, None, o, ol) == (N.VK_SUCCESS, INIT, INIT)
    assert calls(ptr, 4, 4, params_of(alpha=1.0, max_history=1.0, depth_tolerance=0.0), o,
                 ol) == (N.VK_SUCCESS, INIT, INIT)
    # a misaligned device plane
    assert lib.vcrt_reproject_device(ptr[0] + 4, *ptr[1:], 2, 2, None, o, ol, None) == INIT
    assert lib.vcrt_reproject_device(*ptr[:4], ptr[4] + 2, 2, 2, None, o, ol, None) == INIT
    a = pl[0]
    with pytest.raises(ValueError):
        vc.reproject_host(a, a[:2], a, a, pl[4])
    with pytest.raises(ValueError):
        vc.reproject_host(a, a, a, a, a)  # the length plane has no channels
    with pytest.raises(TypeError):
        vc.reproject_host(a, a, a, a, pl[4], sigma=1)
    with pytest.raises(vc.VcrtError):
        vc.reproject_host(a, a, a, a, pl[4], alpha=0)
