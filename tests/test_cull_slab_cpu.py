"""CPU checks of the flat scans' shared y slab (csrc/cluster.cpp CullTables::slab, tracer.hip
fact (3a)): which scenes are eligible, and that the hoisted box test -- the two y planes
evaluated once per ray, their clamped interval joined to each box's x and z planes -- gives the
three-axis test's fp32 gap bit for bit on every box that has members, in the near/far form (node
level and passes) and in the min/max form (chunk-pair boxes), emulated in numpy with the helpers
of test_cull_cpu.py.
"""
import numpy as np
import pytest

from tests.test_cull_cpu import (box_ray, fma, grazing_rays, group_gap, random_rays, rn,
                                 surface_rays, tangent_rays)
from tests.test_gpu_parity import culling_torture_scene
from tests.test_gpu_slab import one_height_scene
from vulkancomputeraytracing_amd import scene as S

f32 = np.float32


def outward(x):
    """(largest float <= x, smallest float >= x) of a double, as cluster.cpp rounds a box."""
    f = f32(x)
    lo = np.nextafter(f, f32(-np.inf)) if float(f) > x else f
    hi = np.nextafter(f, f32(np.inf)) if float(f) < x else f
    return lo, hi


@pytest.mark.parametrize("name", ["final", "stress4096"])
def test_generated_scenes_share_their_slab(name):
    lohi = S.cull_slab(S.builtin_scene(name))
    assert lohi is not None
    assert lohi[0].tobytes() == f32(0.0).tobytes() and lohi[1].tobytes() == f32(0.4).tobytes()
    # and that is every box with members of all three levels
    t = S.cull_tables(S.builtin_scene(name))
    for key in ("bound", "node", "top"):
        b = t[key]
        real = b[:, 0:2] != f32(1e20)
        assert real.any()
        assert (b[:, 2:4][real].view(np.uint32) == lohi[0].view(np.uint32)).all(), key
        assert (b[:, 8:10][real].view(np.uint32) == lohi[1].view(np.uint32)).all(), key


def test_custom_scene_eligibility(monkeypatch):
    sp = one_height_scene()
    lohi = S.cull_slab(sp)
    c, r = float(sp["center"][0, 1]), float(sp["radius"][0])
    assert lohi is not None and lohi[0] == outward(c - r)[0] and lohi[1] == outward(c + r)[1]
    assert lohi != (f32(0.0), f32(0.4))  # its own extent
    # one centre's y moved by one ulp: its group's box differs, no shared slab
    assert S.cull_slab(one_height_scene(perturb=True)) is None
    assert S.cull_slab(culling_torture_scene()) is None
    assert S.cull_slab(S.builtin_scene("three")) is None  # no culling tables at all
    monkeypatch.setenv("VCRT_SLAB", "0")
    assert S.cull_slab(sp) is None
    assert S.cull_slab(S.builtin_scene("final")) is None
    monkeypatch.setenv("VCRT_SLAB", "1")
    assert S.cull_slab(sp) is not None


def slab_gap(t, lohi, o, d, key, near_far):
    """[rays, boxes] fp32 gaps of the hoisted test (tracer.hip box_ray's slab interval, then
    push_bound_pair_nf<true> (near_far) or box_gap<true>)."""
    b = t[key]
    G = 2 * b.shape[0]
    cols = lambda k: np.stack([b[:, k], b[:, k + 1]], 1).reshape(G)  # noqa: E731
    inv, c, c1, c2 = box_ray(t, o, d)
    n = len(o)
    tly = fma(np.full(n, lohi[0], f32), inv[:, 1], c[:, 1])
    thy = fma(np.full(n, lohi[1], f32), inv[:, 1], c[:, 1])
    t0 = np.maximum(np.minimum(tly, thy), f32(0))  # once per ray, the clamp of (4) included
    t1 = np.maximum(tly, thy)
    tn = tf = None
    for k in (0, 2):
        tl = fma(cols(2 * k)[None, :], inv[:, k, None], c[:, k, None])
        th = fma(cols(6 + 2 * k)[None, :], inv[:, k, None], c[:, k, None])
        if near_far:
            neg = np.signbit(inv[:, k, None])
            near, far = np.where(neg, th, tl), np.where(neg, tl, th)
        else:
            near, far = np.minimum(tl, th), np.maximum(tl, th)
        tn = near if tn is None else np.maximum(tn, near)
        tf = far if tf is None else np.minimum(tf, far)
    tn = np.maximum(tn, t0[:, None])
    tf = np.minimum(tf, t1[:, None])
    K = cols(12)
    with np.errstate(over="ignore", invalid="ignore"):
        return fma(np.broadcast_to(K[None, :], tn.shape), np.broadcast_to(c2[:, None], tn.shape),
                   rn(rn(tf - tn) + c1[:, None]))


def slab_rays(sp, t, lohi, rng, n):
    """The ray families of test_cull_cpu.py, then rays built for the y axis: d.y exactly +-0,
    |d.y| below the 2^-40 clamp, d.y < 0, and origins inside, on and outside the slab."""
    chunks = [random_rays(n, rng, -20.0, 20.0), grazing_rays(sp, n, rng),
              tangent_rays(sp, t, n, rng), surface_rays(sp, n, rng)]
    o, d = random_rays(6 * n, rng, -12.0, 12.0)
    lo, hi = float(lohi[0]), float(lohi[1])
    ys = [0.5 * (lo + hi), lo, hi, np.nextafter(f32(hi), f32(9)), hi + 5.0, lo - 3.0]
    o[:, 1] = np.repeat(np.array(ys, f32), n)  # inside, on (both faces), just outside, outside
    kind = np.arange(6 * n) % 6
    d[kind == 0, 1] = 0.0
    d[kind == 1, 1] = -0.0
    d[kind == 2, 1] = f32(2.0 ** -45)
    d[kind == 3, 1] = f32(-2.0 ** -41)
    d[kind == 4, 1] = -np.abs(d[kind == 4, 1])
    chunks.append((o, d))
    return chunks


@pytest.mark.parametrize("name", ["final", "stress4096", "one_height"])
def test_hoisted_gap_equals_three_axis_gap(name):
    rng = np.random.default_rng(21)
    sp = one_height_scene() if name == "one_height" else S.builtin_scene(name)
    t = S.cull_tables(sp)
    lohi = S.cull_slab(sp)
    n = 150 if name == "stress4096" else 400
    for key in ("bound", "node", "top"):
        real = (t[key][:, 0:2] != f32(1e20)).reshape(-1)  # boxes with members
        assert real.any()
        for o, d in slab_rays(sp, t, lohi, rng, n):
            for near_far in (True, False):
                want = group_gap(t, o, d, key, near_far)[:, real]
                got = slab_gap(t, lohi, o, d, key, near_far)[:, real]
                assert np.array_equal(np.signbit(got), np.signbit(want)), (key, near_far)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (key, near_far)


def test_gap_check_has_teeth():
    """The comparison above notices a slab that is off by one ulp."""
    rng = np.random.default_rng(22)
    sp = S.builtin_scene("final")
    t = S.cull_tables(sp)
    lohi = S.cull_slab(sp)
    off = (lohi[0], np.nextafter(lohi[1], f32(1)))
    real = (t["bound"][:, 0:2] != f32(1e20)).reshape(-1)
    o, d = random_rays(400, rng, -20.0, 20.0)
    want = group_gap(t, o, d, "bound", True)[:, real]
    assert np.array_equal(slab_gap(t, lohi, o, d, "bound", True)[:, real], want)
    assert not np.array_equal(slab_gap(t, off, o, d, "bound", True)[:, real], want)
