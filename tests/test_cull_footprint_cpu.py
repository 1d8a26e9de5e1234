"""CPU checks of the footprint tables (csrc/cluster.cpp CullTables::fp_tab, tracer.hip fact (5)):
the LDS-table flat scan forms each ray's node mask from four 1-D table lookups in place of the
node box tests. Emulated in numpy fp32 (tests/footprint_ref.py, with the 1-ulp errors of v_rcp /
v_sqrt as random perturbations) against what the kernel really gets (scene.cull_footprint):
every node the present box test keeps has its bit, no node holding a member the exact test may
accept is missed, the masks are bit-equal with the slab on and off, and the host's tables are the
ones the documented rule gives. The checks have teeth: shrunk boxes and S = 0 are caught.
"""
import numpy as np
import pytest

from tests import footprint_ref as F
from tests.test_cull_cpu import (box_ray, grazing_rays, member_hb_cc_disc, random_rays,
                                 surface_rays, tangent_rays)
from tests.test_gpu_parity import culling_torture_scene
from tests.test_gpu_slab import one_height_scene
from vulkancomputeraytracing_amd import scene as S

f32 = np.float32

SCENES = {
    "final": lambda: S.builtin_scene("final"),
    "one_height": one_height_scene,
    "one_height_ulp": lambda: one_height_scene(True),
    "torture": culling_torture_scene,
    "tall": F.tall_scene,
    "many_groups": F.many_groups_scene,
}

_cache = {}


def tables(name):
    if name not in _cache:
        sp = SCENES[name]()
        _cache[name] = (sp,) + F.scene_tables(sp)
    return _cache[name]


def ray_families(sp, t, fp, rng, n):
    """Random, grazing, box-touching and surface-leaving rays, then the special ones: a direction
    component exactly 0 and at 2^-41, d.y = 0 inside the y extent, origins at 2^20, and rays that
    never reach the y extent."""
    out = [random_rays(n, rng, -20.0, 20.0), random_rays(n, rng, -2.0, 2.0),
           grazing_rays(sp, n, rng), tangent_rays(sp, t, n, rng), surface_rays(sp, n, rng)]
    ylo, yhi = float(fp["y"][0]), float(fp["y"][1])
    o, d = random_rays(8 * n, rng, -12.0, 12.0)
    kind = np.arange(8 * n) % 8
    d[kind == 0, 0] = 0.0
    d[kind == 1, 2] = -0.0
    d[kind == 2, 0] = f32(2.0 ** -41)
    d[kind == 3, 2] = f32(-2.0 ** -41)
    inside = (kind == 4) | (kind == 5)
    o[inside, 1] = rng.uniform(ylo, yhi, int(inside.sum())).astype(f32)
    d[kind == 4, 1] = 0.0
    d[kind == 5, 1] = f32(2.0 ** -41)
    far = kind == 6  # origins at 2^20, aimed at the scene or anywhere
    o[far] = (rng.choice([-1.0, 1.0], (int(far.sum()), 3)) * 2.0 ** 20).astype(f32)
    d[far & (np.arange(8 * n) % 16 == 6)] = -o[far & (np.arange(8 * n) % 16 == 6)] * f32(1e-3)
    away = kind == 7  # above the extent and rising, or below and falling
    up = rng.integers(0, 2, int(away.sum())).astype(bool)
    o[away, 1] = np.where(up, yhi + rng.uniform(0.01, 5, len(up)), ylo - rng.uniform(0.01, 5, len(up)))
    d[away, 1] = np.where(up, 1, -1) * np.abs(d[away, 1]) + np.where(up, 1e-3, -1e-3)
    out.append((o, d))
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_host_tables_follow_the_rule(name):
    """scene.cull_footprint's tables are those of the documented rule applied to the node boxes
    as uploaded, with the kernel's own cell function; padding nodes have no bit; the y extent, Kmax
    and `always` are the node boxes'."""
    sp, t, fp, slab = tables(name)
    lo, hi, K, real = F.node_boxes(t)
    n = fp["tables"].shape[1]
    assert len(lo) <= 32
    want = F.build_tables(lo, hi, real, fp["x"], fp["z"], n)
    assert np.array_equal(fp["tables"], want)
    allbits = int(np.bitwise_or.reduce(np.where(real, 1 << np.arange(len(lo)), 0)))
    assert int(np.bitwise_or.reduce(fp["tables"].reshape(-1))) == allbits
    assert fp["tables"][0][-1] == allbits and fp["tables"][1][0] == allbits  # the end cells
    assert fp["y"][0] == lo[real, 1].min() and fp["y"][1] == hi[real, 1].max()
    finite = real & np.isfinite(K)
    assert float(fp["k2"]) >= 2.0 * float(K[finite].max())
    assert fp["always"] == int(np.bitwise_or.reduce(
        np.where(real & np.isinf(K), 1 << np.arange(len(lo)), 0)))
    if slab is not None:  # bit-equal operands: the masks cannot depend on VCRT_SLAB
        assert fp["y"][0].tobytes() == slab[0].tobytes()
        assert fp["y"][1].tobytes() == slab[1].tobytes()
    if name == "many_groups":
        assert len(lo) > 16 and 128 < t["geom"].shape[0] - t["nbig"] <= 256


def test_tables_do_not_depend_on_the_slab_knob(monkeypatch):
    sp = S.builtin_scene("final")
    monkeypatch.setenv("VCRT_SLAB", "1")
    on = S.cull_footprint(sp)
    monkeypatch.setenv("VCRT_SLAB", "0")
    assert S.cull_slab(sp) is None
    off = S.cull_footprint(sp)
    for k in on:
        assert np.array_equal(np.asarray(on[k]), np.asarray(off[k])), k
    assert S.cull_footprint(S.builtin_scene("three")) is None  # no culling tables at all


def test_undescribable_scene_gets_all_ones():
    """A scene whose coordinates lie below the bound the proof needs (max |box coordinate| <
    2^-20) keeps every node for every ray: all-ones tables and `always`."""
    fp = S.cull_footprint(F.tiny_scene())
    assert fp is not None and fp["always"] == 0xffffffff
    assert (fp["tables"] == np.uint32(0xffffffff)).all()
    assert fp["x"][0] == 1 and fp["x"][1] == 0 and fp["z"][0] == 1 and fp["z"][1] == 0


def check(sp, t, fp, slab, o, d, rng, s_scale=1.0, tabs=None):
    """Violations of the footprint's contract on rays (o, d): (kept nodes without their bit,
    nodes with an acceptable member without their bit)."""
    if tabs is not None:
        fp = dict(fp, tables=tabs)
    br = box_ray(t, o, d, rng)
    _, _, _, real = F.node_boxes(t)
    mask = F.foot_mask(fp, br, d, fp["y"], s_scale)
    nn = len(real)
    has = ((mask[:, None] >> np.arange(nn, dtype=np.uint32)[None, :]) & 1).astype(bool)
    keep = F.node_keep(t, br) & real[None, :]
    if slab is not None:
        keep_s = F.node_keep(t, br, slab) & real[None, :]
        assert np.array_equal(keep, keep_s)  # (3a)
        # slab on: the kernel takes the ray's t0, t1 of the slab -- the same operands
        assert np.array_equal(F.foot_mask(fp, br, d, slab, s_scale), mask)
    hb, cc, disc = member_hb_cc_disc(t, o, d)
    valid = t["index"][t["nbig"]:] >= 0
    hit = ((~(disc < 0)) & (np.signbit(hb) | np.signbit(cc)) & valid[None]).any(2)  # [rays, groups]
    node_hit = hit.reshape(len(o), nn, 8).any(2)
    return int((keep & ~has).sum()), int((node_hit & ~has).sum()), int(has.sum()), int(keep.sum())


@pytest.mark.parametrize("name", list(SCENES))
def test_mask_holds_every_kept_node(name):
    rng = np.random.default_rng(31)
    sp, t, fp, slab = tables(name)
    entered = kept = 0
    for o, d in ray_families(sp, t, fp, rng, 300):
        miss_keep, miss_hit, has, keep = check(sp, t, fp, slab, o, d, rng)
        assert miss_keep == 0, f"{miss_keep} nodes the box test keeps without their bit"
        assert miss_hit == 0, f"{miss_hit} nodes with an acceptable member without their bit"
        entered += has
        kept += keep
    print(f"{name}: {entered} mask bits for {kept} kept nodes")
    if name in ("final", "one_height", "many_groups"):
        assert entered <= 2 * kept + 100  # and the mask does cull


def test_checker_catches_shrunk_boxes_and_no_slack():
    """Teeth: tables built from node boxes shrunk by 1e-4 of their size, and S = 0 with the true
    tables, both lose nodes that the box test keeps."""
    rng = np.random.default_rng(32)
    sp, t, fp, slab = tables("final")
    lo, hi, K, real = F.node_boxes(t)
    n = fp["tables"].shape[1]
    shrink = (hi - lo) * f32(1e-4)
    # The cells are far wider than the shrink, which shows only where a cell edge falls between a
    # box face and its shrunk twin: move the x cells so that one does, at node k's low face.
    k = int(np.flatnonzero(real)[3])
    xb = float(lo[k, 0]) + 0.5 * float(shrink[k, 0])
    m = int(F.cell(f32(xb), fp["x"], n))
    # (The per-box margin K c2 alone is wider than the shrink, as in test_cull_cpu.py's teeth
    # test: none here, k2 = 0, and the yardstick is the members the exact test may accept.)
    fpx = dict(fp, x=np.array([fp["x"][0], m - xb * float(fp["x"][0])], f32), k2=f32(0))
    good = F.build_tables(lo, hi, real, fpx["x"], fpx["z"], n)
    bad = F.build_tables(lo + shrink, hi - shrink, real, fpx["x"], fpx["z"], n)
    # rays in the plane a quarter of the shrink inside that face, through the member that touches
    # it (a disc of radius sqrt(2 r shrink / 4) ~ 7e-3 of that sphere lies in the plane)
    mem = t["index"][t["nbig"] + 8 * k:t["nbig"] + 8 * k + 8].reshape(-1)
    mem = mem[mem >= 0]
    j = mem[np.argmin(sp["center"][mem, 0] - np.abs(sp["radius"][mem]))]
    c = sp["center"][j].astype(np.float64)
    os_, ds_ = [], []
    for _ in range(200):
        q = np.array([float(lo[k, 0]) + 0.25 * float(shrink[k, 0]), c[1], c[2]])
        dv = np.array([0.0, rng.uniform(-0.05, 0.05), rng.choice([-1.0, 1.0])])
        os_.append(q - rng.uniform(0.5, 3.0) * dv)
        ds_.append(dv * rng.choice([0.3, 1.0, 5.0]))
    o, d = np.array(os_, f32), np.array(ds_, f32)
    assert check(sp, t, fpx, slab, o, d, rng, tabs=good)[1] == 0
    assert check(sp, t, fpx, slab, o, d, rng, tabs=bad)[1] > 0
    # S = 0: a ray whose y interval just misses its (margin-grown) slab overlap
    o2, d2 = ray_families(sp, t, fp, rng, 2000)[-1]
    o3, d3 = surface_rays(sp, 4000, rng)
    lost = check(sp, t, fp, slab, o2, d2, rng, s_scale=0.0)[0] + \
        check(sp, t, fp, slab, o3, d3, rng, s_scale=0.0)[0] + \
        check(sp, t, fp, slab, o, d, rng, s_scale=0.0)[0]
    assert lost > 0
