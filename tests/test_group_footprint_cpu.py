"""CPU checks of the group-level footprint tables (csrc/cluster.cpp CullTables::gf_tab, tracer.hip
fact (5g)): on eligible scenes the LDS-table flat scan forms each ray's group mask from four 1-D
table lookups and pushes those groups straight onto the group stack -- no node level, no box test.
Emulated in numpy fp32 (tests/group_footprint_ref.py, with the 1-ulp errors of v_rcp / v_sqrt as
random perturbations) against what the kernel really gets (scene.cull_group_footprint): every
group the box test would keep has its bit, no group holding a member the exact test may accept
is missed, the host's tables are the ones the documented rule gives, and the eligibility decision
is the documented one. The checks have teeth: shrunk boxes and S = 0 are caught.
"""
import numpy as np
import pytest

from tests import footprint_ref as F
from tests import group_footprint_ref as G
from tests.test_cull_cpu import box_ray, member_hb_cc_disc, surface_rays
from tests.test_cull_footprint_cpu import ray_families
from tests.test_gpu_parity import culling_torture_scene
from tests.test_gpu_slab import one_height_scene
from vulkancomputeraytracing_amd import scene as S

f32 = np.float32

SCENES = {
    "final": lambda: S.builtin_scene("final"),
    "one_height": one_height_scene,
    "grid128": G.grid128,
    "grid12": G.grid12,
}

_cache = {}


def tables(name):
    if name not in _cache:
        sp = SCENES[name]()
        _cache[name] = (sp,) + G.scene_tables(sp)
    return _cache[name]


@pytest.mark.parametrize("name", list(SCENES))
def test_host_tables_follow_the_rule(name):
    """scene.cull_group_footprint's tables are those of the documented rule applied to the group
    boxes as uploaded, with the kernel's own cell function over N cells; N is what the LDS bytes of
    the group boxes and the node tables hold; padding groups have no bit; the y extent, Kmax and
    `always` are the group boxes'."""
    sp, t, gf, slab = tables(name)
    lo, hi, K, real = G.group_boxes(t)
    ng = len(lo)
    n = gf["n"]
    assert ng <= 128 and gf["tables"].shape == (4, n, 4)
    assert n == (ng // 8 * 336 + 672) // 64  # 94 at 128 groups: the LDS image keeps its size
    if name in ("final", "grid128"):
        assert ng == 128 and n == 94
    want = G.build_tables(lo, hi, real, gf["x"], gf["z"], n)
    assert np.array_equal(gf["tables"], want)
    allbits = np.zeros(4, np.uint32)
    for g in np.flatnonzero(real):
        allbits[g >> 5] |= np.uint32(1) << np.uint32(g & 31)
    assert np.array_equal(np.bitwise_or.reduce(gf["tables"].reshape(-1, 4), axis=0), allbits)
    assert np.array_equal(gf["tables"][0][-1], allbits)  # the end cells
    assert np.array_equal(gf["tables"][1][0], allbits)
    assert gf["y"][0] == lo[real, 1].min() and gf["y"][1] == hi[real, 1].max()
    finite = real & np.isfinite(K)
    assert float(gf["k2"]) >= 2.0 * float(K[finite].max())
    assert not gf["always"].any()  # no zero radius here
    if name == "grid12":
        assert int(real.sum()) == 12 and ng == 16
    if slab is not None:  # bit-equal operands: the masks cannot depend on VCRT_SLAB
        assert gf["y"][0].tobytes() == slab[0].tobytes()
        assert gf["y"][1].tobytes() == slab[1].tobytes()


def check(sp, t, gf, slab, o, d, rng, s_scale=1.0, tabs=None):
    """Violations of (5g) on rays (o, d): (groups the box test keeps without their bit, groups
    with a member the exact test may accept without their bit), then the bits set and the groups
    kept."""
    if tabs is not None:
        gf = dict(gf, tables=tabs)
    br = box_ray(t, o, d, rng)
    lo, hi, K, real = G.group_boxes(t)
    m = G.group_mask(gf, br, d, gf["y"], s_scale)
    has = G.mask_bits(m, len(lo))
    keep = G.box_keep(lo, hi, K, br) & real[None, :]
    if slab is not None:
        assert np.array_equal(keep, G.box_keep(lo, hi, K, br, slab) & real[None, :])  # (3a)
        # slab on: the kernel takes the ray's t0, t1 of the slab -- the same operands
        assert np.array_equal(G.group_mask(gf, br, d, slab, s_scale), m)
    hb, cc, disc = member_hb_cc_disc(t, o, d)
    valid = t["index"][t["nbig"]:] >= 0
    hit = ((~(disc < 0)) & (np.signbit(hb) | np.signbit(cc)) & valid[None]).any(2)  # [rays, groups]
    return int((keep & ~has).sum()), int((hit & ~has).sum()), int(has.sum()), int(keep.sum())


@pytest.mark.parametrize("name", list(SCENES))
def test_mask_holds_every_kept_group(name):
    """The superset property of (5g) on the ray families of test_cull_footprint_cpu.py: random,
    grazing, box-touching and surface-leaving rays, zero and 2^-41 direction components, d.y = 0
    inside the extent, origins at 2^20, rays that never reach the extent."""
    rng = np.random.default_rng(41)
    sp, t, gf, slab = tables(name)
    entered = kept = 0
    for o, d in ray_families(sp, t, gf, rng, 300):
        miss_keep, miss_hit, has, keep = check(sp, t, gf, slab, o, d, rng)
        assert miss_keep == 0, f"{miss_keep} groups the box test keeps without their bit"
        assert miss_hit == 0, f"{miss_hit} groups with an acceptable member without their bit"
        entered += has
        kept += keep
    print(f"{name}: {entered} mask bits for {kept} kept groups")
    assert entered <= 4 * kept + 1000  # and the mask does cull


def test_checker_catches_shrunk_boxes_and_no_slack():
    """Teeth: tables built from group boxes shrunk by 1e-4 of their size, and S = 0 with the true
    tables, both lose groups."""
    rng = np.random.default_rng(42)
    sp, t, gf, slab = tables("final")
    lo, hi, K, real = G.group_boxes(t)
    n = gf["n"]
    shrink = (hi - lo) * f32(1e-4)
    # The cells are far wider than the shrink, which shows only where a cell edge falls between a
    # box face and its shrunk twin: move the x cells so that one does, at group k's low face.
    k = int(np.flatnonzero(real)[29])
    xb = float(lo[k, 0]) + 0.5 * float(shrink[k, 0])
    m = int(F.cell(f32(xb), gf["x"], n))
    # (The per-box margin K c2 alone is wider than the shrink: none here, k2 = 0, and the
    # yardstick is the members the exact test may accept.)
    gfx = dict(gf, x=np.array([gf["x"][0], m - xb * float(gf["x"][0])], f32), k2=f32(0))
    good = G.build_tables(lo, hi, real, gfx["x"], gfx["z"], n)
    bad = G.build_tables(lo + shrink, hi - shrink, real, gfx["x"], gfx["z"], n)
    # rays in the plane a quarter of the shrink inside that face, through the member that touches
    # it (a disc of radius sqrt(2 r shrink / 4) of that sphere lies in the plane)
    mem = t["index"][t["nbig"] + k]
    mem = mem[mem >= 0]
    j = mem[np.argmin(sp["center"][mem, 0] - np.abs(sp["radius"][mem]))]
    c = sp["center"][j].astype(np.float64)
    os_, ds_ = [], []
    for _ in range(300):
        q = np.array([float(lo[k, 0]) + 0.25 * float(shrink[k, 0]), c[1], c[2]])
        dv = np.array([0.0, rng.uniform(-0.02, 0.02), rng.choice([-1.0, 1.0])])
        os_.append(q - rng.uniform(0.5, 3.0) * dv)
        ds_.append(dv * rng.choice([0.3, 1.0, 5.0]))
    o, d = np.array(os_, f32), np.array(ds_, f32)
    assert check(sp, t, gfx, slab, o, d, rng, tabs=good)[1] == 0
    assert check(sp, t, gfx, slab, o, d, rng, tabs=bad)[1] > 0
    # S = 0: a ray whose y interval just misses its (margin-grown) slab overlap
    o2, d2 = ray_families(sp, t, gf, rng, 2000)[-1]
    o3, d3 = surface_rays(sp, 4000, rng)
    lost = check(sp, t, gf, slab, o2, d2, rng, s_scale=0.0)[0] + \
        check(sp, t, gf, slab, o3, d3, rng, s_scale=0.0)[0] + \
        check(sp, t, gf, slab, o, d, rng, s_scale=0.0)[0]
    assert lost > 0


ELIGIBLE = {
    "final": (lambda: S.builtin_scene("final"), True),
    "one_height": (one_height_scene, True),
    "grid128": (G.grid128, True),
    "grid12": (G.grid12, True),
    "one_height_ulp": (lambda: one_height_scene(True), False),
    "tall": (F.tall_scene, False),
    "torture": (culling_torture_scene, False),
    "grid129": (G.grid129, False),
}


@pytest.mark.parametrize("name", list(ELIGIBLE))
@pytest.mark.parametrize("slab", ["1", "0"])
def test_eligibility(monkeypatch, name, slab):
    """At most 128 hierarchy groups and one y extent in every group box with members -- the
    geometric condition, the same answer whatever VCRT_SLAB says; VCRT_GROUP_FOOT=0 turns it off."""
    make, want = ELIGIBLE[name]
    sp = make()
    monkeypatch.setenv("VCRT_SLAB", slab)
    monkeypatch.delenv("VCRT_GROUP_FOOT", raising=False)
    if slab == "0":
        assert S.cull_slab(sp) is None
    gf = S.cull_group_footprint(sp)
    assert (gf is not None and gf["eligible"]) == want
    if name == "grid129":
        t = S.cull_tables(sp)
        assert gf is None and t["geom"].shape[0] - t["nbig"] == 144
        assert int((t["index"][t["nbig"]:] >= 0).any(1).sum()) == 129
    if want:
        monkeypatch.setenv("VCRT_GROUP_FOOT", "0")
        off = S.cull_group_footprint(sp)
        assert not off["eligible"]
        assert np.array_equal(off["tables"], gf["tables"])  # the knob is the decision alone


def test_undescribable_scene_keeps_every_group():
    """Coordinates below the 2^-20 of the proof: every mask is the groups with members."""
    sp = G.tiny_grid()
    t, gf, _ = G.scene_tables(sp)
    real = (t["index"][t["nbig"]:] >= 0).any(1)
    assert int(real.sum()) == 80 and gf["eligible"]
    want = np.zeros(4, np.uint32)
    for g in np.flatnonzero(real):
        want[g >> 5] |= np.uint32(1) << np.uint32(g & 31)
    assert (gf["tables"] == want[None, None, :]).all() and np.array_equal(gf["always"], want)
