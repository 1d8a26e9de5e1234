"""update_spheres on the host (no GPU): the bindings, the host restatement of a refit
(scene.refit_table) against today's table functions, and the refitted tables' conservativeness
under every move of tests/scene_update_ref.py."""
import ctypes

import numpy as np
import pytest

from tests import scene_update_ref as U
from tests import test_cull_cpu as C
from vulkancomputeraytracing_amd import _native as N
from vulkancomputeraytracing_amd import scene as S

f32 = np.float32
SCENES = ("final", "stress4096", "twenty")
_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = U.twenty() if name == "twenty" else S.builtin_scene(name)
    return _scenes[name]


_tables = {}


def refit(name, move):
    """Every refit table of scene `name` under a move; computed once."""
    if (name, move) not in _tables:
        s = scene(name)
        _tables[name, move] = U.tables(s, U.MOVES[move](s))
    return _tables[name, move]


# ---- 1. bindings ---------------------------------------------------------------------------

def test_symbols_and_bindings_exist():
    lib = N.lib()
    for sym in ("vcrt_update_spheres", "vcrt_update_spheres_device",
                "vcrt_get_scene_update_stats", "vcrt_scene_table_host", "vcrt_scene_table_read"):
        assert sym in N.SIGNATURES and hasattr(lib, sym)
    import vulkancomputeraytracing_amd as vc
    for attr in ("update_spheres", "scene_update_stats", "scene_table"):
        assert callable(getattr(vc.Renderer, attr))
    assert callable(S.refit_table)
    assert ctypes.sizeof(N.vcrt_scene_update_stats) == 56


def test_calls_before_begin_fail_without_touching_the_gpu():
    lib = N.lib()
    lib.vcrt_end()
    s = scene("twenty")
    bad = N.VK_ERROR_INITIALIZATION_FAILED
    assert lib.vcrt_update_spheres(s.ctypes.data, len(s)) == bad
    assert lib.vcrt_update_spheres_device(s.ctypes.data, len(s)) == bad
    assert lib.vcrt_update_spheres(None, 3) == bad
    st = N.vcrt_scene_update_stats()
    assert lib.vcrt_get_scene_update_stats(ctypes.byref(st)) == bad
    assert lib.vcrt_scene_table_read(0, None, 0) == bad


# ---- 2. the refit of an unmoved scene is today's tables ------------------------------------

def linear_numpy(s):
    n = len(s)
    groups = (n + 3) // 4 + 1
    t = np.zeros((groups, 16), f32)
    flat = np.zeros((4 * groups, 4), f32)
    flat[:, 3] = f32(-3.0e38)
    flat[:n, :3] = s["center"]
    flat[:n, 3] = s["radius"] * s["radius"]
    for j in range(4):  # entry j of a group: pair j // 2, element j % 2
        for k in range(4):
            t[:, 8 * (j // 2) + 2 * k + j % 2] = flat[j::4, k]
    return t.reshape(-1)


def pack_foot(tables, ngroups):
    flat = tables.reshape(-1)
    if ngroups > 128:
        return flat
    return (flat[0::2] & np.uint32(0xFFFF)) | (flat[1::2] << np.uint32(16))


def near_far(pairs):
    b = pairs.reshape(-1, 16)
    o = np.zeros((len(b), 20), f32)
    for a in range(3):
        o[:, 6 * a + 0] = o[:, 6 * a + 4] = b[:, 2 * a]
        o[:, 6 * a + 1] = o[:, 6 * a + 5] = b[:, 2 * a + 1]
        o[:, 6 * a + 2] = b[:, 6 + 2 * a]
        o[:, 6 * a + 3] = b[:, 6 + 2 * a + 1]
    o[:, 18], o[:, 19] = b[:, 12], b[:, 13]
    return o.reshape(-1)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("name", SCENES)
def test_refit_of_the_unmoved_scene_is_todays_tables(name):
    s = scene(name)
    t = refit(name, "identity")
    ct = S.cull_tables(s)
    same(t["linear"], linear_numpy(s), "linear")
    same(t["center_radius"].reshape(-1, 4), np.column_stack([s["center"], s["radius"]]), "rows")
    same(t["shade"].reshape(-1, 4), np.column_stack([s["colour"], s["texture"][:, 1]]), "shade")
    ior = s["texture"][:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        r0 = (f32(1) - ior) / (f32(1) + ior)
        mat = np.column_stack([s["texture"][:, 0], f32(1) / ior, r0 * r0, np.zeros_like(ior)])
    same(t["material"].reshape(-1, 4), mat.astype(f32), "material")
    g = t["groups"].reshape(-1, 20)
    same(g[:, :16], ct["geom"], "group geometry")
    same(g[:, 16:].view(np.int32), ct["index"], "group index words")
    for key in ("bound", "node", "top"):
        same(t[key].reshape(-1, 16), ct[key], key)
    same(t["bound_nf"], near_far(ct["bound"]), "bound_nf")
    nodes = np.zeros(((len(ct["node"]) + 3) // 4 * 4, 16), f32)
    nodes[:len(ct["node"])] = ct["node"]
    same(t["node_nf"], near_far(nodes), "node_nf")
    sc = t["scalars"]
    ngroups = 2 * len(ct["bound"])
    assert (sc["nbig"], sc["ngroups"]) == (ct["nbig"], ngroups)
    same(np.array(sc["margin"], f32), ct["margin"], "margin")
    slab = S.cull_slab(s)
    assert sc["slab_on"] == (slab is not None)
    if slab is not None:
        same(np.array(sc["slab"], f32), np.array(slab, f32), "slab")
    fp = S.cull_footprint(s)
    same(t["foot"], pack_foot(fp["tables"], ngroups), "foot")
    for key in ("x", "z", "y"):
        same(np.array(sc["fp_" + key], f32), fp[key], "fp_" + key)
    assert sc["fp_k2"].tobytes() == fp["k2"].tobytes() and sc["fp_always"] == fp["always"]
    gf = S.cull_group_footprint(s)
    assert (t["group_foot"] is None) == (gf is None) and sc["gf_n"] == (gf["n"] if gf else 0)
    if gf:
        same(t["group_foot"], gf["tables"].reshape(-1), "group_foot")
        same(np.array(sc["gf_x"], f32), gf["x"], "gf_x")
        same(np.array(sc["gf_z"], f32), gf["z"], "gf_z")
        assert sc["gf_k2"].tobytes() == gf["k2"].tobytes()
        assert sc["gf_always"] == tuple(int(v) for v in gf["always"])
        assert bool(sc["gf_ok"]) == gf["eligible"]
    assert (sc["bounded"], sc["radii_safe"]) == (1, 1)


@pytest.mark.parametrize("move", U.REFIT_MOVES)
@pytest.mark.parametrize("name", SCENES)
def test_the_grouping_is_kept(name, move):
    base = refit(name, "identity")["groups"].reshape(-1, 20)[:, 16:]
    got = refit(name, move)["groups"].reshape(-1, 20)[:, 16:]
    same(got, base, f"{name} {move}: index words")


def test_unbounded_values_have_no_tables():
    s = scene("final")
    moved = U.unbounded(s)
    assert S.refit_table(s, moved, "groups") is None and S.refit_table(s, moved, "scalars") is None
    assert S.refit_table(s, moved, "linear") is not None
    with pytest.raises(ValueError):
        S.refit_table(s, moved[:-1], "linear")


# ---- 3. refitted tables are conservative ---------------------------------------------------

@pytest.mark.parametrize("name,move", [("final", m) for m in U.REFIT_MOVES] +
                         [("stress4096", "drift"), ("stress4096", "swap"), ("twenty", "resize")])
def test_refitted_boxes_are_conservative(name, move):
    """tests/test_cull_cpu.py's fp32 emulation of the kernels' box tests, its rays against the
    moved scene: every member the exact test may accept lies in a group, node and chunk the
    refitted hierarchy keeps."""
    rng = np.random.default_rng(23)
    moved = U.MOVES[move](scene(name))
    t = U.cull_dict(refit(name, move))
    valid = t["index"][t["nbig"]:] >= 0
    n = 600 if name == "stress4096" else 1500
    chunks = [C.grazing_rays(moved, n, rng), C.tangent_rays(moved, t, n, rng),
              C.random_rays(n, rng, -20.0, 20.0), C.surface_rays(moved, n, rng)]
    checked = 0
    for o, d in chunks:
        hb, cc, disc = C.member_hb_cc_disc(t, o, d)
        hit = (~(disc < 0)) & (np.signbit(hb) | np.signbit(cc)) & valid[None]
        G = hit.shape[1]
        for key, per in (("bound", 1), ("node", 8), ("top", 64)):
            culled = np.repeat(C.group_culled(t, o, d, key, rng=rng), per, axis=1)[:, :G]
            bad = culled[:, :, None] & hit
            assert not bad.any(), f"{name} {move}: {int(bad.sum())} accepted members under " \
                                  f"a culled {key} box"
        checked += int(hit.sum())
    assert checked > 0


# ---- 4-6. what each move changes -----------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_materials_change_only_the_shading_rows(name):
    base, got = refit(name, "identity"), refit(name, "materials")
    changed = {k for k in base if base[k] is not None and (
        base[k] != got[k] if isinstance(base[k], dict) else base[k].tobytes() != got[k].tobytes())}
    assert changed == {"shade", "material"}


def test_bounce_breaks_the_slab_and_the_one_height():
    base, got = refit("final", "identity")["scalars"], refit("final", "bounce")["scalars"]
    assert (base["slab_on"], base["gf_ok"]) == (1, 1)
    assert (got["slab_on"], got["gf_ok"]) == (0, 0)
    assert got["gf_n"] == base["gf_n"] and got["slab"] == (f32(0), f32(0))
    assert got["fp_y"][1] > base["fp_y"][1]


def test_resize_sets_always_bits_and_an_infinite_K():
    t = refit("final", "resize")
    sc = t["scalars"]
    K = t["bound"].reshape(-1, 16)[:, 12:14].reshape(-1)
    inf_groups = np.flatnonzero(np.isinf(K))
    assert len(inf_groups) == 1
    gi = int(inf_groups[0])
    assert sc["gf_always"][gi >> 5] == 1 << (gi & 31)
    assert sc["fp_always"] == 1 << (gi // 8)
    assert np.isinf(t["node"].reshape(-1, 16)[:, 12:14].reshape(-1)[gi // 8])
    assert np.isinf(t["top"].reshape(-1, 16)[:, 12:14].reshape(-1)[gi // 64])
    assert refit("final", "identity")["scalars"]["gf_always"] == (0, 0, 0, 0)
    assert sc["radii_safe"] == 0 and sc["bounded"] == 1
