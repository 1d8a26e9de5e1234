"""Occlusion queries on the GPU (vcrt_occlude_rays, Renderer.occluded / visible): one bit per ray,
equal to the numpy restatement of the contract (tests/occlusion_ref.py) for per-ray reaches that
fall on, just above and just below accepted roots; independence of order, split, wave mates and
render description; no effect on frames; the bounds of what the device path writes."""
import ctypes

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import occlusion_ref as Q
from tests import ray_query_ref as R

pytestmark = pytest.mark.gpu
N = vc._native

FRAME = dict(width=64, height=40, samples_per_pixel=1, max_depth=10, device=0)

_gpu = {}


def final_answers(oracle):
    """The whole batch on the final scene from one call: (occluded, stats)."""
    if "final" not in _gpu:
        O, D, _ = R.ray_batch(oracle)
        T = Q.reference(oracle, "final")["T"]
        with vc.Renderer(vc.RenderDesc(**FRAME), "final") as r:
            _gpu["final"] = r.occluded(O, D, T, stats=True)
    return _gpu["final"]


def check(got, ref, sel=slice(None), what=""):
    fin = ref["finite"][sel]
    want = ref["occ"][sel]
    assert got.dtype == np.bool_ and got.shape == want.shape, what
    bad = np.nonzero((got != want) & fin)[0]
    assert bad.size == 0, f"{what}: rays {bad[:8]} of {bad.size} differ (kinds " \
                          f"{ref['kind'][sel][bad[:8]]})"


@pytest.mark.parametrize("scene", R.SCENES)
def test_parity(oracle, scene):
    O, D, _ = R.ray_batch(oracle)
    ref = Q.reference(oracle, scene)
    if scene == "final":
        occ, st = final_answers(oracle)
    else:
        with vc.Renderer(vc.RenderDesc(**FRAME), R.scene_of(oracle, scene)) as r:
            occ, st = r.occluded(O, D, ref["T"], stats=True)
    check(occ, ref, what=scene)
    assert np.all(occ.view(np.uint8) <= 1)  # the other rays too: 0 or 1
    assert st["kernel"] == "vcrt_occlude_rays" and st["segments"] == R.N_RAYS
    assert st["group_tests"] > 0 and st["kernel_ms"] > 0
    if scene == "three":  # no culling tables: the linear scan only
        assert st["bound_tests"] == 0
    else:
        assert st["bound_tests"] > 0


def test_default_reach(oracle):
    O, D, _ = R.ray_batch(oracle)
    ref = Q.reference(oracle, "final")
    fin = ref["finite"]
    with vc.Renderer(vc.RenderDesc(**FRAME), "final") as r:
        occ = r.occluded(O, D)
        _, hits = r.trace_rays(O, D, 1, hits=True)
        scalar = r.occluded(O, D, 1e5)
    assert np.array_equal(occ[fin], (hits["sphere"] >= 0)[fin])
    assert np.array_equal(occ[fin], ref["occ_default"][fin])
    assert np.array_equal(scalar, occ)  # a scalar reach is broadcast; 1e5 is the default


def test_order_and_split(oracle):
    O, D, _ = R.ray_batch(oracle)
    T = Q.reference(oracle, "final")["T"]
    want, _ = final_answers(oracle)
    perm = np.random.default_rng(7).permutation(R.N_RAYS)
    with vc.Renderer(vc.RenderDesc(**FRAME), "final") as r:
        got = r.occluded(O[perm], D[perm], T[perm])
        bad = np.nonzero(got != want[perm])[0]
        assert bad.size == 0, f"permuted: rays {perm[bad][:8]} differ ({bad.size})"
        start = 0
        for size in (1, 63, 64, 65, R.N_RAYS - 193):
            s = slice(start, start + size)
            assert np.array_equal(r.occluded(O[s], D[s], T[s]), want[s]), \
                f"call of {size} rays at {start}"
            start += size
        assert start == R.N_RAYS


def test_early_exit_does_not_leak_between_lanes(oracle):
    """Waves of 64 rays in which one ray's answer differs from its 63 mates': a lane that stops
    early, or a wave that leaves the scan early, must not change another lane's answer."""
    O, D, C = R.ray_batch(oracle)
    sc = R.scene_of(oracle, "final")
    n = len(sc)
    inf = np.full(R.N_RAYS, np.inf, np.float32)
    # which spheres accept, per ray at T = +inf, from the reference: the ground alone, or the
    # hierarchy alone (guarded rays only, so the wave takes the culled scan)
    guarded = np.isin(C, list("ABCDE"))
    occ_all, cnt_all, _ = Q.occluded_ref(sc, O, D, inf)
    occ_ground, _, _ = Q.occluded_ref(sc[n - 1:], O, D, inf)
    occ_hier, cnt_hier, _ = Q.occluded_ref(sc[:n - 4], O, D, inf)
    ground = np.nonzero(guarded & occ_ground)[0]
    hier_only = np.nonzero(guarded & occ_hier & (cnt_hier == cnt_all))[0]
    free = np.nonzero(guarded & ~occ_all)[0]
    blocked = np.nonzero(guarded & occ_all)[0]
    assert len(ground) >= 63 and len(hier_only) >= 1 and len(free) >= 63 and len(blocked) >= 63
    waves = []
    for one, rest, at in ((hier_only[0], ground[:63], 17), (free[0], blocked[:63], 40),
                          (blocked[5], free[:63], 0), (hier_only[-1], free[:63], 63)):
        idx = np.insert(rest, at, one)
        assert len(idx) == 64
        waves.append(idx)
    with vc.Renderer(vc.RenderDesc(**FRAME), "final") as r:
        for k, idx in enumerate(waves):
            got, st = r.occluded(O[idx], D[idx], np.inf, stats=True)
            assert st["bound_tests"] > 0  # the culled scan, past the big list
            assert np.array_equal(got, occ_all[idx]), f"wave {k}: rays {idx[got != occ_all[idx]]}"
            assert got.sum() == (64, 63, 1, 1)[k]


def test_frames_undisturbed(oracle):
    O, D, _ = R.ray_batch(oracle)
    T = Q.reference(oracle, "final")["T"]
    desc = vc.RenderDesc(width=64, height=40, samples_per_pixel=8, max_depth=10, device=0,
                         progressive=True)
    out = {}
    for query in (False, True):
        with vc.Renderer(desc, "final") as r:
            r.draw_next_frame()
            first = r.stats()
            if query:
                r.occluded(O, D, T)
                after = r.stats()
                assert {k: v for k, v in after.items() if k != "debug"} == \
                    {k: v for k, v in first.items() if k != "debug"}
            r.draw_next_frame()
            out[query] = (r.read_framebuffer(), r.stats())
    assert np.array_equal(out[True][0].view(np.uint32), out[False][0].view(np.uint32))
    for key in ("segments", "accumulated_spp", "frames", "kernel"):
        assert out[True][1][key] == out[False][1][key], key


def test_device_path_bounds(oracle):
    torch = pytest.importorskip("torch")
    O, D, _ = R.ray_batch(oracle)
    T = Q.reference(oracle, "final")["T"]
    n, guard = R.N_RAYS, 64
    want, _ = final_answers(oracle)
    dev = torch.device("cuda", 0)
    with vc.Renderer(vc.RenderDesc(**FRAME), "final") as r:
        to, td = torch.from_numpy(O.copy()).to(dev), torch.from_numpy(D.copy()).to(dev)
        tt = torch.from_numpy(T.copy()).to(dev)
        tocc = r.occluded(to, td, tt)
        assert tocc.dtype == torch.bool and tuple(tocc.shape) == (n,) and tocc.device == to.device
        assert np.array_equal(tocc.cpu().numpy(), want)
        # the output with guard bytes of a sentinel pattern, through the C ABI itself (filled on
        # the host and copied: the test launches no torch kernel)
        lib = r._L()
        gocc = torch.from_numpy(np.full(n + guard, 0xA5, np.uint8)).to(dev)
        torch.cuda.synchronize(dev)
        st = N.vcrt_ray_stats()
        assert lib.vcrt_occlude_rays_device(to.data_ptr(), td.data_ptr(), tt.data_ptr(), n,
                                            gocc.data_ptr(), ctypes.byref(st)) == 0
        g = gocc.cpu().numpy()
        assert np.array_equal(g[:n], want.view(np.uint8)) and np.all(g[n:] == 0xA5)
        assert st.kernel == b"vcrt_occlude_rays" and st.segments == n
        # an output that is not aligned: one byte into the buffer
        gocc = torch.from_numpy(np.full(n + guard, 0xA5, np.uint8)).to(dev)
        torch.cuda.synchronize(dev)
        assert lib.vcrt_occlude_rays_device(to.data_ptr(), td.data_ptr(), tt.data_ptr(), n,
                                            gocc.data_ptr() + 1, None) == 0
        g = gocc.cpu().numpy()
        assert g[0] == 0xA5 and np.array_equal(g[1:n + 1], want.view(np.uint8))
        assert np.all(g[n + 1:] == 0xA5)
        # count == 0 succeeds and writes nothing
        gocc = torch.from_numpy(np.full(guard, 0xA5, np.uint8)).to(dev)
        torch.cuda.synchronize(dev)
        assert lib.vcrt_occlude_rays_device(to.data_ptr(), td.data_ptr(), None, 0,
                                            gocc.data_ptr(), ctypes.byref(st)) == 0
        assert st.segments == 0 and np.all(gocc.cpu().numpy() == 0xA5)
        assert lib.vcrt_occlude_rays(None, None, None, 0, None, None) == 0
        e = r.occluded(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
        assert e.shape == (0,) and e.dtype == np.bool_
        e = r.occluded(to[:0], td[:0])
        assert tuple(e.shape) == (0,) and e.dtype == torch.bool
        # the error table
        p = (to.data_ptr(), td.data_ptr(), tt.data_ptr())
        f = lib.vcrt_occlude_rays_device
        assert f(None, p[1], p[2], 4, gocc.data_ptr(), None) == -3
        assert f(p[0], None, p[2], 4, gocc.data_ptr(), None) == -3
        assert f(p[0], p[1], p[2], 4, None, None) == -3
        assert f(p[0], p[1], p[2], (1 << 30) + 1, gocc.data_ptr(), None) == -11
        out = np.full(4, 0xA5, np.uint8)
        assert lib.vcrt_occlude_rays(O.ctypes.data, D.ctypes.data, None, (1 << 30) + 1,
                                     out.ctypes.data, None) == -11
        assert lib.vcrt_occlude_rays(O.ctypes.data, D.ctypes.data, None, 4, None, None) == -3
        assert np.all(out == 0xA5) and np.all(gocc.cpu().numpy() == 0xA5)


def test_description_independence(oracle):
    O, D, _ = R.ray_batch(oracle)
    T = Q.reference(oracle, "final")["T"]
    want, _ = final_answers(oracle)
    for extra in (dict(world_size=8, rank=3), dict(kernel_variant=vc.KERNEL_LDS),
                  dict(kernel_variant=vc.KERNEL_CULL_FLAT)):
        with vc.Renderer(vc.RenderDesc(**FRAME, **extra), "final") as r:
            assert np.array_equal(r.occluded(O, D, T), want), extra


def test_visible(oracle):
    rng = np.random.default_rng(5)
    n = 257
    a = np.stack([rng.uniform(-11, 11, n), rng.uniform(0.05, 3.0, n),
                  rng.uniform(-11, 11, n)], axis=1).astype(np.float32)
    b = np.stack([rng.uniform(-11, 11, n), rng.uniform(0.05, 3.0, n),
                  rng.uniform(-11, 11, n)], axis=1).astype(np.float32)
    sc = R.scene_of(oracle, "final")
    d = b - a
    assert d.dtype == np.float32
    want, _, _ = Q.occluded_ref(sc, a, d, np.ones(n, np.float32))
    with vc.Renderer(vc.RenderDesc(**FRAME), "final") as r:
        vis = r.visible(a, b)
        occ = r.occluded(a, d, 1.0)
    assert vis.dtype == np.bool_ and np.array_equal(vis, ~occ)
    assert np.array_equal(occ, want)
    assert 20 <= want.sum() <= n - 20  # both answers occur
