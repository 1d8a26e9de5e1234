"""The frame passes on generated scenes (GPU): vcrt_draw_features, vcrt_draw_occlusion and
vcrt_draw_motion bit for bit against tests/features_ref.py, tests/ambient_ref.py and
tests/motion_ref.py on every case of tests/frame_fuzz_ref.py -- the 59 scenes of the query fuzz as
44 x 20 frames with seeded sample ranges, secondary rays, reaches, lens radii and previous states
of the motion pass. Per case: parity of every plane and count; the route each pass's rays took
(camera-ray lists, culled scan, linear scan) against what the host builders predict; the same
bits without the lists (VCRT_FEATURE_LISTS=0); the feature kernel's own first hit and
frame_first_hit's against vcrt_trace_rays on the same rays; where spheres moved, the motion pass
again from the caller's 40-byte records on the device; on every fifth case a shard's packed
tiles; on the orbit and through cases the consumers, reproject and denoise, on the GPU planes.
tests/test_frame_fuzz_cpu.py holds the conditions on the inputs that make a pass mean something.
"""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import denoise_ref as D
from tests import features_ref as FR
from tests import frame_fuzz_ref as FF
from tests import motion_ref as M
from tests import reproject_ref as P
from tests.test_gpu_ambient import SENTINEL as A_FILL, draw_packed as occlusion_packed
from tests.test_gpu_features import SENTINEL as F_FILL, draw_packed as features_packed
from tests.test_gpu_fuzz import _same_bits_or_both_nan
from tests.test_gpu_motion import SENTINEL as M_FILL, draw_packed as motion_packed

pytestmark = pytest.mark.gpu

F = np.float32
W, H = FF.W, FF.H
F_PLANES = ("albedo", "normal_depth")
M_PLANES = ("motion", "surface")


def same(got, want, what):
    """Bitwise equal, or both NaN (the reference's NaN pixels: test_frame_fuzz_cpu pins where)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    _same_bits_or_both_nan(got.reshape(len(got), -1), want.reshape(len(want), -1), what)


def draw_all(r, f, prev_desc, prev_scene):
    feat = r.draw_features(samples=f["n"], first=f["first"], stats=True)
    occ, occ_st = r.draw_occlusion(samples=f["n"], first=f["first"], rays=f["m"],
                                   reach=f["reach"], stats=True)
    mot = r.draw_motion(prev_camera=prev_desc, prev_spheres=prev_scene, stats=True)
    return feat, occ, occ_st, mot


def check_routes(name, f, rt, feat_st, occ_st, mot_st):
    """The stats' route counts against the host builders' prediction."""
    lens = f["lens"] > 0
    lists = rt["words"] is not None and not lens
    assert lists == (rt["tables"] and rt["bounded"] and not lens)
    scans = rt["tables"] and (rt["unlisted"] > 0 or lens)  # some ray takes the culled scan
    for what, st, pairs, guarded in (("features", feat_st, rt["pairs"], rt["guarded_pairs"]),
                                     ("occlusion", occ_st, rt["pairs"], rt["guarded_pairs"]),
                                     ("motion", mot_st, rt["pairs_centre"], rt["guarded_centre"])):
        listed = st["listed_rays"]
        if not lists or pairs == 0:
            assert listed == 0, (name, what, listed)
        elif guarded == pairs:
            assert listed == pairs, (name, what, listed, pairs)
        else:
            assert 0 < listed <= pairs, (name, what, listed, pairs)
        if not rt["tables"]:
            assert st["bound_tests"] == 0, (name, what)
        elif what == "occlusion":   # (its secondary rays take the culled scan too)
            assert st["bound_tests"] > 0 or not scans, (name, what)
        else:
            assert (st["bound_tests"] > 0) == scans, (name, what, st["bound_tests"])
        assert st["group_tests"] > 0, (name, what)


@pytest.mark.parametrize("name", FF.CASE_NAMES)
def test_frame_passes_bitwise(oracle, monkeypatch, name):
    f = FF.frame(name, oracle)
    for k, v in f["env"].items():
        monkeypatch.setenv(k, v)
    sc, desc, n, first, m = f["scene"], f["desc"], f["n"], f["first"], f["m"]
    ref = FF.reference(oracle, f)
    rt = FF.routes(oracle, f)
    prev_desc, prev_scene, _ = FF.previous(oracle, f)
    want_f, want_o, want_m = ref["features"], ref["ambient"], ref["motion"]
    pin = FF.pinhole(f)
    y, x = np.mgrid[0:H, 0:W]
    o1, d1 = vc.frame_rays(desc, np.stack([x.ravel(), y.ravel()], axis=1), first, 1)
    oc, dc = M.centre_rays(oracle, pin)
    Dc = np.ascontiguousarray(dc.reshape(-1, 3))
    Oc = np.ascontiguousarray(np.broadcast_to(oc, Dc.shape))
    consumers = f["prev"] in ("orbit", "through") and name != "edge-nan-centre"

    with vc.Renderer(desc, sc) as r:
        feat, occ, occ_st, mot = draw_all(r, f, prev_desc, prev_scene)
        one = r.draw_features(samples=1, first=first) if f["lens"] == 0 else None
        _, hits1 = r.trace_rays(o1[:, 0], d1[:, 0], max_depth=1, hits=True)
        _, hitsc = r.trace_rays(Oc, Dc, max_depth=1, hits=True)
        mot_rec = None
        if prev_scene is not None:
            # the caller's own 40-byte records on the device: the form with a stride of 10
            import torch
            rec = torch.from_numpy(
                np.ascontiguousarray(prev_scene).view(F).reshape(-1, 10).copy()).cuda()
            mot_rec = r.draw_motion(prev_camera=prev_desc, prev_spheres=rec, stats=True)
            mot_rec = {k: (v if k == "stats" else v.cpu().numpy()) for k, v in mot_rec.items()}
        if consumers:
            r.draw_next_frame()
            frame = r.read_framebuffer()
            hist = dict(colour=FF.colour_planes()[1], surface=mot["surface"],
                        length=np.full((H, W), 3, F))
            rep, hist2 = r.reproject(frame, mot["motion"], hist, surface=mot["surface"])
            den = r.denoise(frame, dict(albedo=feat["albedo"],
                                        normal_depth=feat["normal_depth"]))
    feat_st, mot_st = feat.pop("stats"), mot.pop("stats")
    print(name, f"n{n} first{first} m{m} reach {f['reach']} lens {f['lens']} prev {f['prev']}",
          "listed f/o/m", feat_st["listed_rays"], occ_st["listed_rays"], mot_st["listed_rays"],
          "of", rt["pairs"], rt["pairs"], rt["pairs_centre"],
          "bound f/o/m", feat_st["bound_tests"], occ_st["bound_tests"], mot_st["bound_tests"],
          "tables", rt["tables"], "bounded", rt["bounded"], "quarters listed/unlisted",
          rt["listed"], rt["unlisted"], "mixed tiles", rt["mixed_tiles"])

    # ---- the three passes against their references ----
    assert np.array_equal(feat["sphere"], want_f["sphere"]), name
    for k in F_PLANES:
        same(feat[k], want_f[k], f"{name} {k}")
    assert feat_st["rays"] == W * H * n and feat_st["kernel"] == "vcrt_frame_features"
    same(occ, want_o["visibility"], f"{name} visibility")
    assert occ_st["rays"] == W * H * n and occ_st["kernel"] == "vcrt_frame_occlusion"
    assert occ_st["hit_rays"] == want_o["hit_rays"], name
    assert occ_st["secondary_rays"] == want_o["secondary_rays"], name
    assert occ_st["occluded"] == want_o["occluded"], name
    for k in M_PLANES:
        same(mot[k], want_m[k], f"{name} {k}")
    assert mot_st["rays"] == W * H and mot_st["kernel"] == "vcrt_frame_motion"
    assert mot_st["hit_rays"] == want_m["hit"], name
    assert mot_st["projected"] == want_m["projected"], name
    assert mot_st["identity"] == want_m["identity"], name
    if mot_rec is not None:
        for k in M_PLANES:
            same(mot_rec[k], want_m[k], f"{name} {k} from device records")
        assert all(mot_rec["stats"][k] == mot_st[k]
                   for k in ("rays", "hit_rays", "projected", "identity", "listed_rays")), name

    # ---- the routes ----
    check_routes(name, f, rt, feat_st, occ_st, mot_st)

    # ---- the two copies of the first hit, against the ray queries ----
    if one is not None:
        hit = hits1["sphere"] >= 0
        assert np.array_equal(one["sphere"].ravel(), hits1["sphere"]), name
        t = np.where(hit, hits1["t"], F(0))
        nrm = np.where(hit[:, None], hits1["normal"], F(0)).astype(F)
        same(one["normal_depth"].reshape(-1, 4), np.concatenate([nrm, t[:, None]], axis=1),
             f"{name} features against trace_rays")
    assert np.array_equal((mot["surface"][..., 0].ravel() - 2).astype(np.int32),
                          hitsc["sphere"]), name
    same(mot["surface"][..., 1].reshape(-1, 1),
         np.where(hitsc["sphere"] >= 0, hitsc["t"], F(0)).reshape(-1, 1),
         f"{name} motion against trace_rays")

    # ---- the same bits without the lists ----
    monkeypatch.setenv("VCRT_FEATURE_LISTS", "0")
    with vc.Renderer(desc, sc) as r:
        feat0, occ0, occ0_st, mot0 = draw_all(r, f, prev_desc, prev_scene)
    monkeypatch.delenv("VCRT_FEATURE_LISTS")
    assert np.array_equal(feat0["sphere"], feat["sphere"]), name
    for k in F_PLANES:
        same(feat0[k], feat[k], f"{name} {k} without lists")
    same(occ0, occ, f"{name} visibility without lists")
    for k in M_PLANES:
        same(mot0[k], mot[k], f"{name} {k} without lists")
    assert feat0["stats"]["listed_rays"] == occ0_st["listed_rays"] == 0, name
    assert mot0["stats"]["listed_rays"] == 0, name
    assert (occ0_st["hit_rays"], occ0_st["occluded"]) == (occ_st["hit_rays"], occ_st["occluded"])
    if rt["tables"]:
        assert feat0["stats"]["bound_tests"] > 0 and mot0["stats"]["bound_tests"] > 0, name

    # ---- rank 1 of 3: packed tiles, the slots outside the frame untouched ----
    if FF.CASE_NAMES.index(name) % 5 == 0:
        d3 = vc.RenderDesc(width=W, height=H, samples_per_pixel=4, max_depth=3, device=0,
                           lens_radius=f["lens"], world_size=3, rank=1, **f["cam"])
        with vc.Renderer(d3, sc) as r:
            f3, fst3 = features_packed(r, first, n)
            o3, ost3 = occlusion_packed(r, first, n, m, f["reach"])
            m3, mst3 = motion_packed(r, prev_desc, prev_scene)
        want3 = FR.packed(want_f["sphere"], W, H, 3, 1, F_FILL["sphere"])
        assert np.array_equal(f3["sphere"], want3), name
        valid = int((want3 != F_FILL["sphere"]).sum())
        assert 0 < valid < want3.size
        for k in F_PLANES:
            same(f3[k], FR.packed(want_f[k], W, H, 3, 1, F_FILL[k]), f"{name} {k} rank 1 of 3")
        same(o3, FR.packed(want_o["visibility"], W, H, 3, 1, A_FILL),
             f"{name} visibility rank 1 of 3")
        for k in M_PLANES:
            same(m3[k], FR.packed(want_m[k], W, H, 3, 1, M_FILL), f"{name} {k} rank 1 of 3")
        mine = vc.tile_pixel_map(W, H, 3)[..., 0] == 1
        assert fst3.rays == ost3.rays == valid * n and mst3.rays == valid
        assert ost3.hit_rays == want_o["C"][mine].sum(), name
        assert ost3.occluded == want_o["blocked"][mine].sum(), name
        assert mst3.hit_rays == int((want_m["sphere"][mine] >= 0).sum()), name

    # ---- the consumers on the GPU planes ----
    if consumers:
        for k, v in (("frame", frame), ("motion", mot["motion"]), ("surface", mot["surface"]),
                     ("albedo", feat["albedo"]), ("normal_depth", feat["normal_depth"])):
            assert np.isfinite(v).all(), (name, k)
        want_rep, want_len, took = P.reproject(frame, mot["motion"], hist["colour"],
                                               hist["surface"], hist["length"], **P.DEFAULTS)
        same(rep, want_rep, f"{name} reproject")
        same(hist2["length"], want_len, f"{name} reproject length")
        if f["prev"] == "through":
            assert 0 < took.mean() < 1, (name, took.mean())
        same(den, D.denoise(frame, feat["albedo"], feat["normal_depth"], **D.DEFAULTS),
             f"{name} denoise")
