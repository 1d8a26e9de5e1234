"""The ray and occlusion queries on generated scenes (GPU): vcrt_trace_rays and vcrt_occlude_rays
bit for bit against the references, on every case of tests/query_fuzz_ref.py with a ray batch
built from the case's own geometry -- hierarchies of 16 to 384 groups (last chunks of 2, 4 and 6
nodes, odd chunk counts, exactly 64 and 128 groups), big lists of 0 to 3 groups (full and partly
filled), duplicate, nested and hollow spheres, scenes scaled by 10^-2 to 10^3, flat boxes, scenes
without tables, unbounded scenes and radii outside the safe range. Each batch runs in class
order (the waves of guarded rays take the culled scan) and under one permutation (nearly every
wave holds an unguarded ray and takes the linear scan): a ray's result depends on neither.
tests/test_query_fuzz_cpu.py holds the conditions on the inputs that make a pass mean something.
"""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import query_fuzz_ref as F
from tests.test_gpu_ray_query import bits

pytestmark = pytest.mark.gpu

DEPTH = F.DEPTH


def same_or_nan_where_the_reference_is(got, want, fin, what):
    """Bitwise equal on the contract's rays; where the reference's own value is NaN (a NaN
    centre, a zero radius) the result must be NaN too (the rule of
    test_gpu_fuzz._same_bits_or_both_nan)."""
    got = np.ascontiguousarray(got, np.float32).reshape(len(fin), -1)
    want = np.ascontiguousarray(want, np.float32).reshape(len(fin), -1)
    both_nan = np.isnan(got) & np.isnan(want)
    bad = np.nonzero(((bits(got) != bits(want)) & ~both_nan).any(axis=1) & fin)[0]
    assert bad.size == 0, f"{what}: rays {bad[:8]} of {bad.size} differ: " \
                          f"{got[bad[:3]]} for {want[bad[:3]]}"


def check_trace(rad, hits, st, ref, sel, what):
    """test_gpu_ray_query.check_parity with the NaN rule, and the batch's statistics."""
    fin = ref["finite"][sel]
    assert rad.shape == (F.N_RAYS, 4) and hits.shape == (F.N_RAYS,), what
    assert np.all(bits(rad[:, 3]) == 0x3F800000), what
    assert np.all(hits["reserved"] == 0) and np.all(bits(hits["reserved2"]) == 0), what
    same_or_nan_where_the_reference_is(rad[:, :3], ref["rgb"][sel], fin, what + " rgb")
    bad = np.nonzero((hits["segments"] != ref["segs"][sel].astype(np.uint32)) & fin)[0]
    assert bad.size == 0, f"{what}: segments of rays {bad[:8]} of {bad.size}"
    bad = np.nonzero((hits["sphere"] != ref["sphere"][sel]) & fin)[0]
    assert bad.size == 0, f"{what}: sphere of rays {bad[:8]} of {bad.size}: " \
                          f"{hits['sphere'][bad[:8]]} for {ref['sphere'][sel][bad[:8]]}"
    same_or_nan_where_the_reference_is(hits["t"], ref["t"][sel], fin, what + " t")
    same_or_nan_where_the_reference_is(hits["normal"], ref["normal"][sel], fin, what + " normal")
    # the other rays (class H): traced without a fault, at most max_depth scans each
    other = hits["segments"][~fin]
    assert np.all((other >= 1) & (other <= DEPTH)), what
    assert st["segments"] == int(ref["segs"][sel][fin].sum()) + int(other.sum()), what
    assert st["kernel"] == "vcrt_trace_rays" and st["group_tests"] > 0, what


def check_occlusion(occ, st, want, fin, what):
    assert occ.dtype == np.bool_ and occ.shape == (F.N_RAYS,), what
    assert np.all(occ.view(np.uint8) <= 1), what  # the other rays too: 0 or 1
    bad = np.nonzero((occ != want) & fin)[0]
    assert bad.size == 0, f"{what}: rays {bad[:8]} of {bad.size} differ"
    assert st["kernel"] == "vcrt_occlude_rays" and st["segments"] == F.N_RAYS, what
    assert st["group_tests"] > 0, what


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_queries_bitwise(oracle, monkeypatch, name):
    c = F.case(name, oracle)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    O, D, _ = F.rays(c)
    ref = F.reference(oracle, c)
    fin = ref["finite"]
    T = ref["T"]
    culled = F.bounded(c["scene"]) and F.tables_of(c) is not None
    perm = np.random.default_rng(7).permutation(F.N_RAYS)
    desc = vc.RenderDesc(width=16, height=16, samples_per_pixel=1, max_depth=DEPTH, device=0,
                         **c["cam"])
    with vc.Renderer(desc, c["scene"]) as r:
        for order, sel in (("class order", slice(None)), ("permuted", perm)):
            what = f"{name}, {order}"
            rad, hits, st = r.trace_rays(O[sel], D[sel], DEPTH, hits=True, stats=True)
            check_trace(rad, hits, st, ref, sel, what)
            occ, ost = r.occluded(O[sel], D[sel], T[sel], stats=True)
            check_occlusion(occ, ost, ref["occ"][sel], fin[sel], what)
            if order == "class order":
                # the waves of classes A..E are guarded whole: the culled scan, where it applies
                assert (st["bound_tests"] > 0) == culled and (ost["bound_tests"] > 0) == culled
                first_sphere = hits["sphere"]
        # the default reach: "trace_rays finds a first hit"
        occ, ost = r.occluded(O, D, stats=True)
        check_occlusion(occ, ost, ref["occ_default"], fin, f"{name}, default reach")
        assert np.array_equal(occ[fin], (first_sphere >= 0)[fin])
