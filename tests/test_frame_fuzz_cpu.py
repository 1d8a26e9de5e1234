"""The frame-pass fuzz's inputs (tests/frame_fuzz_ref.py) do what tests/test_gpu_frame_fuzz.py
relies on: every case shows enough of its scene, and over the set the camera-ray lists take every
shape the list loop has (counts 0, 1, odd, 14, tiles that mix listed and unlisted quarters, a
frame of empty lists), scenes without tables and unbounded scenes occur, the normal's divs
fallback is needed, the motion pass rejects, projects and keeps pixels in one frame, and the
ambient pass finds blocked and open rays. Everything here is computed from the references and
the host builders; nothing reads a value of the GPU path."""
import numpy as np
import pytest

from tests import frame_fuzz_ref as FF
from tests import reproject_ref as P

F = np.float32
PIXELS = FF.W * FF.H

# Frames that are covered by design: hit share above 0.95, each with its reason.
COVERED = {
    **{f"fuzz-inside-{s}": "the eye is in the middle of a glass sphere" for s in (5, 17)},
    **{f"fuzz-big-{s}": "the camera looks into a cluster of 1500 spheres on its ground"
       for s in (0, 2, 3, 4)},
    "shape-big9": "the eight spheres of the ring (radius 25 to 40) stand behind the field",
    "edge-nan-centre": "every ray hits the NaN sphere in the reference's arithmetic",
    "fuzz-grid-8": "make_case's camera (13, 2, 3) looks down on the grid's ground, no sky in view",
    "fuzz-scaled-4": "make_case's camera at 3 s above the ground, vfov 9: no sky in view",
}
# Cases whose references hold NaN.
NAN_CASES = ("edge-nan-centre",)


@pytest.fixture(scope="module")
def table(oracle):
    """Per case: the frame, its references, routes, fallback counts and first-sample hits."""
    out = {}
    for name in FF.CASE_NAMES:
        f = FF.frame(name, oracle)
        _, _, _, s, _ = FF.sample_hits(oracle, f)
        out[name] = dict(f=f, ref=FF.reference(oracle, f), routes=FF.routes(oracle, f),
                         fallback=FF.fallback(oracle, f),
                         first=s.reshape(PIXELS, f["n"])[:, 0])
    return out


def test_the_seeded_parameters_take_every_value(table):
    fs = [t["f"] for t in table.values()]
    assert {f["n"] for f in fs} == set(FF.SAMPLES) and {f["first"] for f in fs} == set(FF.FIRSTS)
    assert {f["m"] for f in fs} == set(FF.SECONDARY)
    assert {f["reach_kind"] for f in fs} == set(FF.REACH_KINDS)
    assert {f["reach"] for f in fs if f["reach_kind"] == "min_t"} == {FF.MIN_T, 0.0}
    assert {f["prev"] for f in fs} == set(FF.PREV_KINDS)
    assert [f["lens"] for f in fs] == [FF.LENS_RADIUS if i % 4 == 3 else 0.0
                                       for i in range(len(fs))]
    assert all(len(f["scene"]) <= 1500 for f in fs)
    # every previous state occurs on a pinhole renderer (the lists exist)
    assert {f["prev"] for f in fs if f["lens"] == 0} == set(FF.PREV_KINDS)
    for name in list(FF.CAMERA) + list(FF.PREVIOUS) + list(FF.THROUGH_AT) + list(FF.REACH):
        assert name in FF.CASE_NAMES, name
    for name in FF.THROUGH_AT:
        assert table[name]["f"]["prev"] == "through", name


@pytest.mark.parametrize("name", FF.CASE_NAMES)
def test_a_case_shows_its_scene(table, name):
    t = table[name]
    first = t["first"]
    share = float((first >= 0).mean())
    distinct = len(np.unique(first[first >= 0]))
    print(name, "hit share", share, "distinct first-hit spheres", distinct)
    assert share >= 0.10
    assert (share > 0.95) == (name in COVERED), share
    if name != "edge-nan-centre":
        assert distinct >= 3


@pytest.mark.parametrize("name", FF.CASE_NAMES)
def test_nan_only_where_listed(table, name):
    ref = table[name]["ref"]
    planes = dict(albedo=ref["features"]["albedo"], normal_depth=ref["features"]["normal_depth"],
                  visibility=ref["ambient"]["visibility"], motion=ref["motion"]["motion"],
                  surface=ref["motion"]["surface"])
    nan = {k: int(np.isnan(v).sum()) for k, v in planes.items()}
    print(name, nan)
    if name in NAN_CASES:
        assert any(nan.values())
    else:
        assert not any(nan.values())
        # (the bound on what the both-NaN rule may excuse)
        assert all(n <= 0.02 * planes[k].size for k, n in nan.items())


def test_the_routes_over_the_set(table):
    r = {name: t["routes"] for name, t in table.items()}
    with_lists = [n for n, x in r.items() if x["words"] is not None and x["listed"] > 0]
    no_tables = [n for n, x in r.items() if not x["tables"]]
    unbounded = [n for n, x in r.items() if not x["bounded"]]
    mixed = [n for n, x in r.items() if x["mixed_tiles"] > 0]
    empty = [n for n, x in r.items() if x["listed"] > 0 and not x["counts"].any()]
    print("lists", len(with_lists), "no tables", no_tables, "unbounded", unbounded,
          "mixed tiles", len(mixed), "all lists empty", empty)
    assert len(with_lists) >= 40
    assert len(no_tables) >= 3 and len(unbounded) >= 2
    assert all(not r[n]["tables"] for n in unbounded)       # an unbounded scene has no tables
    assert all(r[n]["words"] is None for n in no_tables)
    counts = np.unique(np.concatenate([x["counts"] for x in r.values()]))
    assert counts.min() == 0 and counts.max() == 14
    assert 1 in counts and any(c >= 3 and c % 2 == 1 for c in counts)
    assert len(mixed) >= 5
    assert len(empty) >= 1
    # the pinhole cases among them: a lens renderer has no lists
    pin = [n for n in with_lists if table[n]["f"]["lens"] == 0]
    assert len(pin) >= 30 and any(n in pin for n in mixed) and any(n in pin for n in empty)
    # every ray of every frame is inside guard_a's range: listed_rays equals the prediction
    for n, x in r.items():
        assert x["guarded_pairs"] == x["pairs"] and x["guarded_centre"] == x["pairs_centre"], n
        assert 0 <= x["pairs_centre"] <= PIXELS and x["pairs"] == x["pairs_centre"] * \
            table[n]["f"]["n"]


def test_the_divs_fallback_is_needed(table):
    needs = [n for n, t in table.items()
             if not t["fallback"]["radii_safe"] or t["fallback"]["samples"] > 0
             or t["fallback"]["centre"] > 0]
    print("divs fallback", needs)
    assert len(needs) >= 2
    # off the identity route, where the motion pass computes the normal
    assert sum(table[n]["f"]["prev"] != "same" for n in needs) >= 2


def test_motion_rejects_keeps_and_projects(oracle, table):
    seen_changed = []
    for name, t in table.items():
        f, mo = t["f"], t["ref"]["motion"]
        rejected = 1.0 - mo["projected"] / PIXELS
        if f["prev"] == "through":
            print(name, "rejected", rejected)
            assert 0.05 <= rejected <= 0.95, (name, rejected)
        if f["prev"] == "moved-only":
            print(name, "identity", mo["identity"], "projected", mo["projected"])
            assert 0 < mo["identity"] < mo["projected"], name
        if f["prev"] == "same":
            assert mo["identity"] == PIXELS == mo["projected"], name
        if f["prev"] in ("orbit", "orbit-moved", "through"):
            assert mo["identity"] == 0, name
        _, prev_scene, changed = FF.previous(oracle, f)
        if changed >= 0:
            # the radius alone differs: three equal words, the fourth decides
            assert np.array_equal(prev_scene["center"][changed], f["scene"]["center"][changed])
            assert prev_scene["radius"][changed] != f["scene"]["radius"][changed]
            if f["prev"] == "orbit-moved" and (mo["sphere"] == changed).any():
                seen_changed.append(name)
    print("orbit-moved cases that see the changed radius", seen_changed)
    assert len(seen_changed) >= 1


def test_the_consumers_inputs(table):
    """reproject on the reference's planes of the through cases takes some history, not all."""
    for name, t in table.items():
        f, mo = t["f"], t["ref"]["motion"]
        if f["prev"] != "through":
            continue
        colour, hcol = FF.colour_planes()
        _, _, took = P.reproject(colour, mo["motion"], hcol, mo["surface"],
                                 np.full((FF.H, FF.W), 3, F), **P.DEFAULTS)
        print(name, "took", took.mean())
        assert 0 < took.mean() < 1, name


def test_ambient_blocks_some_and_not_all(table):
    between = []
    for name, t in table.items():
        f, am = t["f"], t["ref"]["ambient"]
        assert am["secondary_rays"] == am["hit_rays"] * f["m"] > 0, name
        assert int(am["blocked"].sum()) == am["occluded"], name
        if f["reach"] <= FF.MIN_T:
            assert am["occluded"] == 0, name
        if 0 < am["occluded"] < am["secondary_rays"]:
            between.append(name)
    print("blocked strictly between 0 and all:", len(between))
    assert len(between) >= 30
