"""The adaptive-sampling fuzz's inputs (tests/adaptive_fuzz_ref.py) do what
tests/test_gpu_adaptive_fuzz.py relies on: every count plane has idle pixels and a whole idle
tile, clamped words, partial quanta, pixels of several quanta and an item count that leaves the
last wave short; over the set every depth, max_count and first index meets the camera-ray lists,
depth 1 meets them often, scenes without tables and a frame of empty lists occur; NaN sums occur
only where named; paths both end early and bounce; the variance chain's reference takes both
branches of the variance and spreads the counts. Everything here is computed from the references
and the host builders; nothing reads a value of the GPU path."""
import numpy as np
import pytest

from tests import adaptive_fuzz_ref as AF
from tests import adaptive_ref as AR
from tests import frame_fuzz_ref as FF

F = np.float32
PIXELS = AF.W * AF.H

# Cases whose reference sums hold NaN, each with its reason: none. Every case is compared purely
# bit for bit on the GPU. The two candidates of the other fuzz files:
#   edge-nan-centre   every segment "hits" the NaN sphere, a diffuse one, so no path reaches the
#                     sky: ray_color returns 0 at any depth, and the sums are +0;
#   edge-zero-radius  a sphere of radius 0 has a discriminant >= 0 only for a ray through its
#                     centre, and no ray of the two rounds is one: its 0 / 0 normal is never made.
NAN_CASES = {}


@pytest.fixture(scope="module")
def table(oracle):
    out = {}
    for name in AF.CASE_NAMES:
        c = AF.case(name, oracle)
        out[name] = dict(c=c, ref=AF.reference(oracle, c), routes=FF.routes(oracle, c))
    return out


def with_lists(t):
    """A pinhole case that has camera-ray lists."""
    return t["c"]["lens"] == 0 and t["routes"]["words"] is not None and t["routes"]["listed"] > 0


@pytest.mark.parametrize("name", AF.CASE_NAMES)
def test_a_case_has_every_kind_of_pixel(table, name):
    c, (one, two) = table[name]["c"], table[name]["ref"]
    m = c["max_count"]
    most = min(5, (m + AR.Q - 1) // AR.Q)  # 5 quanta, or all that max_count admits (2 of 5, 3 of 9)
    for k, plane in enumerate(c["planes"]):
        n = AR.clamp_counts(plane, m)
        q = AF.quanta(plane, m)
        zero, clamped = float((plane == 0).mean()), int((plane > m).sum())
        print(name, f"plane {k} depth {c['depth']} max_count {m} first {c['start']}",
              f"zero {zero:.3f} clamped {clamped} quanta max {q.max()} items {q.sum()}",
              f"samples {n.sum()} heavy on hits {int((c['hits'] & (plane == m)).sum())}")
        assert plane.shape == (AF.H, AF.W) and plane.dtype == np.uint16
        assert zero >= 0.05
        assert clamped >= 1 and (plane == 65535).any()
        assert {1, 2, 3} <= set((n % 4).ravel().tolist())
        assert q.max() >= most
        assert int(q.sum()) % 64 != 0
        # a whole tile of zeros beside a tile without one
        ty_n, tx_n = AF.H // 8, AF.W // 8   # the full tiles
        t0 = np.array([[not plane[8 * y:8 * y + 8, 8 * x:8 * x + 8].any() for x in range(tx_n + 1)]
                       for y in range(ty_n)])
        t1 = np.array([[plane[8 * y:8 * y + 8, 8 * x:8 * x + 8].all() for x in range(tx_n + 1)]
                       for y in range(ty_n)])
        assert (t0[:, :-1] & t1[:, 1:]).any()
        if c["hits"].any():
            assert (c["hits"] & (plane == m)).any()
    assert c["start"] + 2 * m <= AF.LIMIT
    idle = c["planes"][1] == 0
    same = (one[0].view(np.uint32) == two[0].view(np.uint32)).all(axis=-1)
    assert idle.any() and same[idle].all() and not same[~idle].all()
    never = idle & (c["planes"][0] == 0)
    assert (two[1][never] == F([0, 0, 0, 1])).all()
    assert one[2]["items"] == int(AF.quanta(c["planes"][0], m).sum())


def test_the_parameters_over_the_set(table):
    every = dict(depth=set(AF.DEPTHS), max_count=set(AF.MAX_COUNTS), first_kind=set(AF.FIRST_KINDS))
    cs = [t["c"] for t in table.values()]
    listed = [t["c"] for t in table.values() if with_lists(t)]
    for k, want in every.items():
        assert {c[k] for c in cs} == want, k
        assert {c[k] for c in listed} == want, k
    assert any(AF.quanta(c["planes"][0], c["max_count"]).max() >= 5 for c in listed)
    deep1 = [c["name"] for c in listed if c["depth"] == 1]
    no_tables = [n for n, t in table.items() if not t["routes"]["tables"]]
    empty = [n for n, t in table.items()
             if t["routes"]["listed"] > 0 and not t["routes"]["counts"].any()]
    print("pinhole with lists", len(listed), "of them depth 1", deep1, "no tables", no_tables,
          "all lists empty", empty)
    assert len(deep1) >= 3 and len(no_tables) >= 3 and len(empty) >= 1
    for name in list(AF.DEPTH) + list(AF.MAX_COUNT) + list(AF.FIRST) + list(AF.TARGET) + \
            list(AF.CHAIN_PREV) + list(NAN_CASES):
        assert name in AF.CASE_NAMES, name
    for name in AF.CHAIN_PREV:
        assert table[name]["c"]["prev"] == "through", name
    from tests.test_frame_fuzz_cpu import NAN_CASES as frame_nan
    assert AF.FRAME_NAN_CASES == frame_nan
    assert [c["lens"] for c in cs] == [FF.LENS_RADIUS if i % 4 == 3 else 0.0
                                       for i in range(len(cs))]
    # the prediction of listed_rays is exact: every camera ray is inside guard_a's range
    for n, t in table.items():
        assert t["routes"]["guarded_pairs"] == t["routes"]["pairs"], n


@pytest.mark.parametrize("name", AF.CASE_NAMES)
def test_nan_only_where_named(table, name):
    one, two = table[name]["ref"]
    nan = [int(np.isnan(r[k]).sum()) for r in (one, two) for k in (0, 1)]
    print(name, "NaN words in sums / mean of round one, two:", nan)
    if name in NAN_CASES:
        assert NAN_CASES[name] and all(nan)
    else:
        assert not any(nan)


@pytest.mark.parametrize("name", AF.CASE_NAMES)
def test_paths_end_early_and_bounce(table, name):
    c = table[name]["c"]
    for st in (r[2] for r in table[name]["ref"]):
        print(name, "depth", c["depth"], "samples", st["samples"], "segments", st["segments"])
        if c["depth"] == 1:
            assert st["segments"] == st["samples"]
        elif name not in NAN_CASES:
            assert st["samples"] < st["segments"] < st["samples"] * c["depth"]


def test_the_chain_takes_both_branches(oracle, table):
    ran = 0
    for name, t in table.items():
        c = t["c"]
        if not AF.in_chain(c, NAN_CASES):
            continue
        ch = AF.reference_chain(oracle, c)
        spatial, values = float(ch["spatial"].mean()), np.unique(ch["counts"])
        print(name, f"prev {AF.chain_prev(c)} target {ch['target']:.5f} spatial {spatial:.3f}",
              f"accepted {ch['accepted'].mean():.3f} counts {values.tolist()} total {ch['total']}")
        assert all(np.isfinite(ch[k]).all() for k in ("mean", "out", "moments", "variance")), name
        assert 0.05 <= spatial <= 0.95, name
        assert len(values) >= 4 and 0 < ch["total"] < AF.CHAIN_MOST * PIXELS, name
        ran += 1
    assert ran >= 10
