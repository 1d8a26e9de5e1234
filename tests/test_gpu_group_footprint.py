"""GPU parity of the group-level footprint (tracer.hip fact (5g), TraceParams.gf_tab): on eligible
scenes the LDS-table flat kernel takes each ray's groups from four table lookups and pushes them
straight onto the group stack, with no node level and no box test. Only the issued tests may
change: every case is bit-identical to the CPU oracle with equal segment counts, through the
LDS-table kernel and its cost-order build -- the final scene, a one-height scene, a one-height grid
of exactly 128 groups (no box test at all) and its twin of 129 (the node level as before), and a
grid of 80 groups too small for the tables (every lane pushes every group: the sliced push). Each
eligible case runs again with VCRT_GROUP_FOOT=0: the same bits and segments from the node level,
which issues box tests and no more group tests than the tables do.
"""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import group_footprint_ref as G
from tests.test_gpu_slab import CUSTOM_CAM, one_height_scene

pytestmark = pytest.mark.gpu

#        scene, w, h, spp, depth, camera, eligible
CASES = {
    "final": ("final", 96, 54, 4, 10, {}, True),
    "one_height": (one_height_scene, 64, 36, 8, 8, CUSTOM_CAM, True),
    "grid128": (G.grid128, 64, 36, 2, 8, G.GRID_CAM, True),
    "grid129": (G.grid129, 64, 36, 2, 8, G.GRID_CAM, False),
    # coordinates below the tables' bound: all-ones masks, 64 lanes x 80 groups: the sliced push
    "sliced": (G.tiny_grid, 64, 36, 2, 6, G.TINY_CAM, True),
}

_want = {}


def reference(oracle, case, st):
    key = (case, st["accumulate_quantum"])
    if key not in _want:
        scene, w, h, spp, depth, cam, _ = CASES[case]
        sc = oracle.scene(scene) if isinstance(scene, str) else scene()
        cfg = oracle.config(w, h, spp, depth, **oracle.partition(st), **cam)
        _want[key] = oracle.render(cfg, sc)
    return _want[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render(oracle, case, cost, what):
    """The case through the LDS-table kernel, checked against the oracle; the last frame's stats."""
    scene, w, h, spp, depth, cam, _ = CASES[case]
    sc = scene if isinstance(scene, str) else scene()
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=vc.KERNEL_CULL_FLAT, **cam)
    with vc.Renderer(desc, sc) as r:
        for frame in range(2 if cost else 1):  # cost order: the measuring frame, then the order
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
            want, segs = reference(oracle, case, st)
            assert st["kernel"] == "vcrt_trace_cull_flat" + ("_cost" if cost else ""), what
            assert np.array_equal(bits(got), bits(want)), f"{what} frame {frame}"
            assert st["segments"] == segs, f"{what} frame {frame}"
    return st


@pytest.mark.parametrize("cost", [False, True], ids=["plain", "cost"])
@pytest.mark.parametrize("case", list(CASES))
def test_group_footprint_bitwise(oracle, monkeypatch, case, cost):
    eligible = CASES[case][6]
    if cost:
        monkeypatch.setenv("VCRT_WORK_ORDER", "cost")
    monkeypatch.delenv("VCRT_GROUP_FOOT", raising=False)
    on = render(oracle, case, cost, f"{case} cost={cost} tables on")
    print(f"{case} cost={cost}: bound_tests {on['bound_tests']} group_tests {on['group_tests']} "
          f"segments {on['segments']}")
    if not eligible:
        assert on["bound_tests"] > 0  # the node level, as before
        return
    assert on["bound_tests"] == 0  # no box test on this path
    monkeypatch.setenv("VCRT_GROUP_FOOT", "0")
    off = render(oracle, case, cost, f"{case} cost={cost} VCRT_GROUP_FOOT=0")
    print(f"{case} cost={cost} VCRT_GROUP_FOOT=0: bound_tests {off['bound_tests']} group_tests "
          f"{off['group_tests']}")
    assert off["bound_tests"] > 0
    assert off["group_tests"] <= on["group_tests"]
    assert off["lds_bytes"] == on["lds_bytes"] and off["ring_entries"] == on["ring_entries"]
