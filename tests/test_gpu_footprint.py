"""GPU parity of the footprint tables (tracer.hip fact (5), TraceParams.fp_tab): the LDS-table
flat kernel forms each ray's node mask from four table lookups in place of the node box tests.
Only the issued tests may change: every case is bit-identical to the CPU oracle with equal
segment counts, through the LDS-table kernel and its cost-order build -- the final scene, a
camera inside its slab looking horizontally (d.y ~ 0), a one-height scene and its one-ulp twin
(no shared slab: the y interval comes from the overall extent), a tall scene, a scene of 176
groups (22 nodes: 32-bit masks), and a scene too small for the tables (all-ones masks: every lane
enters every node, the fullest the node stack gets).
"""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import footprint_ref as F
from tests.test_gpu_slab import CUSTOM_CAM, INSIDE_CAM, one_height_scene

pytestmark = pytest.mark.gpu

TALL_CAM = dict(lookfrom=(9, 5, 10), lookat=(0, 3, 0), vfov=45)
MANY_CAM = dict(lookfrom=(10, 3, 9), lookat=(0, 0.2, 0), vfov=45)

#        scene, w, h, spp, depth, camera
CASES = {
    "final": ("final", 96, 54, 4, 10, {}),
    "inside_slab": ("final", 32, 32, 4, 10, INSIDE_CAM),
    "one_height": (one_height_scene, 64, 36, 8, 8, CUSTOM_CAM),
    "one_height_ulp": (lambda: one_height_scene(True), 64, 36, 8, 8, CUSTOM_CAM),
    "tall": (F.tall_scene, 64, 36, 4, 8, TALL_CAM),
    "many_groups": (F.many_groups_scene, 64, 36, 2, 8, MANY_CAM),
    # coordinates below the tables' bound: all-ones masks, every lane enters every node
    "all_ones": (F.tiny_scene, 32, 32, 2, 4, CUSTOM_CAM),
}

_want = {}


def reference(oracle, case, st):
    key = (case, st["accumulate_quantum"])
    if key not in _want:
        scene, w, h, spp, depth, cam = CASES[case]
        sc = oracle.scene(scene) if isinstance(scene, str) else scene()
        cfg = oracle.config(w, h, spp, depth, **oracle.partition(st), **cam)
        _want[key] = oracle.render(cfg, sc)
    return _want[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("cost", [False, True], ids=["plain", "cost"])
@pytest.mark.parametrize("case", list(CASES))
def test_footprint_bitwise(oracle, monkeypatch, case, cost):
    scene, w, h, spp, depth, cam = CASES[case]
    sc = scene if isinstance(scene, str) else scene()
    if cost:
        monkeypatch.setenv("VCRT_WORK_ORDER", "cost")
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=vc.KERNEL_CULL_FLAT, **cam)
    with vc.Renderer(desc, sc) as r:
        for frame in range(2 if cost else 1):  # cost order: the measuring frame, then the order
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
            want, segs = reference(oracle, case, st)
            what = f"{case} cost={cost} frame {frame}"
            assert st["kernel"] == "vcrt_trace_cull_flat" + ("_cost" if cost else ""), what
            assert np.array_equal(bits(got), bits(want)), what
            assert st["segments"] == segs, what
    print(f"{case} cost={cost}: bound_tests {st['bound_tests']} group_tests {st['group_tests']} "
          f"segments {st['segments']}")
