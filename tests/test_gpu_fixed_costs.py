"""GPU parity of the flat scan's trimmed per-iteration code (tracer.hip group_foot_mask with
kFootBitop: the group mask by two v_bitop3 a word, a ray that never reaches the y extent reading
the tables' zero row). The masks are the parent's bit for bit, so every frame is the CPU oracle's
with its segment count, and the stats build's group_tests, segments, quanta and retire_iters are
the parent commit's.

Frames (the final scene at 44 x 20: both edges partial):
 - spp 1, 3, 4, 5 and 9 in items of 4 and 8 samples with G = 4, at depth 1 and depth 10: items of
   one quantum, ragged last quanta, items that end on the sample that ends a quantum (the retire's
   corner);
 - VCRT_FETCH_MIN=1, and VCRT_FETCH_MIN=8 with VCRT_FETCH_WAIT=2 (the deferred fetch's rules);
 - both ranks of a two-way shard (the drain and its steal), the cost-order build, a lens frame;
 - a camera above the spheres that looks straight up (no ray reaches the y extent: only the zero
   row and `always`), one inside the slab of small spheres, and a scene of 16 groups, whose tables
   fill their LDS bytes exactly, so that the zero row takes the one float4 the image grows by
   (vcrt_kernel_abi.h group_foot_zero_pad).

PARENT holds the parent commit's stats build (its code object under this host library) on the
frames of STATS, recorded twice with equal numbers; the constants do not come from the build under
test. retire_iters is held equal, not below: the deferred retire (a lane's finished quantum waits
one iteration for the wave's next retire) was not built, because a lane whose quantum ended in
iteration i can end its next sample in the camera phase of iteration i + 1 (a pending sky or depth
limit, or a fresh camera ray that leaves through the sky), which adds to `acc` before a retire at
the top of iteration i + 2: every finished lane is such a lane.
"""
import pytest

import vulkancomputeraytracing_amd as vc
from tests import group_footprint_ref as G
from tests import lens_ref as L
from tests import ray_query_ref as R
from tests import test_gpu_iter_trim as IT
from tests.stats_layout import dbg
from tests.test_gpu_lens import assert_same

pytestmark = pytest.mark.gpu

W, H = 44, 20
G4 = dict(accumulate_quantum=4, accumulate_tail=-1)
UP_CAM = dict(lookfrom=(0.0, 4.0, 0.0), lookat=(0.0, 9.0, 0.0), vup=(0.0, 0.0, 1.0), vfov=40.0)
SLAB_CAM = dict(lookfrom=(3.0, 0.2, 2.0), lookat=(0.0, 0.2, 0.0), vfov=50.0)
FETCH = {"min1": {"VCRT_FETCH_MIN": "1"},
         "min8wait2": {"VCRT_FETCH_MIN": "8", "VCRT_FETCH_WAIT": "2"}}


def render(oracle, monkeypatch, case, env=None, **kw):
    for name in ("VCRT_FETCH_MIN", "VCRT_FETCH_WAIT"):
        monkeypatch.delenv(name, raising=False)
    st = None
    # (IT.frames clears the suite's other variables itself; these two it leaves alone)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    try:
        st = IT.frames(oracle, monkeypatch, case, **kw)
    finally:
        for name in (env or {}):
            monkeypatch.delenv(name, raising=False)
    return st


@pytest.mark.parametrize("depth", [1, 10])
@pytest.mark.parametrize("spp", [1, 3, 4, 5, 9])
def test_retire_corners(oracle, monkeypatch, spp, depth):
    for chunk in (4, 8):
        (st,) = render(oracle, monkeypatch, ("final", W, H, spp, depth), accumulate_chunk=chunk,
                       **G4)
        assert st["kernel"] == "vcrt_trace_cull_flat"
        assert st["accumulate_quantum"] == 4


@pytest.mark.parametrize("rule", list(FETCH))
@pytest.mark.parametrize("depth", [1, 10])
def test_fetch_rules(oracle, monkeypatch, rule, depth):
    for spp, chunk in ((5, 4), (9, 8)):
        (st,) = render(oracle, monkeypatch, ("final", W, H, spp, depth), env=FETCH[rule],
                       accumulate_chunk=chunk, **G4)
        assert st["kernel"] == "vcrt_trace_cull_flat"


@pytest.mark.parametrize("rank", [0, 1])
def test_two_rank_shard(oracle, monkeypatch, rank):
    # items of four quanta: once the queues are empty the drain has quanta to steal
    render(oracle, monkeypatch, ("final", W, H, 17, 10), rank=rank, world_size=2,
           accumulate_chunk=16, **G4)


def test_cost_order(oracle, monkeypatch):
    # (IT.frames clears VCRT_WORK_ORDER: the plain frame's oracle image, then the loop here)
    case = ("final", W, H, 5, 10)
    fields = dict(accumulate_chunk=4, **G4)
    (st,) = render(oracle, monkeypatch, case, **fields)
    want, segs = oracle.render(oracle.config(W, H, 5, 10, **oracle.partition(st)),
                               oracle.scene("final"))
    monkeypatch.setenv("VCRT_WORK_ORDER", "cost")
    desc = vc.RenderDesc(width=W, height=H, samples_per_pixel=5, max_depth=10, device=0,
                         kernel_variant=vc.KERNEL_CULL_FLAT, **fields)
    with vc.Renderer(desc, "final") as r:
        for frame in range(2):  # the measuring frame, then the order
            r.draw_next_frame()
            got, sc = r.read_framebuffer(), r.stats()
            assert sc["kernel"] == "vcrt_trace_cull_flat_cost", frame
            assert sc["accumulate_quantum"] == st["accumulate_quantum"] == 4
            assert_same(got, want, f"cost order frame {frame}")
            assert sc["segments"] == segs, frame
    assert sc["cost_order"] != 0


def test_lens_frame(oracle):
    sc = R.scene_of(oracle, "final")
    desc = vc.RenderDesc(width=24, height=16, samples_per_pixel=5, max_depth=10, device=0,
                         lens_radius=0.1)
    with vc.Renderer(desc, sc) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    want, segs = L.reference_frame(oracle, sc, desc)
    assert st["kernel"].startswith("vcrt_trace_cull_flat_lens")
    assert_same(got, want, "lens 24x16x5")
    assert st["segments"] == segs


# ---- the stats build against the parent's ----------------------------------------------------

#          case, camera, desc fields
STATS = {
    "final5": (("final", W, H, 5, 10), {}, dict(accumulate_chunk=4, **G4)),
    "up": (("final", W, H, 4, 10), UP_CAM, {}),
    "slab": (("final", W, H, 4, 10), SLAB_CAM, {}),
    "grid12": (("grid12", 24, 16, 8, 8), G.GRID_CAM, {}),  # 16 groups: the image grows by the row
}
COUNTERS = ("group_tests", "segments", "quanta_retired", "retire_iters")
# the parent commit's vcrt_trace_cull_flat_stats, COUNTERS in that order
PARENT = {
    "final5": [1642, 9235, 1760, 247],
    "up": [102, 3520, 880, 18],
    "slab": [1483, 9436, 880, 163],
    "grid12": [373, 5288, 768, 41],
}


def stats_counters(oracle, monkeypatch, name, **kw):
    """The stats build's frame of STATS[name] (image and segments checked) and its COUNTERS."""
    case, cam, fields = STATS[name]
    (ss,) = render(oracle, monkeypatch, case, cam=cam, stats=True, **fields, **kw)
    assert ss["kernel"] == "vcrt_trace_cull_flat_stats"
    return ss, [ss[c] if c in ss else dbg(ss, c) for c in COUNTERS]


@pytest.mark.parametrize("name", list(STATS))
def test_stats_counters_as_the_parent(oracle, monkeypatch, name):
    case, cam, fields = STATS[name]
    (st,) = render(oracle, monkeypatch, case, cam=cam, **fields)
    ss, got = stats_counters(oracle, monkeypatch, name)
    print(f"{name}: {dict(zip(COUNTERS, got))} product group_tests {st['group_tests']} "
          f"lds_bytes {st['lds_bytes']}")
    assert st["kernel"] == "vcrt_trace_cull_flat" and st["bound_tests"] == 0  # the group tables
    assert (ss["group_tests"], ss["segments"]) == (st["group_tests"], st["segments"])
    assert got == PARENT[name], dict(zip(COUNTERS, zip(got, PARENT[name])))
    if name == "grid12":  # 2 nodes of boxes + 16 records + the node tables, the row, four waves
        assert st["lds_bytes"] == 16 * (2 * 21 + 16 * 5 + 1) + 672 + 4 * 3464
    if name == "up":  # nothing above the camera: every sample is one camera ray into the sky
        assert st["segments"] == W * H * 4
