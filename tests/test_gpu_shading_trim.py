"""GPU checks of the trimmed hit shading (tracer.hip unit_of and rand_arg_first, vcrt_math.h
sin_accept with the small-argument threshold at 2^-20): the helpers' own self-tests on the device
and parity frames through every kernel family that shades.

 - vcrt_selftest_unit (kernel vcrt_check_unit: unit_of alone) on 2^20 seeded triples and the edge
   triples of tests/test_unit_rcp_cpu.py, against numpy's float32 sqrt and division bit for bit
   (NaN for NaN: the all-zero triple and the NaN and infinite components).
 - vcrt_selftest_sin over the positive bit patterns of [2^-12, 2^10): no mismatch, and its fallback
   count is the rejected count of tests/test_sin_guard_cpu.py's host mirror on the same range
   (the device and the host run one predicate), below the 25 432 of the predicate before.
 - Frames against the CPU oracle, image and segments: the final scene at 44 x 20, spp 5, depth 10
   and depth 1; "three" at 24 x 16, spp 8 (the linear scan's kernel); both ranks of a two-way
   shard; a thin-lens frame.
 - The stats build of the first frame: group_tests and segments are the product build's, and with
   quanta_retired and retire_iters the numbers tests/test_gpu_fixed_costs.py holds for this frame;
   kUnitFallback, the full division's region, is never entered.
"""
import ctypes

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import lens_ref as L
from tests import ray_query_ref as R
from tests import test_gpu_fixed_costs as FC
from tests import test_gpu_iter_trim as IT
from tests import test_sin_guard_cpu as SG
from tests import test_unit_rcp_cpu as UR
from tests.stats_layout import REGION_DEBUG_BASE
from tests.test_gpu_lens import assert_same

pytestmark = pytest.mark.gpu
N = vc._native

PARENT_FALLBACKS = 25_432  # 2^-12 <= |x| < 2^10 with the threshold at 2^-12 (test_sin_poly_cpu.py)


@pytest.fixture(scope="module")
def begun():
    desc = vc.RenderDesc(width=8, height=8, samples_per_pixel=1, max_depth=1, device=0)
    with vc.Renderer(desc, "red"):
        yield N.lib()


def device_unit(lib, t):
    t = np.ascontiguousarray(t, dtype=np.float32)
    out = np.full_like(t, -7.0)
    assert lib.vcrt_selftest_unit(t.ctypes.data, len(t), out.ctypes.data) == 0
    return out


def test_unit_vector_selftest(begun):
    edge, _ = UR.edges()
    t = np.concatenate([UR.random_triples(1 << 20, seed=20), edge])
    got, want = device_unit(begun, t), UR.reference(t)
    diff = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    assert not diff.any(), (int(diff.sum()), t[diff.any(axis=1)][:4], got[diff.any(axis=1)][:4])
    assert np.isnan(got[-len(edge):][(edge == 0).all(axis=1)]).all()  # 0 / 0 by the full division
    zero_in = (t == 0) & ~np.isnan(want)
    assert (got[zero_in].view(np.uint32) == 0).all()  # +0
    # one triple, and none
    assert UR.same_bits(device_unit(begun, t[:1]), want[:1])
    assert begun.vcrt_selftest_unit(None, 0, None) == 0


def test_sin_fallbacks_are_the_host_predicates(begun, tmp_path_factory):
    mirror = SG.build(tmp_path_factory.mktemp("sin_guard_gpu"), "sin_guard")
    rejected = SG.mirror_rejected(mirror, SG.K12M, SG.K10)
    bad, fb, first_bad = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
    r = begun.vcrt_selftest_sin(SG.K12M, SG.K10 - SG.K12M, ctypes.byref(bad), ctypes.byref(fb),
                                ctypes.byref(first_bad))
    assert r == 0
    print(f"2^-12 <= x < 2^10: device fallbacks {fb.value}, host mirror rejected {rejected}")
    assert bad.value == 0, f"first bit pattern {first_bad.value:#010x}"
    assert fb.value == rejected
    assert fb.value < PARENT_FALLBACKS


FIRST = FC.STATS["final5"]  # the final scene at 44 x 20, spp 5, depth 10, items of one quantum


@pytest.mark.parametrize("depth", [10, 1])
def test_final_scene(oracle, monkeypatch, depth):
    case, cam, fields = FIRST
    (st,) = FC.render(oracle, monkeypatch, case[:4] + (depth,), cam=cam, **fields)
    assert st["kernel"] == "vcrt_trace_cull_flat"


def test_three_spheres_linear_scan(oracle, monkeypatch):
    (st,) = IT.frames(oracle, monkeypatch, ("three", 24, 16, 8, 10), variant=N.KERNEL_AUTO)
    assert "cull" not in st["kernel"]


@pytest.mark.parametrize("rank", [0, 1])
def test_two_rank_shard(oracle, monkeypatch, rank):
    IT.frames(oracle, monkeypatch, ("final", 44, 20, 5, 10), rank=rank, world_size=2)


def test_lens_frame(oracle):
    sc = R.scene_of(oracle, "final")
    desc = vc.RenderDesc(width=24, height=16, samples_per_pixel=5, max_depth=10, device=0,
                         lens_radius=0.07)
    with vc.Renderer(desc, sc) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    want, segs = L.reference_frame(oracle, sc, desc)
    assert st["kernel"].startswith("vcrt_trace_cull_flat_lens")
    assert_same(got, want, "lens 24x16x5")
    assert st["segments"] == segs


def test_stats_build_of_the_first_frame(oracle, monkeypatch):
    from tools import valu_regions
    with open(valu_regions.TRACER) as f:
        unit_fallback = valu_regions.enum_values(f.read())["kUnitFallback"]
    case, cam, fields = FIRST
    (st,) = FC.render(oracle, monkeypatch, case, cam=cam, **fields)
    ss, got = FC.stats_counters(oracle, monkeypatch, "final5")
    print(dict(zip(FC.COUNTERS, got)), "kUnitFallback", ss["debug"][REGION_DEBUG_BASE + unit_fallback])
    assert (ss["group_tests"], ss["segments"]) == (st["group_tests"], st["segments"])
    assert got == FC.PARENT["final5"]
    assert ss["debug"][REGION_DEBUG_BASE + unit_fallback] == 0
