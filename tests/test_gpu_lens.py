"""Thin-lens frames on the GPU (vcrt_render_desc.lens_radius > 0): every pixel of every frame bit
for bit against tests/lens_ref.py -- the oracle's ray_color over the lens rays, accumulated by the
rule -- for each lens kernel, progressive frames, shards, the outlier path and the CLI. The
frames are the smallest that still have partial edge tiles, several quanta per pixel and several
blocks per wave."""
import os
import subprocess

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import lens_ref as L
from tests import ray_query_ref as R

pytestmark = pytest.mark.gpu
N = vc._native

W, H, SPP, DEPTH, RADIUS = 44, 20, 8, 6, 0.1   # both edges partial; two quanta of the rule's G = 4


def desc_of(**kw):
    base = dict(width=W, height=H, samples_per_pixel=SPP, max_depth=DEPTH, device=0,
                lens_radius=RADIUS)
    base.update(kw)
    return vc.RenderDesc(**base)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what):
    """All pixels, none excluded: NaN positions coincide, every other word is equal."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    diff = np.argwhere((bits(got) != bits(want)) & ~gn)
    assert len(diff) == 0, f"{what}: {len(diff)} words differ, first {diff[:5].tolist()}"


def render(desc, scene, frames=1):
    with vc.Renderer(desc, scene) as r:
        for _ in range(frames):
            r.draw_next_frame()
        return r.read_framebuffer(), r.stats()


_gpu = {}


def final_frame(oracle):
    """The 44x20x8 lens frame of the final scene with every default (AUTO, G = 4), once."""
    if "final" not in _gpu:
        _gpu["final"] = render(desc_of(), R.scene_of(oracle, "final"))
    return _gpu["final"]


def lens_symbol(pinhole_kernel):
    """The lens build of a pinhole frame kernel: vcrt_trace_x[_cost] -> vcrt_trace_x_lens[_cost]."""
    cost = pinhole_kernel.endswith("_cost")
    base = pinhole_kernel[:-len("_cost")] if cost else pinhole_kernel
    return base + "_lens" + ("_cost" if cost else "")


def test_oracle_parity(oracle):
    sc = R.scene_of(oracle, "final")
    # one quantum covers the pixel: the reference's sequential fp32 sum, divided
    d_seq = desc_of(accumulate_quantum=8)
    got, st = render(d_seq, sc)
    want, segs = L.reference_frame(oracle, sc, d_seq)
    assert st["accumulate_quantum"] == 8
    assert_same(got, want, "G = 8")
    assert st["segments"] == segs
    # the rule's quantum: two quantized quanta per pixel
    got, st = final_frame(oracle)
    want4, segs4 = L.reference_frame(oracle, sc, desc_of())
    assert st["accumulate_quantum"] == 4
    assert_same(got, want4, "G = 4")
    assert st["segments"] == segs4 == segs
    assert st["kernel"].startswith("vcrt_trace_cull_flat_lens")
    # the lens moves the image: it is not the pinhole's
    pin, _ = render(desc_of(lens_radius=0.0), sc)
    assert (bits(pin) != bits(got)).any()


@pytest.mark.parametrize("variant,tables,symbol", [
    (N.KERNEL_AUTO, None, "vcrt_trace_cull_flat"),
    (N.KERNEL_SMEM, None, "vcrt_trace_smem"),
    (N.KERNEL_CULL_FLAT, None, "vcrt_trace_cull_flat"),
    (N.KERNEL_CULL_FLAT, "global", "vcrt_trace_cull_flat_global"),
    (N.KERNEL_CULL_FLAT, "boxes", "vcrt_trace_cull_flat_boxes"),
])
def test_variants(oracle, monkeypatch, variant, tables, symbol):
    sc = R.scene_of(oracle, "final")
    want, want_st = final_frame(oracle)
    if tables:
        monkeypatch.setenv("VCRT_CULL_LANE_TABLES", tables)
    got, st = render(desc_of(kernel_variant=variant), sc)
    _, pin = render(desc_of(kernel_variant=variant, lens_radius=0.0), sc)
    assert_same(got, want, f"variant {variant} tables {tables}")
    assert st["segments"] == want_st["segments"]
    assert pin["kernel"] in (symbol, symbol + "_cost")
    assert st["kernel"] == lens_symbol(pin["kernel"])


def test_agrees_with_ray_queries(oracle):
    sc = R.scene_of(oracle, "final")
    want, _ = final_frame(oracle)
    d = desc_of()
    origins, dirs = L.frame_rays(oracle, d)
    O = np.ascontiguousarray(np.broadcast_to(origins, dirs.shape)).reshape(-1, 3)
    with vc.Renderer(d, sc) as r:
        rad = r.trace_rays(O, dirs.reshape(-1, 3), DEPTH)
    img = L.accumulate_frame(oracle, rad[:, :3].reshape(H, W, SPP, 3), 4, SPP)
    assert_same(img, want, "trace_rays on the lens rays")


@pytest.mark.parametrize("name,w,h,spp,depth,symbol", [
    ("three", 24, 16, 4, 8, "vcrt_trace_smem_lens"),               # no tables
    ("stress4096", 24, 16, 4, 4, "vcrt_trace_cull_flat_boxes_lens"),
    ("mixed", 24, 16, 8, 6, "vcrt_trace_cull_flat_lens"),          # no shared slab
])
def test_small_and_large_scenes(oracle, name, w, h, spp, depth, symbol):
    sc = R.scene_of(oracle, name)
    d = desc_of(width=w, height=h, samples_per_pixel=spp, max_depth=depth)
    got, st = render(d, sc)
    want, segs = L.reference_frame(oracle, sc, d)
    assert_same(got, want, name)
    assert st["segments"] == segs
    assert st["kernel"] in (symbol, symbol + "_cost")


def test_progressive(oracle):
    sc = R.scene_of(oracle, "final")
    d = desc_of(samples_per_pixel=4, progressive=True)
    want1, segs1 = L.reference_frame(oracle, sc, d, frames=1)   # sample indices 0..3
    want2, segs2 = L.reference_frame(oracle, sc, d, frames=2)   # 0..7, quanta restart per frame
    with vc.Renderer(d, sc) as r:
        r.draw_next_frame()
        f1, s1 = r.read_framebuffer(), r.stats()
        r.draw_next_frame()
        f2, s2 = r.read_framebuffer(), r.stats()
        r.reset_accumulation()
        r.draw_next_frame()
        again, s3 = r.read_framebuffer(), r.stats()
    assert_same(f1, want1, "frame 0")
    assert_same(f2, want2, "frame 1")
    assert (s1["segments"], s2["segments"]) == (segs1, segs2)
    assert s2["accumulated_spp"] == 8 and s3["accumulated_spp"] == 4
    assert_same(again, f1, "after reset_accumulation")
    assert s3["segments"] == segs1


@pytest.mark.parametrize("world", [2, 3])
def test_sharding(oracle, world):
    sc = R.scene_of(oracle, "final")
    want, want_st = final_frame(oracle)
    m = vc.tile_pixel_map(W, H, world)
    segs = 0
    for rank in range(world):
        got, st = render(desc_of(rank=rank, world_size=world), sc)
        mine = m[..., 0] == rank
        assert_same(got.reshape(-1, 4)[m[..., 1][mine]], want[mine], f"rank {rank} of {world}")
        assert st["kernel"].startswith("vcrt_trace_cull_flat_lens")
        segs += st["segments"]
    assert segs == want_st["segments"]


def test_outlier_path(oracle):
    sc = oracle.bright_scene(3.0)
    d = desc_of(width=24, height=16, samples_per_pixel=16, max_depth=8)
    want, segs = L.reference_frame(oracle, sc, d)   # per-pixel scales (oracle.pixel_scale_log2)
    got, st = render(d, sc)
    assert st["scale_rerenders"] >= 1 and st["accumulate_scale_log2"] < 32
    assert_same(got, want, "bright scene")
    assert st["segments"] == segs


def test_zero_radius_is_the_pinhole(oracle):
    sc = R.scene_of(oracle, "final")
    never = vc.RenderDesc(width=W, height=H, samples_per_pixel=SPP, max_depth=DEPTH, device=0)
    a, sa = render(never, sc)
    b, sb = render(desc_of(lens_radius=0.0), sc)
    assert_same(b, a, "lens_radius 0")
    assert sa["kernel"] == sb["kernel"] and "lens" not in sb["kernel"]
    assert sa["segments"] == sb["segments"]
    want, segs = oracle.render(oracle.config(W, H, SPP, DEPTH, **oracle.partition(sa)), sc)
    assert_same(a, want, "pinhole against the oracle")


@pytest.mark.parametrize("variant", [N.KERNEL_LDS, N.KERNEL_CULL, N.KERNEL_CULL_LANE])
def test_unsupported_variants(oracle, variant):
    with pytest.raises(vc.VcrtError) as e:
        vc.Renderer(desc_of(kernel_variant=variant), "final")
    assert e.value.code == N.VK_ERROR_FEATURE_NOT_PRESENT
    # a pinhole renderer of that variant in the same process still works
    sc = R.scene_of(oracle, "final")
    got, st = render(desc_of(kernel_variant=variant, lens_radius=0.0), sc)
    want, segs = oracle.render(oracle.config(W, H, SPP, DEPTH, **oracle.partition(st)), sc)
    assert_same(got, want, f"pinhole variant {variant}")
    assert st["segments"] == segs


def test_stats_builds_unsupported(monkeypatch):
    monkeypatch.setenv("VCRT_DEBUG_STATS", "1")
    with pytest.raises(vc.VcrtError) as e:
        vc.Renderer(desc_of(), "final")
    assert e.value.code == N.VK_ERROR_FEATURE_NOT_PRESENT


def test_cli(oracle, tmp_path):
    from tests.test_gpu_configs import read_pfm
    want, want_st = final_frame(oracle)
    out = tmp_path / "lens.pfm"
    cmd = [os.path.join(N.BIN_DIR, "vcrt_render"), "--scene", "final", "--width", str(W),
           "--height", str(H), "--spp", str(SPP), "--depth", str(DEPTH), "--lens-radius",
           str(RADIUS), "--out", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip().endswith(f"{want_st['segments']} segments")
    assert_same(read_pfm(out), want[..., :3], "vcrt_render --lens-radius")
