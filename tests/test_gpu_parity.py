"""GPU parity: the gfx950 tracer (through the C ABI) against the CPU oracle.

Bar (DESIGN.md "Parity"): bit-identical images and identical segment counts on every config
the oracle finishes in seconds; at BASELINE sizes, bit-identical rows on an oracle-rendered
row subset and per-channel RMS <= 1e-4 (north_star tolerance) over those rows.
"""
import ctypes
import os

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from vulkancomputeraytracing_amd import _native as N

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4  # north_star: per-channel RMS <= 1e-4 vs reference
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def gpu_render(scene, width, height, spp, depth, variant=vc.KERNEL_AUTO, rank=0, world=1,
               frames=1, scene_arr=None, chunk=0, quantum=0):
    desc = vc.RenderDesc(width=width, height=height, samples_per_pixel=spp, max_depth=depth,
                         kernel_variant=variant, rank=rank, world_size=world, device=0,
                         accumulate_chunk=chunk, accumulate_quantum=quantum)
    with vc.Renderer(desc, scene_arr if scene_arr is not None else scene) as r:
        for _ in range(frames):
            r.draw_next_frame()
        return r.read_framebuffer(), r.stats()


def chunk_of(w, h, spp, chunk=0, world=1, tail=0, tail_chunk=0, quantum=0):
    """The accumulation quantum and the work partition the renderer uses, as oracle.config()
    keywords (C ABI vcrt_work_quantum, vcrt_work_chunk and vcrt_work_tail, no
    re-implementation). The oracle's image depends on the quantum alone."""
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, accumulate_chunk=chunk,
                         world_size=world, accumulate_tail=tail, accumulate_tail_chunk=tail_chunk,
                         accumulate_quantum=quantum)
    t, kt = vc.renderer.work_tail(desc)
    return dict(chunk=vc.renderer.work_chunk(desc), tail=t, tail_chunk=kt,
                quantum=vc.renderer.work_quantum(desc))


def seq_quantum(spp):
    """The smallest quantum (a power of two) that covers spp samples: one quantum per pixel,
    the reference's sequential sum and division (shader.comp:46-56)."""
    return 1 << (spp - 1).bit_length()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bitwise(got, want, what=""):
    if not np.array_equal(bits(got), bits(want)):
        diff = np.argwhere(bits(got) != bits(want))
        rms = np.sqrt(np.nanmean((got.astype(np.float64) - want) ** 2, axis=(0, 1)))
        raise AssertionError(f"{what}: {len(diff)} words differ, first {diff[:5].tolist()}, "
                             f"per-channel rms {rms}")


CASES = [
    # BASELINE config 1 (CPU plumbing config) run on the GPU too
    ("red", 256, 144, 1, 1),
    ("three", 200, 112, 8, 8),     # config 2 scene, reduced size
    ("final", 160, 90, 4, 10),     # config 3 scene, reduced size
    ("final", 96, 54, 2, 50),      # reference depth (MAX_RECURSION_LEVEL 50)
    ("three", 37, 23, 3, 5),       # ragged sizes (not multiples of 8/16)
    ("red", 1, 1, 5, 3),           # single pixel
    ("final", 50, 1, 2, 10),       # single row
]


VARIANTS = [vc.KERNEL_LDS, vc.KERNEL_SMEM, vc.KERNEL_CULL, vc.KERNEL_CULL_LANE,
            vc.KERNEL_CULL_FLAT]
CULLED = (vc.KERNEL_CULL, vc.KERNEL_CULL_LANE, vc.KERNEL_CULL_FLAT)


def expected_variant(variant, nspheres):
    # the culled scans need >= 16 spheres (vcrt.h); below that the linear SMEM scan runs
    return vc.KERNEL_SMEM if variant in CULLED and nspheres < 16 else variant


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scene,w,h,spp,depth", CASES)
def test_bitwise_vs_oracle(oracle, scene, w, h, spp, depth, variant):
    got, st = gpu_render(scene, w, h, spp, depth, variant)
    # default accumulation: the oracle sums in the same quanta
    assert oracle.partition(st) == chunk_of(w, h, spp)
    want, want_segs = oracle.render(oracle.config(w, h, spp, depth,
                                                  **oracle.partition(st)),
                                    oracle.scene(scene))
    assert got.shape == want.shape
    assert_bitwise(got, want, f"{scene} {w}x{h} spp{spp} d{depth} v{variant}")
    assert st["segments"] == want_segs
    assert st["kernel_variant"] == expected_variant(variant, st["nspheres"])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scene,w,h,spp,depth,chunk,quantum", [
    ("final", 64, 36, 64, 10, 16, 0),   # 4 items of one quantum (16)
    ("final", 48, 30, 40, 10, 0, 0),    # the default for a tiny frame: ten quanta of 4
    ("three", 72, 40, 96, 8, 7, 1),     # 14 items (the last of 5), every sample a quantum
    ("final", 64, 36, 48, 10, 32, 4),   # items of 8 quanta (the last of 4): mid-item retires
    ("three", 40, 24, 40, 8, 0, 8),     # 5 quanta of 8 inside items of 32 and 8
    ("final", 40, 24, 33, 10, 33, 64),  # one quantum = the reference's sequential order
])
def test_chunked_accumulation_bitwise_vs_oracle(oracle, scene, w, h, spp, depth, chunk, quantum,
                                                variant):
    k = chunk_of(w, h, spp, chunk, quantum=quantum)
    want, want_segs = oracle.render(oracle.config(w, h, spp, depth, **k), oracle.scene(scene))
    got, st = gpu_render(scene, w, h, spp, depth, variant, chunk=chunk, quantum=quantum)
    assert oracle.partition(st) == k
    assert_bitwise(got, want, f"{scene} spp{spp} chunk{k}")
    assert st["segments"] == want_segs
    # the chunked order stays within the north_star tolerance of the sequential order
    seq, _ = oracle.render(oracle.config(w, h, spp, depth), oracle.scene(scene))
    rms = np.sqrt(((got.astype(np.float64) - seq) ** 2).mean(axis=(0, 1)))
    assert np.all(rms <= RMS_TOL), rms
    assert np.all(rms <= 1e-6), rms  # in practice a few ulps


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scene,w,h,spp,depth,chunk,tail,tail_chunk,quantum", [
    ("final", 64, 36, 40, 10, 8, 12, 5, 1),   # head 28 = 8+8+8+4, tail 12 = 5+5+2
    ("three", 72, 40, 33, 8, 16, 9, 1, 1),    # a tail of single samples
    ("final", 40, 24, 20, 10, 16, 6, 4, 1),   # the head one chunk of 14
    ("final", 64, 36, 40, 10, 16, 16, 4, 4),  # head 24 = 16+8, tail 16 = 4 x 4: whole quanta
    ("three", 72, 40, 36, 8, 8, 10, 2, 4),    # rounded to quanta: head 24, tail 12 in 4s
])
def test_tail_partition_bitwise_vs_oracle(oracle, scene, w, h, spp, depth, chunk, tail,
                                          tail_chunk, quantum, variant):
    """The tail of the work partition (the last samples of every pixel in their own items,
    handed out after the head), items holding whole quanta: the oracle's image, bit for bit."""
    k = chunk_of(w, h, spp, chunk, tail=tail, tail_chunk=tail_chunk, quantum=quantum)
    if quantum == 1:
        assert (k["tail"], k["tail_chunk"]) == (tail, tail_chunk)
    else:  # whole quanta: the head ends on a quantum boundary
        assert (spp - k["tail"]) % quantum == 0 and k["tail_chunk"] % quantum == 0
    want, want_segs = oracle.render(oracle.config(w, h, spp, depth, **k), oracle.scene(scene))
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=variant, accumulate_chunk=chunk, accumulate_tail=tail,
                         accumulate_tail_chunk=tail_chunk, accumulate_quantum=quantum)
    with vc.Renderer(desc, scene) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    assert oracle.partition(st) == k
    assert_bitwise(got, want, f"{scene} spp{spp} {k}")
    assert st["segments"] == want_segs


@pytest.mark.parametrize("world", [1, 3])
def test_tail_partition_progressive_and_sharded(oracle, world):
    """Progressive frames with a tail in each frame, rendered in `world` shards: every rank's
    pixels equal the oracle's at every frame."""
    w, h, spp, depth, frames = 56, 32, 10, 10, 2
    part = dict(chunk=3, tail=4, tail_chunk=2, quantum=1)
    m = vc.tile_pixel_map(w, h, world)
    sc = oracle.scene("final")
    wants = [oracle.render(oracle.config(w, h, (f + 1) * spp, depth, frame_spp=spp, **part),
                           sc)[0] for f in range(frames)]
    for rank in range(world):
        desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth,
                             device=0, rank=rank, world_size=world, progressive=True,
                             accumulate_chunk=3, accumulate_tail=4, accumulate_tail_chunk=2,
                             accumulate_quantum=1)
        mine = m[..., 0] == rank
        with vc.Renderer(desc, "final") as r:
            assert oracle.partition(r.stats()) == part
            for f in range(frames):
                r.draw_next_frame()
                got = r.read_framebuffer()
                if world > 1:
                    got = got.reshape(-1, 4)[m[..., 1][mine]]
                    assert_bitwise(got, wants[f][mine], f"rank {rank}/{world} frame {f}")
                else:
                    assert_bitwise(got, wants[f], f"frame {f}")


def test_golden_oracle_images():
    from tests.golden.make_golden import IMAGES
    data = np.load(os.path.join(GOLDEN, "oracle_images.npz"))
    for name, scene, w, h, spp, depth in IMAGES:
        # the goldens hold the reference's sequential sum: one quantum per pixel
        got, st = gpu_render(scene, w, h, spp, depth, quantum=seq_quantum(spp))
        assert_bitwise(got, data[name], name)
        assert st["segments"] == int(data[name + "__segments"][0])


def test_stress_scene_small(oracle):
    w, h, spp, depth = 48, 27, 2, 10
    want, segs = oracle.render(oracle.config(w, h, spp, depth), oracle.scene("stress4096"))
    for variant in (vc.KERNEL_AUTO, vc.KERNEL_SMEM, vc.KERNEL_CULL, vc.KERNEL_CULL_LANE,
                    vc.KERNEL_CULL_FLAT):
        got, st = gpu_render("stress4096", w, h, spp, depth, variant)
        assert_bitwise(got, want, f"stress v{variant}")
        assert st["segments"] == segs and st["nspheres"] == 4100


@pytest.mark.parametrize("tables", ["lds", "global"])
@pytest.mark.parametrize("scene", ["final", "stress4096"])
def test_per_lane_culled_scan_table_placement(oracle, monkeypatch, tables, scene):
    # the per-lane scan gathers table rows from an LDS copy or from global memory
    # (VCRT_CULL_LANE_TABLES forces either; the default picks LDS up to 32 KB)
    monkeypatch.setenv("VCRT_CULL_LANE_TABLES", tables)
    w, h, spp, depth = 40, 24, 3, 12
    k = chunk_of(w, h, spp, 0)
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **k), oracle.scene(scene))
    got, st = gpu_render(scene, w, h, spp, depth, vc.KERNEL_CULL_LANE)
    assert st["kernel_variant"] == vc.KERNEL_CULL_LANE
    assert_bitwise(got, want, f"{scene} lane tables={tables}")
    assert st["segments"] == segs
    if tables == "global":
        assert st["lds_bytes"] == 0 and not st["tables_in_lds"]
    elif scene == "final":  # 14 KB of tables: 256-thread workgroups, one copy each
        assert 0 < st["lds_bytes"] <= 32768 and st["block_threads"] == 256
        assert st["tables_in_lds"]
    elif st["lds_bytes"] > 0:  # 114 KB: one copy per 1024-thread workgroup
        assert st["lds_bytes"] > 32768 and st["block_threads"] == 1024
    # the flat scan: tables beside its stacks in LDS up to 32 KB, else the boxes alone in LDS
    # (up to 1024 groups), else everything in global memory
    got, st = gpu_render(scene, w, h, spp, depth, vc.KERNEL_CULL_FLAT)
    assert st["kernel_variant"] == vc.KERNEL_CULL_FLAT
    assert_bitwise(got, want, f"{scene} flat tables={tables}")
    assert st["segments"] == segs
    if tables == "global":
        assert st["tables_in_lds"] == 0
        assert st["lds_bytes"] == 4 * 6920 and st["block_threads"] == 256
    elif scene == "final":
        assert st["tables_in_lds"] == 1 and st["block_threads"] == 256
    else:
        assert st["tables_in_lds"] == 2 and st["block_threads"] == 1024
        assert st["kernel"] == "vcrt_trace_cull_flat_boxes"


@pytest.mark.parametrize("scene,w,h,spp,depth,chunk", [
    ("final", 40, 24, 3, 12, 0),
    ("stress4096", 48, 27, 4, 50, 0),
    ("stress4096", 37, 19, 6, 10, 4),
    ("random3000", 40, 24, 2, 8, 0),
    ("random9000", 40, 24, 2, 8, 0),
    ("torture", 33, 21, 5, 50, 5),
])
def test_flat_scan_boxes_in_lds(oracle, monkeypatch, scene, w, h, spp, depth, chunk):
    """The flat scan with only the boxes in LDS (1024-thread workgroups, group records from
    global memory, 16-bit stacks): bit-identical to the oracle; scenes beyond 1024 hierarchy
    groups fall back to the global-table kernel."""
    monkeypatch.setenv("VCRT_CULL_LANE_TABLES", "boxes")
    cfg = {}
    if scene.startswith("random"):
        n = int(scene[6:])
        sc = random_large_scene(n, seed=n)
        cfg = dict(lookfrom=(-80, 10, 5), lookat=(0, 0, 0), vfov=50)
    elif scene == "torture":
        sc = culling_torture_scene()
    else:
        sc = scene
    quantum = 1 if chunk else 0  # explicit items: a quantum per sample, several items per pixel
    k = chunk_of(w, h, spp, chunk, quantum=quantum)
    oscene = oracle.scene(sc) if isinstance(sc, str) else sc
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **k, **cfg), oscene)
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=vc.KERNEL_CULL_FLAT, accumulate_chunk=chunk,
                         accumulate_quantum=quantum, **cfg)
    with vc.Renderer(desc, sc) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    assert_bitwise(got, want, f"{scene} flat boxes")
    assert st["segments"] == segs
    if scene == "random9000":  # 2250 groups: beyond the 16-bit entries
        assert st["kernel"] == "vcrt_trace_cull_flat_global"
    else:
        assert st["kernel"] == "vcrt_trace_cull_flat_boxes"
        assert st["block_threads"] == 1024 and st["lds_bytes"] > 16 * 4360


def culling_torture_scene():
    """>= 16 spheres that stress the culled scan's exactness: exact duplicates with different
    materials (ties must go to the lower index), nested and overlapping spheres, a hollow glass
    shell (negative radius), spheres below the margin's r_min (1e-3), a huge sphere and a far
    one."""
    rng = np.random.default_rng(5)
    rows = [((0, -1000, 0), 1000.0, (0.5, 0.5, 0.5), 1, 0.0)]
    for i in range(24):
        c = (float(rng.uniform(-3, 3)), float(rng.uniform(0.1, 1.5)), float(rng.uniform(-3, 3)))
        r = float(rng.uniform(0.05, 0.6))
        rows.append((c, r, tuple(rng.uniform(0, 1, 3)), 1 + i % 3, float(rng.uniform(0, 1.6))))
        if i % 4 == 0:  # exact duplicate, other material
            rows.append((c, r, (1.0, 0.0, 0.0), 1 + (i + 1) % 3, 0.3))
        if i % 6 == 0:  # concentric inner sphere / hollow shell
            rows.append((c, -0.9 * r, (1, 1, 1), 3, 1.5))
    rows.append(((0.2, 0.5, 0.1), 5e-4, (0, 1, 0), 1, 0.0))    # tiny: never culled
    rows.append(((0.2, 0.5, 0.1), 5e-4, (0, 0, 1), 2, 0.0))    # its duplicate
    rows.append(((0, 4, -2), 3.0, (0.7, 0.6, 0.5), 2, 0.0))
    rows.append(((40, 3, 90), 2.0, (0.1, 0.8, 0.2), 1, 0.0))
    return vc.make_spheres(rows)


def random_large_scene(n, seed):
    """n spheres with log-uniform radii from 5e-4 to 2 (some below the culling margin's r_min),
    a few huge ones, all materials, in a 60-unit box seen from outside: many hierarchy chunks,
    tables far beyond LDS, several hits per path."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        c = tuple(float(v) for v in rng.uniform(-30, 30, 3))
        r = float(np.exp(rng.uniform(np.log(5e-4), np.log(2.0))))
        if i % 997 == 0:
            r = float(rng.uniform(5, 15))
        rows.append((c, r, tuple(rng.uniform(0, 1, 3)), 1 + i % 3, float(rng.uniform(0, 1.6))))
    return vc.make_spheres(rows)


@pytest.mark.parametrize("n", [3000, 9000])
def test_large_random_scene_all_variants(oracle, n):
    sc = random_large_scene(n, seed=n)
    w, h, spp, depth = 40, 24, 2, 8
    cfg = dict(lookfrom=(-80, 10, 5), lookat=(0, 0, 0), vfov=50)
    k = chunk_of(w, h, spp, 0)
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **k, **cfg), sc)
    for variant in (vc.KERNEL_SMEM, vc.KERNEL_CULL, vc.KERNEL_CULL_LANE, vc.KERNEL_CULL_FLAT):
        desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth,
                             device=0, kernel_variant=variant, **cfg)
        with vc.Renderer(desc, sc) as r:
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
        assert st["kernel_variant"] == variant and st["nspheres"] == n
        if variant == vc.KERNEL_CULL_FLAT:  # tables beyond 32 KB: boxes only in LDS (up to
            # 1024 groups), else the global-table flat kernel
            assert st["tables_in_lds"] == (2 if n <= 4096 else 0)
        assert_bitwise(got, want, f"random {n} v{variant}")
        assert st["segments"] == segs


@pytest.mark.parametrize("w,h,spp,depth,chunk", [(64, 40, 8, 12, 0), (33, 21, 5, 50, 5)])
def test_culled_scan_torture_scene(oracle, w, h, spp, depth, chunk):
    sc = culling_torture_scene()
    assert len(sc) >= 16
    cfg = dict(lookfrom=(6, 2.5, 5), lookat=(0, 0.6, 0), vfov=45)
    quantum = 1 if chunk else 0
    k = chunk_of(w, h, spp, chunk, quantum=quantum)
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **k, **cfg), sc)
    for variant in (vc.KERNEL_SMEM, vc.KERNEL_CULL, vc.KERNEL_CULL_LANE, vc.KERNEL_CULL_FLAT):
        desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth,
                             device=0, kernel_variant=variant, accumulate_chunk=chunk,
                             accumulate_quantum=quantum, **cfg)
        with vc.Renderer(desc, sc) as r:
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
        assert st["kernel_variant"] == variant
        assert_bitwise(got, want, f"torture v{variant}")
        assert st["segments"] == segs
        if variant in CULLED:
            assert 0 < st["group_tests"]
            assert st["bound_tests"] > 0


@pytest.mark.parametrize("cam", [dict(lookfrom=(2, 0.3, 1.5), lookat=(-6, 0.2, -2), vfov=60),
                                 dict(lookfrom=(0.5, 30, 0.5), lookat=(0, 0, 0), vfov=30),
                                 dict(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vfov=20)])
def test_camera_ray_lists_bitwise(oracle, cam):
    """The flat scan's camera rays start from their pixel quarter's group list (csrc/primary.cpp):
    a camera inside the sphere field, one looking straight down and the reference camera, with
    the lists in use, give the oracle's bits and segment counts."""
    from vulkancomputeraytracing_amd import scene as S
    w, h, spp, depth = 192, 108, 3, 10
    sc = S.builtin_scene("final")
    pl = S.primary_lists(sc, vc.RenderDesc(width=w, height=h, **cam))
    assert ((pl["info"] & 15) != 15).mean() > 0.3  # the lists are in use
    k = chunk_of(w, h, spp, 0)
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **k, **cam), sc)
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         **cam)
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    assert st["kernel_variant"] == vc.KERNEL_CULL_FLAT
    assert_bitwise(got, want, f"camera {cam}")
    assert st["segments"] == segs


def test_custom_scene_and_empty_scene(oracle):
    custom = vc.make_spheres([((0, 0.5, -1), 0.5, (0.9, 0.1, 0.1), 2, 0.3),
                              ((1, 0.5, -1), 0.5, (1, 1, 1), 3, 1.5),
                              ((0, -100.5, -1), 100.0, (0.8, 0.8, 0.0), 1, 0.9)])
    cfg = oracle.config(64, 40, 4, 8, lookfrom=(0, 1, 3), lookat=(0, 0.5, -1), vfov=40)
    want, segs = oracle.render(cfg, custom)
    desc = vc.RenderDesc(width=64, height=40, samples_per_pixel=4, max_depth=8,
                         lookfrom=(0, 1, 3), lookat=(0, 0.5, -1), vfov=40, device=0)
    with vc.Renderer(desc, custom) as r:
        r.draw_next_frame()
        assert_bitwise(r.read_framebuffer(), want, "custom")
        assert r.stats()["segments"] == segs
        # no spheres: every ray is sky
        r.set_scene(custom[:0])
        r.draw_next_frame()
        got = r.read_framebuffer()
    want0, _ = oracle.render(cfg, custom[:0])
    assert_bitwise(got, want0, "empty scene")


def test_depth_zero_fills_undefined_value():
    got, st = gpu_render("final", 33, 17, 3, 0)
    assert np.all(got[..., :3] == 0) and np.all(got[..., 3] == 1)
    assert st["segments"] == 0


def test_frames_are_identical(oracle):
    # the reference re-renders the same deterministic frame every DrawNextFrame
    desc = vc.RenderDesc(width=64, height=36, samples_per_pixel=2, max_depth=10, device=0)
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        a = r.read_framebuffer()
        r.draw_next_frame()
        b = r.read_framebuffer()
        assert r.stats()["frames"] == 2
    assert_bitwise(a, b, "frame 2 vs frame 1")


@pytest.mark.parametrize("world", [2, 3, 8, 5])
def test_sharded_tiles_reassemble_bitwise(world):
    import torch
    w, h, spp, depth = 75, 46, 2, 10  # ragged: edge tiles are partial
    full, _ = gpu_render("final", w, h, spp, depth)
    pad = max(len(vc.tiles_for_rank(w, h, world, r)) for r in range(world))
    m = vc.tile_pixel_map(w, h, world)
    gathered = torch.zeros((world, pad * 64, 4), dtype=torch.float32, device="cuda:0")
    for rank in range(world):
        part, st = gpu_render("final", w, h, spp, depth, rank=rank, world=world)
        ntiles = len(vc.tiles_for_rank(w, h, world, rank))
        assert part.shape == (ntiles, 64, 4) and st["local_tiles"] == ntiles
        mine = m[..., 0] == rank
        flat = part.reshape(-1, 4)
        assert_bitwise(flat[m[..., 1][mine]], full[mine], f"rank {rank}/{world}")
        gathered[rank, :ntiles * 64] = torch.from_numpy(flat).to("cuda:0")
    frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    desc = vc.RenderDesc(width=w, height=h, world_size=world, device=0)
    with vc.Renderer(desc) as r:
        r.assemble_tiles(gathered.data_ptr(), frame.data_ptr(), pad)
        with pytest.raises(vc.VcrtError):
            r.assemble_tiles(gathered.data_ptr(), frame.data_ptr(), pad - 1)
    torch.cuda.synchronize()
    assert_bitwise(frame.cpu().numpy(), full, "assembled")


def test_sharded_chunked_render_matches_oracle(oracle):
    # a rank shard with several sample chunks (resolve kernel on packed tiles)
    w, h, spp, depth, world = 64, 40, 24, 10, 3
    want, _ = oracle.render(oracle.config(w, h, spp, depth, quantum=8), oracle.scene("final"))
    m = vc.tile_pixel_map(w, h, world)
    for rank in range(world):
        part, st = gpu_render("final", w, h, spp, depth, rank=rank, world=world, chunk=8,
                              quantum=8)
        mine = m[..., 0] == rank
        assert_bitwise(part.reshape(-1, 4)[m[..., 1][mine]], want[mine], f"rank {rank}")


def test_render_into_external_device_buffer():
    import torch
    w, h = 40, 24
    ref, _ = gpu_render("three", w, h, 2, 6)
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=2, max_depth=6, device=0)
    buf = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda:0")
    with vc.Renderer(desc, "three") as r:
        r.set_framebuffer_device(buf.data_ptr(), buf.numel() * 4)
        r.draw_next_frame()
        torch.cuda.synchronize()
        assert_bitwise(buf.cpu().numpy(), ref, "external buffer")
        with pytest.raises(vc.VcrtError):
            r.set_framebuffer_device(buf.data_ptr(), 16)  # too small


def test_shader_load_from_file_and_errors(tmp_path):
    desc = vc.RenderDesc(width=16, height=16, samples_per_pixel=1, max_depth=4, device=0)
    with vc.Renderer(desc, "red") as r:
        r.shader_load(N.CODE_OBJECT_PATH)
        r.draw_next_frame()
        with pytest.raises(vc.VcrtError) as e:
            r.shader_load(str(tmp_path / "missing.hsaco"))
        assert e.value.code == N.VK_ERROR_INCOMPATIBLE_SHADER_BINARY_EXT
        junk = tmp_path / "junk.hsaco"
        junk.write_bytes(b"\x7fELF not a code object" * 8)
        with pytest.raises(vc.VcrtError) as e:
            r.shader_load(str(junk))
        assert e.value.code == N.VK_ERROR_INCOMPATIBLE_SHADER_BINARY_EXT
        r.draw_next_frame()  # previous module still bound


def test_reference_named_lifecycle():
    vc.SetRenderDescription(vc.RenderDesc(width=32, height=18, samples_per_pixel=1,
                                          max_depth=5, device=0))
    vc.SetRenderScene(vc.builtin_scene("three"))
    assert vc.BeginRenderingOperation() == vc.VK_SUCCESS
    assert vc.DrawNextFrame() == vc.VK_SUCCESS
    assert vc.EndRenderingOperation() == vc.VK_SUCCESS
    assert vc.EndRenderingOperation() == vc.VK_SUCCESS
    assert vc.DrawNextFrame() == vc.VK_ERROR_INITIALIZATION_FAILED
    vc.SetRenderScene(None)


@pytest.mark.parametrize("variant", [vc.KERNEL_AUTO, vc.KERNEL_SMEM, vc.KERNEL_CULL_LANE,
                                     vc.KERNEL_CULL_FLAT])
def test_full_size_rows_subset_rms(oracle, variant):
    # BASELINE config 3 geometry (1920x1080, depth 10) at 16 spp; oracle renders every 90th row.
    w, h, spp, depth = 1920, 1080, 16, 10
    got, st = gpu_render("final", w, h, spp, depth, variant)
    rows = range(7, h, 90)
    want, _ = oracle.render(oracle.config(w, h, spp, depth, **oracle.partition(st)),
                            oracle.scene("final"), rows=rows)
    sel = list(rows)
    g, o = got[sel].astype(np.float64), want[sel].astype(np.float64)
    rms = np.sqrt(((g - o) ** 2).mean(axis=(0, 1)))
    assert np.all(rms[:3] <= RMS_TOL), rms
    assert_bitwise(got[sel], want[sel], "full-size row subset")
    # size-independent properties of the whole frame
    assert np.all(got[..., 3] == 1.0)
    assert np.all(np.isfinite(got)) and np.all(got[..., :3] >= 0)
    assert st["samples"] == w * h * spp
    assert st["segments"] >= w * h * spp  # at least one segment per sample


def test_srgb8_encode_bitwise(oracle):
    w, h = 96, 54
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=4, max_depth=10, device=0)
    with vc.Renderer(desc, "final") as r:
        r.draw_next_frame()
        lin = r.read_framebuffer()
        srgb = r.read_framebuffer_srgb8()
    assert srgb.shape == (h, w, 4) and srgb.dtype == np.uint8
    assert np.array_equal(srgb, oracle.encode_srgb8(lin))
    want, _ = oracle.render(oracle.config(w, h, 4, 10), oracle.scene("final"))
    assert np.array_equal(srgb, oracle.encode_srgb8(want))


@pytest.mark.parametrize("spp,chunk,quantum", [(4, 0, 0), (6, 4, 2), (3, 1, 1), (40, 0, 0)])
def test_progressive_frames_bitwise(oracle, spp, chunk, quantum):
    w, h, depth, frames = 48, 30, 10, 3
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         progressive=True, accumulate_chunk=chunk, accumulate_quantum=quantum)
    scene = oracle.scene("final")
    with vc.Renderer(desc, "final") as r:
        k = oracle.partition(r.stats())
        outs = []
        for f in range(frames):
            r.draw_next_frame()
            outs.append(r.read_framebuffer())
            assert r.stats()["accumulated_spp"] == (f + 1) * spp
        r.reset_accumulation()
        r.draw_next_frame()
        again = r.read_framebuffer()
    for f, got in enumerate(outs):
        want, _ = oracle.render(oracle.config(w, h, (f + 1) * spp, depth, **k,
                                              frame_spp=spp), scene)
        assert_bitwise(got, want, f"progressive frame {f}")
    assert_bitwise(again, outs[0], "after reset")


def test_sin_fast_exhaustive():
    """The kernel's sin (vcrt_math.h sin_fast: one polynomial modulo pi, accepted only when it
    provably rounds like the canonical sin, else the canonical fdlibm path) equals the canonical
    sin on every one of the 2^32 fp32 inputs, evaluated on the GPU."""
    import ctypes
    lib = vc._native.lib()
    desc = vc.RenderDesc(width=8, height=8, samples_per_pixel=1, max_depth=1, device=0)
    with vc.Renderer(desc, "red"):
        total_fallback = 0
        for first in range(0, 1 << 32, 1 << 30):  # four launches of 2^30 inputs
            bad, fb, first_bad = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
            r = lib.vcrt_selftest_sin(first, 1 << 30, ctypes.byref(bad), ctypes.byref(fb),
                                      ctypes.byref(first_bad))
            assert r == 0
            assert bad.value == 0, (f"{bad.value} inputs differ, first bit pattern "
                                    f"{first_bad.value:#010x}")
            total_fallback += fb.value
    # the fallback is rare for the arguments rand() sees, but counts every input >= 2^19, NaN
    # and inf (about 3/4 of all bit patterns)
    assert total_fallback < (1 << 32)


def test_bench_multirank_gather_bitwise():
    """bench.py's N-rank path end to end on one GPU (3 ranks rendering their tile shares in
    turn, gloo standing in for RCCL, which refuses two ranks on one device): the frame gathered
    to rank 0 and re-interleaved by vcrt_assemble is bit-identical to a default 1-GPU render.
    At N > 1 the --full line validates itself without --validate (the driver's
    first multi-GPU run must prove its gather): bitwise_vs_1gpu, the oracle rows, the per-rank
    kernel times and gather_ms are in the JSON."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, VCRT_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(root, "bench.py"),
           "--gpus", "3", "--steps", "1", "--warmup", "0", "--width", "200", "--height", "120",
           "--spp", "40", "--depth", "10", "--scene", "final", "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 3
    assert res["validated"]["bitwise_vs_1gpu"] is True
    assert res["validated"]["bitwise_vs_oracle"] is True
    assert res["validated"]["quantum"] == [4, 4]
    pr = res["per_rank_kernel_ms"]
    assert len(pr["ranks"]) == 3 and 0 < pr["min"] <= pr["max"]
    assert "gather_ms" in res


def test_bench_rccl_init_failure_falls_back_to_gloo():
    """bench.py's default N-rank path (RCCL inside libvcrt) when vcrt_comm_init fails on a rank:
    two ranks on one GPU (RCCL refuses a duplicate device). Every rank sees the failure through
    the all-reduced flag, opens a fresh renderer and gathers through gloo; the job completes,
    names the path in config.gather, and the frame is bit-identical to a 1-GPU render."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k != "VCRT_DIST_BACKEND"}
    env["VCRT_COMM_TIMEOUT_MS"] = "20000"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "1", "--warmup", "0", "--width", "160", "--height", "96",
           "--spp", "8", "--depth", "10", "--scene", "final", "--full", "--no-cpu-baseline",
           "--validate"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2
    assert res["config"]["gather"].startswith("gloo fallback"), res["config"]["gather"]
    assert res["validated"]["bitwise_vs_1gpu"] is True


def test_rccl_comm_inside_libvcrt_world1(oracle):
    """vcrt_comm_init (RCCL linked into libvcrt.so) on a one-rank communicator: the
    communicator comes up on the GPU, frames draw through the gather-aware path, the frame is
    the oracle's, and a second init or an external framebuffer is refused. (RCCL refuses two
    ranks on one device; the N-rank exchange is exercised by the driver's multi-GPU bench.)"""
    w, h, spp, depth = 96, 54, 4, 10
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0)
    cid = vc.renderer.comm_unique_id()
    with vc.Renderer(desc, "final") as r:
        r.comm_init(cid)
        with pytest.raises(vc.VcrtError):
            r.comm_init(cid)
        with pytest.raises(vc.VcrtError):
            r.set_framebuffer_device(1 << 20, 1 << 30)
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **oracle.partition(st)),
                               oracle.scene("final"))
    assert_bitwise(got, want, "comm world 1")
    assert st["segments"] == segs


def test_rccl_comm_missing_peer_fails_within_deadline(oracle, monkeypatch):
    """The communicator is non-blocking with a deadline (csrc/comm_wait.hpp): rank 0 of a
    2-rank world whose peer never joins gets VK_ERROR_INITIALIZATION_FAILED from vcrt_comm_init
    once VCRT_COMM_TIMEOUT_MS has passed -- instead of blocking forever -- the communicator is
    aborted, and the renderer goes on drawing its own shard (no gather), equal to the oracle's
    pixels. (The reference bubbles every error up as a VkResult: VulkanComputeRayTracing.cpp:
    20-35.)"""
    import time
    monkeypatch.setenv("VCRT_COMM_TIMEOUT_MS", "3000")
    w, h, spp, depth, world = 64, 40, 2, 10, 2
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         rank=0, world_size=world)
    cid = vc.renderer.comm_unique_id()
    with vc.Renderer(desc, "final") as r:
        t0 = time.monotonic()
        with pytest.raises(vc.VcrtError) as err:
            r.comm_init(cid)
        dt = time.monotonic() - t0
        assert err.value.code == N.VK_ERROR_INITIALIZATION_FAILED
        assert 2.5 <= dt < 60.0
        r.draw_next_frame()  # the shard still renders, without a gather
        part, st = r.read_framebuffer(), r.stats()
    want, _ = oracle.render(oracle.config(w, h, spp, depth, **oracle.partition(st)),
                            oracle.scene("final"))
    m = vc.tile_pixel_map(w, h, world)
    mine = m[..., 0] == 0
    assert_bitwise(part.reshape(-1, 4)[m[..., 1][mine]], want[mine], "rank 0 after comm failure")


def test_bench_single_gpu_validates_against_oracle():
    """bench.py --full at N = 1 validates its own frame by default (verdict r04 item 5): without
    --validate the line carries `validated`, whose two full-width rows at full spp are the
    oracle's bit for bit; --no-validate leaves it out."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0",
           "--config", "c3", "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    v = res["validated"]
    assert v["bitwise_vs_oracle"] is True
    assert v["pixels_vs_oracle"] == 2 * 1920 and v["pixel_stride"] == 1
    assert v["accumulate_scale_log2"] == 32
    out = subprocess.run(cmd + ["--no-validate"], cwd=root, capture_output=True, text=True,
                         timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    res2 = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert "validated" not in res2
    assert res["roofline"]["frac"] <= 1.0
    assert res["roofline"]["speedup_vs_bruteforce_at_peak"] > 1.0


def test_bench_plain_run_is_lean_and_dumps_its_frame(oracle, tmp_path):
    """A plain bench.py run (no --full) times exactly --steps steps and leaves out the
    validation and the CPU baseline; --dump-outputs writes the frame of the last timed step as
    framebuffer.npy (float32, [H][W][4]), which is the oracle's bit for bit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, spp, depth = 200, 120, 8, 10
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2",
           "--warmup", "1", "--min-warmup-seconds", "0", "--width", str(w), "--height", str(h),
           "--spp", str(spp), "--depth", str(depth), "--scene", "final",
           "--dump-outputs", str(tmp_path / "dump")]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert "validated" not in res and "cpu_baseline" not in res
    assert res["steps"] == 2 and out.stderr.count("] step ") == 2
    assert res["ms_per_step"] > 0 and res["unit"] == "Msamples/s" and res["dtype"] == "f32"
    # value and ms_per_step are the same measurement, each rounded to 3 decimals
    assert res["value"] == pytest.approx(w * h * spp / res["ms_per_step"] / 1e3,
                                         rel=1e-3 + 5e-4 / res["ms_per_step"])
    assert sorted(os.listdir(tmp_path / "dump")) == ["framebuffer.npy"]
    got = np.load(tmp_path / "dump" / "framebuffer.npy")
    assert got.dtype == np.float32 and got.shape == (h, w, 4)
    want, _ = oracle.render(oracle.config(w, h, spp, depth, **chunk_of(w, h, spp)),
                            oracle.scene("final"))
    assert_bitwise(got, want, "bench.py --dump-outputs")


@pytest.mark.parametrize("world", [3, 8])
def test_sharded_camera_ray_lists_bitwise(oracle, world):
    """Tile-sharded renders with the camera-ray lists in use (each rank builds the lists of its
    own tiles, indexed by local tile): every rank's pixels equal the oracle's."""
    from vulkancomputeraytracing_amd import distributed as D
    from vulkancomputeraytracing_amd import scene as S
    w, h, spp, depth = 320, 180, 2, 10
    sc = S.builtin_scene("final")
    k = chunk_of(w, h, spp, world=world)
    want, _ = oracle.render(oracle.config(w, h, spp, depth, **k), sc)
    m = vc.tile_pixel_map(w, h, world)
    for rank in range(world):
        pl = S.primary_lists(sc, vc.RenderDesc(width=w, height=h, rank=rank, world_size=world))
        assert ((pl["info"] & 15) != 15).mean() > 0.5
        part, st = gpu_render("final", w, h, spp, depth, rank=rank, world=world)
        assert oracle.partition(st) == k  # every rank: the largest rank's default
        mine = m[..., 0] == rank
        assert_bitwise(part.reshape(-1, 4)[m[..., 1][mine]], want[mine], f"rank {rank}/{world}")


def test_camera_ray_lists_switch_keeps_bits(monkeypatch):
    """VCRT_PRIMARY_LISTS=0 (camera rays through the hierarchy) and the default give the same
    image and segment count."""
    outs = []
    for v in ("0", "1"):
        monkeypatch.setenv("VCRT_PRIMARY_LISTS", v)
        outs.append(gpu_render("final", 256, 144, 4, 10))
    assert_bitwise(outs[0][0], outs[1][0], "lists off vs on")
    assert outs[0][1]["segments"] == outs[1][1]["segments"]
    assert outs[0][1]["bound_tests"] > outs[1][1]["bound_tests"]  # the lists skipped box tests


@pytest.mark.parametrize("scene,variant,kernel", [
    ("final", vc.KERNEL_AUTO, "vcrt_trace_cull_flat"),
    ("three", vc.KERNEL_AUTO, "vcrt_trace_smem"),
    ("stress4096", vc.KERNEL_AUTO, "vcrt_trace_cull_flat_boxes"),
    ("final", vc.KERNEL_LDS, "vcrt_trace_lds"),
    ("final", vc.KERNEL_CULL, "vcrt_trace_cull"),
    ("final", vc.KERNEL_CULL_LANE, "vcrt_trace_cull_lane_lds"),
])
def test_stats_name_the_launched_kernel(scene, variant, kernel):
    """vcrt_stats.kernel (and the shader stage's pName, Shader.cpp:89's analogue) is the code-
    object symbol the frame dispatched: what bench.py reports and rocprof lists."""
    _, st = gpu_render(scene, 64, 36, 1, 4, variant)
    assert st["kernel"] == kernel


@pytest.mark.parametrize("scene,w,h,spp,depth,chunk,tail,tail_chunk,quantum,ring", [
    ("final", 64, 36, 40, 10, 8, 12, 5, 1, "0"),      # ring off: sums straight to memory
    ("final", 64, 36, 40, 10, 8, 12, 5, 1, "8"),      # a small ring: entries recycled often
    ("three", 37, 23, 48, 8, 4, 0, 0, 4, "1"),        # ragged edge tiles, 12 items per pixel
    ("final", 50, 30, 33, 10, 7, 0, 0, 1, "1"),       # 5 items: blocks straddle pixels
    ("final", 50, 30, 64, 10, 32, 0, 0, 8, "1"),      # four quanta per item into one entry
    ("stress4096", 40, 24, 20, 12, 4, 8, 2, 2, "1"),  # the boxes-in-LDS kernel's ring
])
def test_accumulation_ring_bitwise(oracle, monkeypatch, scene, w, h, spp, depth, chunk, tail,
                                   tail_chunk, quantum, ring):
    """The per-wave LDS accumulation ring (tracer.hip RingEntry): quantum sums added in LDS and
    flushed per pixel give the same exact sums as adding every quantum sum to global memory."""
    monkeypatch.setenv("VCRT_ACCUM_RING", ring)
    k = chunk_of(w, h, spp, chunk, tail=tail, tail_chunk=tail_chunk, quantum=quantum)
    want, want_segs = oracle.render(oracle.config(w, h, spp, depth, **k), oracle.scene(scene))
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         accumulate_chunk=chunk, accumulate_tail=tail,
                         accumulate_tail_chunk=tail_chunk, accumulate_quantum=quantum)
    with vc.Renderer(desc, scene) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    assert_bitwise(got, want, f"{scene} ring={ring}")
    assert st["segments"] == want_segs
    if ring == "0":
        assert st["ring_entries"] == 0
    elif ring == "8":
        assert st["ring_entries"] == 8
    else:
        assert st["ring_entries"] >= 8


@pytest.mark.parametrize("scene,w,h,spp,depth,variant,tail,tail_chunk,tables", [
    ("three", 96, 54, 40, 8, vc.KERNEL_SMEM, 0, 0, ""),
    ("three", 37, 23, 48, 8, vc.KERNEL_SMEM, 16, 4, ""),   # ragged edge tiles, a tail part
    ("final", 40, 24, 12, 10, vc.KERNEL_LDS, 0, 0, ""),
    # the flat scans' cost-order builds: tables in LDS, boxes in LDS, tables in global memory
    ("final", 40, 24, 12, 10, vc.KERNEL_CULL_FLAT, 0, 0, ""),
    ("final", 37, 23, 48, 10, vc.KERNEL_CULL_FLAT, 16, 4, ""),
    ("final", 37, 23, 24, 10, vc.KERNEL_CULL_FLAT, 8, 4, "boxes"),
    ("final", 37, 23, 24, 10, vc.KERNEL_CULL_FLAT, 0, 0, "global"),
])
def test_cost_order_bitwise(oracle, monkeypatch, scene, w, h, spp, depth, variant, tail,
                            tail_chunk, tables):
    """The cost-ordered schedule (VCRT_WORK_ORDER=cost; automatic for frames with few items per
    lane and for the cost partition): the first frame counts each pixel's segments
    (TraceParams.pixel_cost), the next hands out the blocks most expensive first (block_order).
    Both frames are the oracle's image. The flat scans run their cost-order builds."""
    monkeypatch.setenv("VCRT_WORK_ORDER", "cost")
    if tables:
        monkeypatch.setenv("VCRT_CULL_LANE_TABLES", tables)
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=variant, accumulate_tail=tail,
                         accumulate_tail_chunk=tail_chunk)
    with vc.Renderer(desc, scene) as r:
        r.draw_next_frame()
        first, st1 = r.read_framebuffer(), r.stats()
        r.draw_next_frame()
        second, st2 = r.read_framebuffer(), r.stats()
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **oracle.partition(st1)),
                               oracle.scene(scene))
    assert (st1["cost_order"], st2["cost_order"]) == (0, 1)
    assert_bitwise(first, want, f"{scene} measuring frame")
    assert_bitwise(second, want, f"{scene} cost-ordered frame")
    assert st1["segments"] == st2["segments"] == segs
    flat = {"": "vcrt_trace_cull_flat", "boxes": "vcrt_trace_cull_flat_boxes",
            "global": "vcrt_trace_cull_flat_global"}
    if variant == vc.KERNEL_CULL_FLAT:
        assert st1["kernel"] == st2["kernel"] == flat[tables] + "_cost"


@pytest.mark.parametrize("world", [1, 4])
def test_cost_partition_bitwise(monkeypatch, world):
    """The cost partition (capi.cpp default_chunk): a frame whose largest rank has few items at
    the per-pixel rule's K keeps that K, has no tail and runs the cost order (here 48x32 at 1024
    spp: K = 64, where the item-count rule gives K = 16 and a tail). Every rank's framebuffer, on
    the measuring frame and the cost-ordered one, equals the static schedule's
    (VCRT_WORK_ORDER=static: the item-count partition) bit for bit; the image depends on the
    quantum alone (the static frames are the oracle's: test_bitwise_vs_oracle and the tail tests)."""
    w, h, spp, depth = 48, 32, 1024, 10
    for rank in range(world):
        desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth,
                             device=0, rank=rank, world_size=world)
        assert vc.renderer.work_chunk(desc) == 64 and vc.renderer.work_tail(desc) == (0, 0)
        with vc.Renderer(desc, "final") as r:
            r.draw_next_frame()
            first, st1 = r.read_framebuffer(), r.stats()
            r.draw_next_frame()
            second, st2 = r.read_framebuffer(), r.stats()
        assert (st1["cost_order"], st2["cost_order"]) == (0, 1)
        assert st2["kernel"] == "vcrt_trace_cull_flat_cost"
        assert (st2["accumulate_chunk"], st2["accumulate_tail"]) == (64, 0)
        monkeypatch.setenv("VCRT_WORK_ORDER", "static")
        assert vc.renderer.work_chunk(desc) == 16
        with vc.Renderer(desc, "final") as r:
            r.draw_next_frame()
            want, st = r.read_framebuffer(), r.stats()
        monkeypatch.delenv("VCRT_WORK_ORDER")
        assert st["cost_order"] == 0 and st["kernel"] == "vcrt_trace_cull_flat"
        assert st["accumulate_chunk"] == 16
        assert_bitwise(first, want, f"rank {rank}/{world} measuring frame")
        assert_bitwise(second, want, f"rank {rank}/{world} cost-ordered frame")
        assert st1["segments"] == st2["segments"] == st["segments"]


@pytest.mark.parametrize("scene,variant,cap", [("three", vc.KERNEL_SMEM, "3"),
                                               ("final", vc.KERNEL_CULL_FLAT, "2")])
def test_occupancy_cap_bitwise(oracle, monkeypatch, scene, variant, cap):
    """VCRT_MAX_BLOCKS_PER_CU caps the occupancy rule's workgroups per CU (the grid shrinks to
    cap x CUs) and keeps the LDS accumulation ring; the image is the oracle's."""
    monkeypatch.setenv("VCRT_MAX_BLOCKS_PER_CU", cap)
    w, h, spp, depth = 64, 36, 24, 8
    got, st = gpu_render(scene, w, h, spp, depth, variant)
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **oracle.partition(st)),
                               oracle.scene(scene))
    assert_bitwise(got, want, f"{scene} cap={cap}")
    assert st["segments"] == segs
    assert st["grid_blocks"] % int(cap) == 0 and st["grid_blocks"] <= 256 * int(cap)
    assert st["ring_entries"] >= 8


@pytest.mark.parametrize("stage", ["1", "0"])
@pytest.mark.parametrize("scene,w,h,spp,depth", [("three", 96, 54, 40, 8),   # staged: 1 KB
                                                  ("red", 24, 16, 506, 3),   # 8192 B: staged
                                                  ("red", 24, 16, 507, 3),   # 8208 B: global
                                                  ("red", 33, 21, 1200, 3),  # too big: global
                                                  ("final", 40, 24, 3, 10)])  # 485 spheres
def test_smem_staged_tables_bitwise(oracle, monkeypatch, stage, scene, w, h, spp, depth):
    """The SMEM scan's LDS copy of the shading rows and the jitter (TraceParams.stage_*, small
    scenes: C2) gives the oracle's bits, as does the global-memory path (VCRT_STAGE_TABLES=0, or
    tables beyond the staging budget)."""
    monkeypatch.setenv("VCRT_STAGE_TABLES", stage)
    got, st = gpu_render(scene, w, h, spp, depth, vc.KERNEL_SMEM)
    assert st["kernel"] == "vcrt_trace_smem"
    want, segs = oracle.render(oracle.config(w, h, spp, depth, **oracle.partition(st)),
                               oracle.scene(scene))
    assert_bitwise(got, want, f"{scene} staged={stage}")
    assert st["segments"] == segs
    # the host's budget: 48 B of shading rows per sphere + a float4 jitter term per sample
    staged = stage == "1" and 48 * st["nspheres"] + 16 * spp <= 8192
    assert (st["lds_bytes"] > 0) == staged


def _rel_rms(got, seq):
    d = got[..., :3].astype(np.float64) - seq[..., :3]
    return np.sqrt((d ** 2).mean(axis=(0, 1))) / np.sqrt(
        (seq[..., :3].astype(np.float64) ** 2).mean(axis=(0, 1)))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("param,depth", [(3.0, 8), (3.0, 50), (2.0, 50)])
def test_bright_scene_accumulation_faithful(oracle, variant, param, depth):
    """Accumulation holds any scene: the bright test scene (Lambertian param
    > 1, textures.glsl:22, white ground; tests/oracle_py.py) has quantum sums past 2^12, where a
    fixed 2^32 scale overflows the exact sums and round 5's per-scene bound (A^depth: 2^-38 at
    param 3, depth 50) rounded ordinary pixels to 0. Each pixel now takes its own scale from its
    own largest quantum sum (vcrt_math.h "Accumulation"): the first frame finds the outliers and
    renders again (scale_rerenders 1), later frames start at the recorded scales (0). The frame
    is finite, bit-identical to the oracle's restatement of the rule, and within 1e-4 RELATIVE
    per-channel RMS of the reference's sequential fp32 sum (shader.comp:46-56) -- relative since
    radiance passes 1 here; north_star's absolute 1e-4 is stated for [0, 1] radiance."""
    w, h, spp = 160, 90, 64
    sc = oracle.bright_scene(param)
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth,
                         kernel_variant=variant, device=0)
    with vc.Renderer(desc, sc) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
        r.draw_next_frame()
        again, st2 = r.read_framebuffer(), r.stats()
    assert st["scale_rerenders"] == 1 and st2["scale_rerenders"] == 0
    assert st["accumulate_scale_log2"] < 32 and st2["accumulate_scale_log2"] == \
        st["accumulate_scale_log2"]
    assert np.isfinite(got).all()
    want, seq, want_segs = oracle.render_seq(
        oracle.config(w, h, spp, depth, **oracle.partition(st)), sc)
    assert_bitwise(got, want, f"bright {param} d{depth} v{variant}")
    assert_bitwise(again, want, f"bright {param} d{depth} v{variant} second frame")
    assert st["segments"] == want_segs == st2["segments"]
    assert (_rel_rms(got, seq) <= RMS_TOL).all(), _rel_rms(got, seq)


def test_bright_scene_progressive_and_sharded(oracle):
    """The per-pixel scales with progressive frames and shards. Progressive: a frame whose
    pixels first pass 2^12 renders every frame so far again at the pixels' scales; every frame
    equals the oracle's progressive render bit for bit. Sharded: each rank measures its own
    pixels (a pixel's scale depends on its own samples only), so 3 ranks' tiles equal the 1-GPU
    frame bit for bit."""
    w, h, spp, depth, frames = 96, 54, 8, 50, 4
    sc = oracle.bright_scene(3.0)
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         progressive=True)
    rer = []
    with vc.Renderer(desc, sc) as r:
        k = oracle.partition(r.stats())
        for f in range(frames):
            r.draw_next_frame()
            got = r.read_framebuffer()
            rer.append(r.stats()["scale_rerenders"])
            want, _ = oracle.render(oracle.config(w, h, (f + 1) * spp, depth, **k,
                                                  frame_spp=spp), sc)
            assert_bitwise(got, want, f"bright progressive frame {f}")
    assert sum(rer) >= 1, rer
    full, st1 = gpu_render(None, w, h, 32, depth, scene_arr=sc)
    assert st1["scale_rerenders"] == 1
    world = 3
    m = vc.tile_pixel_map(w, h, world)
    for rank in range(world):
        part, st = gpu_render(None, w, h, 32, depth, rank=rank, world=world, scene_arr=sc)
        mine = m[..., 0] == rank
        assert_bitwise(part.reshape(-1, 4)[m[..., 1][mine]], full[mine], f"bright rank {rank}")
