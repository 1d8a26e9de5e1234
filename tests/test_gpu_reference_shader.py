"""The GPU kernels against the reference's own compute shader, through the recorded fixture
tests/golden/reference_shader.npz (tests/reference_shader_ref.py): frames
at the fixture's pixels, Renderer.trace_rays and Renderer.occluded, bit for bit (NaN against NaN
counts as equal). Frames use one accumulation quantum per pixel, the reference's sequential fp32
sum. Nothing here reads the reference: the fixture is data."""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import reference_shader_ref as RS

pytestmark = pytest.mark.gpu

FX = RS.load_fixture()
FRAMES = RS.frame_names(FX)


VARIANT_NAMES = {vc.KERNEL_AUTO: "auto", vc.KERNEL_SMEM: "smem", vc.KERNEL_CULL_FLAT: "cull_flat"}


def frame_params():
    """AUTO and SMEM for every case, the flat culled scan too for the 485-sphere scene; one
    frame per test."""
    out = []
    for name in FRAMES:
        final = int(FX["frame_scene"][FRAMES.index(name)]) < 0
        for v in (vc.KERNEL_AUTO, vc.KERNEL_SMEM) + ((vc.KERNEL_CULL_FLAT,) if final else ()):
            out.append(pytest.param(name, v, id=f"{name}-{VARIANT_NAMES[v]}"))
    return out


@pytest.mark.parametrize("name,variant", frame_params())
def test_frames_equal_the_reference_shader(name, variant):
    c = RS.frame_case(FX, name)
    w, h, spp, depth = c["cfg"]
    x, y = c["xy"][:, 0], c["xy"][:, 1]
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=variant,
                         accumulate_quantum=1 << (spp - 1).bit_length(),  # a power of two >= spp
                         **RS.cam_kwargs(c["cam"]))
    with vc.Renderer(desc, "final" if c["scene"] is None else c["scene"]) as r:
        r.draw_next_frame()
        got, st = r.read_framebuffer(), r.stats()
    assert got.shape == (h, w, 4) and st["accumulate_quantum"] >= spp
    if variant != vc.KERNEL_AUTO and depth > 0:  # (depth 0 launches no tracer)
        assert st["kernel_variant"] == variant
    px = got[y, x]
    assert (RS.canon_bits(px[:, 3]) == 0x3F800000).all()
    bad = RS.differing_blocks(RS.digests(px[:, :3], c["block"]), c["digests"])
    assert bad.size == 0, (f"blocks {bad[:8]} of {len(c['digests'])} differ "
                           f"({'rows' if c['whole'] else 'runs of 64 listed pixels'})")
    dead = c["undefined"] == spp   # every sample took ray_color's undefined return
    assert (RS.canon_bits(px[dead, :3]) == 0).all()


@pytest.mark.parametrize("scene", RS.RAY_SCENES)
def test_trace_rays_equal_the_reference_shader(oracle, scene):
    sc, rc = RS.ray_scene(oracle, FX, scene), RS.ray_case(FX, scene)
    O, D, C = FX["ray_O"], FX["ray_D"], FX["ray_class"]
    desc = vc.RenderDesc(width=64, height=40, samples_per_pixel=1, max_depth=10, device=0)
    with vc.Renderer(desc, sc) as r:
        for depth in RS.RAY_DEPTHS:
            rad, hits = r.trace_rays(O, D, depth, hits=True)
            bad = RS.differing_blocks(RS.class_digests(rad[:, :3], C), rc["rgb"][depth])
            assert bad.size == 0, f"{scene} depth {depth}: classes {[RS.RAY_CLASSES[b] for b in bad]}"
            assert (RS.canon_bits(rad[rc["undefined"][depth], :3]) == 0).all()
            bad = np.nonzero(RS.canon_bits(hits["t"]) != rc["t"])[0]
            assert bad.size == 0, f"{scene} depth {depth}: t of rays {bad[:8]} ({bad.size})"
            assert np.array_equal(hits["sphere"], rc["sphere"])
            assert np.array_equal(hits["sphere"] >= 0, rc["accepted"])
            bad = RS.differing_blocks(RS.class_digests(hits["normal"], C), rc["normal"])
            assert bad.size == 0, f"{scene}: normals of classes {[RS.RAY_CLASSES[b] for b in bad]}"


def test_root_test_boundaries_equal_the_reference_shader():
    """The fixture's hand-aimed rays: a near root equal to min_t, two roots that tie, reaches on
    and one ulp above an accepted root."""
    sc, O, D = FX["edge_scene"], FX["edge_O"], FX["edge_D"]
    desc = vc.RenderDesc(width=64, height=40, samples_per_pixel=1, max_depth=10, device=0)
    with vc.Renderer(desc, sc) as r:
        for i, depth in enumerate(RS.RAY_DEPTHS):
            rad, hits = r.trace_rays(O, D, depth, hits=True)
            assert np.array_equal(RS.canon_bits(rad[:, :3]), FX["edge_rgb"][i]), f"depth {depth}"
            assert np.array_equal(RS.canon_bits(hits["t"]), FX["edge_t"])
            assert np.array_equal(hits["sphere"], FX["edge_sphere"])
            assert np.array_equal(RS.canon_bits(hits["normal"]), FX["edge_normal"])
        occ = r.occluded(O, D, np.ascontiguousarray(FX["edge_T"]))
    assert np.array_equal(occ, FX["edge_occluded"] != 0)


@pytest.mark.parametrize("scene", RS.RAY_SCENES)
def test_occluded_equals_the_reference_hit_sphere(oracle, scene):
    sc, rc = RS.ray_scene(oracle, FX, scene), RS.ray_case(FX, scene)
    O, D = FX["ray_O"], FX["ray_D"]
    desc = vc.RenderDesc(width=64, height=40, samples_per_pixel=1, max_depth=10, device=0)
    with vc.Renderer(desc, sc) as r:
        occ = r.occluded(O, D, np.ascontiguousarray(rc["T"]))
        dflt = r.occluded(O, D)
    bad = np.nonzero(occ != rc["occluded"])[0]
    assert bad.size == 0, f"{scene}: rays {bad[:8]} ({bad.size})"
    assert np.array_equal(dflt, rc["accepted"])
