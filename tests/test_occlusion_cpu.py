"""Occlusion queries without a GPU: the numpy restatement against the first-hit helper, the
composition of the per-ray reaches (so that the GPU parity in test_gpu_occlusion.py cannot pass
vacuously), and the argument checks of the C ABI and of Renderer.occluded."""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import occlusion_ref as Q
from tests import ray_query_ref as R

N = vc._native


@pytest.mark.parametrize("scene", R.SCENES)
def test_reference_and_reaches(oracle, scene):
    _, _, C = R.ray_batch(oracle)
    ref = Q.reference(oracle, scene)
    fin, T, kind, occ = ref["finite"], ref["T"], ref["kind"], ref["occ"]
    t, sphere = ref["t"], ref["sphere"]
    hit = fin & (sphere >= 0)
    assert not np.isnan(T[fin]).any()
    # the rule: up to the first-hit query's own far limit, occluded == a first hit nearer than T
    rule = fin & (T <= R.INFINITY)
    assert np.array_equal(occ[rule], ((sphere >= 0) & (t < T))[rule])
    assert np.array_equal(ref["occ_default"][fin], (sphere >= 0)[fin])
    # the boundary is sharp: T on the accepted root leaves the ray unoccluded, one ulp above
    # occludes it
    k0, k1 = hit & (kind == 0), hit & (kind == 1)
    far = fin & ref["far_first"] & occ
    several = fin & (ref["accepting"] >= 2)
    beyond = fin & (kind == 5) & occ & (sphere < 0)
    print(f"{scene}: kind 0 {k0.sum()}, kind 1 {k1.sum()}, far root {far.sum()}, "
          f"several {several.sum()}, beyond 1e5 {beyond.sum()}")
    assert k0.sum() >= 250 and not occ[k0].any()
    assert k1.sum() >= 250 and occ[k1].all()
    # +inf sees what the first-hit query does, and may see more (hits beyond 1e5: class G)
    k5 = fin & (kind == 5)
    assert np.all(occ[k5] >= (sphere >= 0)[k5])
    assert np.all(C[beyond] == "G")
    assert not occ[fin & (kind == 7)].any()  # T = min_t: nothing between
    assert far.sum() >= 50
    assert several.sum() >= 100


def test_occlude_rays_before_begin():
    lib = N.lib()
    assert lib.vcrt_end() == 0  # no renderer: idempotent
    o = np.zeros((2, 3), np.float32)
    t = np.ones(2, np.float32)
    out = np.full(2, 0xA5, np.uint8)
    for f in (lib.vcrt_occlude_rays, lib.vcrt_occlude_rays_device):
        for tm in (None, t.ctypes.data):
            assert f(o.ctypes.data, o.ctypes.data, tm, 2, out.ctypes.data, None) == \
                N.VK_ERROR_INITIALIZATION_FAILED
    assert np.all(out == 0xA5)


def test_python_argument_errors_need_no_gpu():
    r = object.__new__(vc.Renderer)  # no vcrt_begin: validation comes before any native call
    good = np.zeros((5, 3), np.float32)
    for o, d, t in ((np.zeros((5, 4), np.float32), good, None),
                    (good, np.zeros((5, 2), np.float32), None),
                    (good, np.zeros((4, 3), np.float32), None),
                    (np.zeros(15, np.float32), np.zeros(15, np.float32), None),
                    (good, good, np.ones(4, np.float32)),
                    (good, good, np.ones((5, 1), np.float32)),
                    (good, good, "far")):
        with pytest.raises(ValueError):
            r.occluded(o, d, t)
    with pytest.raises(ValueError):
        r.visible(good, np.zeros((4, 3), np.float32))


def test_python_torch_argument_errors_need_no_gpu():
    torch = pytest.importorskip("torch")
    r = object.__new__(vc.Renderer)
    good = np.zeros((5, 3), np.float32)
    with pytest.raises(ValueError):  # torch tensors are taken as they are: float32 only
        r.occluded(torch.zeros((5, 3), dtype=torch.float64),
                   torch.zeros((5, 3), dtype=torch.float64))
    with pytest.raises(ValueError):  # and not mixed with numpy
        r.occluded(torch.zeros((5, 3)), good)
    with pytest.raises(ValueError):
        r.occluded(good, good, torch.ones(5))
