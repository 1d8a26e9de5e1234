"""A refused code object leaves no HIP error behind: vcrt_shader_load reports a file that is no
gfx950 code object through its result, and the next kernel launch of whoever shares the HIP
runtime -- here torch's fill behind draw_motion(device=True) -- does not find that error in its
own launch check."""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc

pytestmark = pytest.mark.gpu
N = vc._native


def test_a_torch_launch_after_a_refused_code_object(tmp_path):
    import torch
    junk = tmp_path / "junk.hsaco"
    junk.write_bytes(b"not a code object" * 64)
    desc = vc.RenderDesc(width=16, height=16, samples_per_pixel=1, max_depth=2, device=0)
    with vc.Renderer(desc, "three") as r:
        with pytest.raises(vc.VcrtError) as e:
            r.shader_load(str(junk))
        assert e.value.code == N.VK_ERROR_INCOMPATIBLE_SHADER_BINARY_EXT
        z = torch.zeros((4, 4), device="cuda:0")  # a kernel launch and its launch check
        assert float(z.sum()) == 0.0
        mo = r.draw_motion(device=True, stats=True)  # the old code object still serves
        assert mo["stats"]["identity"] == 16 * 16
        assert np.array_equal(mo["motion"][..., 0].cpu().numpy(),
                              np.tile(np.arange(16, dtype=np.float32), (16, 1)))
