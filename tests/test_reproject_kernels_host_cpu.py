"""The temporal accumulation kernel (csrc/reproject.hip) without a GPU: compiled for the host with
g++ against a stand-in for the HIP runtime and run one thread at a time over the generated planes
of tests/reproject_ref -- motion that points outside the frame on every side, partial taps,
integers, NaN, infinities, 1e30 -- its planes equal vcrt_reproject_host's word for word. The
driver runs the launch of csrc/image_pass_plan.hpp's reproject_plan, the one the library makes
(csrc/image_passes.cpp). The same driver, a stand-alone program, also runs built with -fsanitize=address,undefined over exactly sized
heap planes: this is where "no plane is read outside the frame" is pinned.
tests/test_gpu_reproject.py pins the device's arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from tests import reproject_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkancomputeraytracing_amd", "csrc")


def build(exe, *extra):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-Wno-unknown-pragmas", *extra, "-x", "c++", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "tests", "reproject_host"), "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "reproject_host_driver.cpp"),
                    os.path.join(CSRC, "reproject.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("reproject")
    return {"plain": build(str(d / "reproject_host_driver")),
            "sanitized": build(str(d / "reproject_host_driver_san"), "-g",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}


@pytest.fixture(scope="module")
def plane_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("planes")
    files = {}
    for w, h in P.SHAPES:
        path = str(d / f"planes_{w}x{h}.f32")
        with open(path, "wb") as f:
            for a in P.planes(w, h):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        files[(w, h)] = path
    return files


def run(exe, path, w, h, name):
    p = P.PARAM_SETS[name]
    res = subprocess.run([exe, path, str(w), str(h), repr(p["alpha"]), repr(p["max_history"]),
                          repr(p["depth_tolerance"])], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    words = res.stdout.split()
    return dict(zip(words[::2], (int(v) for v in words[1::2])))


@pytest.mark.parametrize("build_kind", ["plain", "sanitized"])
@pytest.mark.parametrize("name", list(P.PARAM_SETS))
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_host_definition(drivers, plane_files, shape, name, build_kind):
    w, h = shape
    r = run(drivers[build_kind], plane_files[shape], w, h, name)
    assert r["bad"] == 0 and r["pixels"] == w * h
    took = P.reference(w, h, name)[2]
    assert r["accepted"] == int(took.sum())
