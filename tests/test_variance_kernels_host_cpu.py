"""The variance-guided kernels (csrc/variance.hip) without a GPU: compiled for the host with g++
against a stand-in for the HIP runtime and run over the generated planes of tests/variance_ref --
the direct kernels one thread at a time, the LDS kernel's workgroup as 256 threads around a
barrier -- their planes equal the _host functions' word for word. The driver runs the launches of
csrc/image_pass_plan.hpp's plans, the ones the library makes (csrc/image_passes.cpp), so the
library's own sequencing is what is checked against the definitions. The same driver, a stand-alone
program, also runs built with -fsanitize=address,undefined over exactly sized heap planes: this is
where "no plane is read outside the frame" is pinned for the new planes.
tests/test_gpu_variance.py pins the device's arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from tests import variance_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkancomputeraytracing_amd", "csrc")
ORDER = ("colour", "motion", "hcol", "hsurf", "hlen", "albedo", "nd", "hmom", "moments",
         "surface", "var")

# width, height, set, demodulate, leading LDS passes, albedo, guides
DENOISE_CASES = {
    "all-lds": (44, 20, "all", 1, 2, 1, 1),
    "all-direct": (44, 20, "all", 1, 0, 1, 1),
    "one-lds-pass": (44, 20, "normal", 1, 1, 1, 1),
    "wide-no-demodulation": (70, 5, "all", 0, 2, 1, 1),
    "tiny": (3, 2, "all", 1, 2, 1, 1),
    "one-pixel": (1, 1, "all-1", 1, 1, 1, 1),
    "colour-only-no-guides": (44, 20, "colour", 1, 2, 1, 0),
    "no-albedo-8": (44, 20, "all-8", 1, 2, 0, 1),
    "one-pass-first-and-last": (100, 37, "all-1", 1, 1, 1, 1),
    "colour-off": (44, 20, "depth", 1, 2, 1, 1),
    "none": (70, 5, "none", 1, 2, 0, 0),
}


def build(exe, *extra):
    subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-Wno-unknown-pragmas", *extra, "-x", "c++", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "tests", "variance_host"), "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "variance_host_driver.cpp"),
                    os.path.join(CSRC, "variance.cpp"), os.path.join(CSRC, "reproject.cpp"),
                    os.path.join(CSRC, "denoise.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("variance")
    return {"plain": build(str(d / "variance_host_driver")),
            "sanitized": build(str(d / "variance_host_driver_san"), "-g",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}


@pytest.fixture(scope="module")
def plane_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("planes")
    files = {}
    for w, h in V.SHAPES:
        path = str(d / f"planes_{w}x{h}.f32")
        p = V.planes(w, h)
        with open(path, "wb") as f:
            for name in ORDER:
                f.write(np.ascontiguousarray(p[name], np.float32).tobytes())
        files[(w, h)] = path
    return files


def run(exe, path, w, h, *args):
    res = subprocess.run([exe, path, str(w), str(h)] + [str(a) for a in args],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    words = res.stdout.split()
    return dict(zip(words[::2], (int(v) for v in words[1::2])))


@pytest.mark.parametrize("build_kind", ["plain", "sanitized"])
@pytest.mark.parametrize("name", list(V.MOMENTS_SETS))
@pytest.mark.parametrize("shape", V.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_kernel_equals_the_host_definition(drivers, plane_files, shape, name, build_kind):
    w, h = shape
    p = V.MOMENTS_SETS[name]
    for albedo in (1, 0):
        r = run(drivers[build_kind], plane_files[shape], w, h, "moments", repr(p["alpha"]),
                repr(p["max_history"]), repr(p["depth_tolerance"]), repr(p["alpha_moments"]),
                albedo)
        assert r["bad"] == 0 and r["pixels"] == w * h
        assert r["tally"] == int(V.moments_reference(w, h, name)[3].sum())


@pytest.mark.parametrize("build_kind", ["plain", "sanitized"])
@pytest.mark.parametrize("name", list(V.VARIANCE_SETS))
@pytest.mark.parametrize("shape", V.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_variance_kernel_equals_the_host_definition(drivers, plane_files, shape, name, build_kind):
    w, h = shape
    p = V.VARIANCE_SETS[name]
    for lds in (0, 1):
        r = run(drivers[build_kind], plane_files[shape], w, h, "variance",
                repr(p["min_history"]), repr(p["alpha"]), lds)
        assert r["bad"] == 0 and r["pixels"] == w * h and r["lds"] == lds
        assert r["tally"] == int(V.variance_reference(w, h, name)[1].sum())


@pytest.mark.parametrize("build_kind", ["plain", "sanitized"])
@pytest.mark.parametrize("case", list(DENOISE_CASES))
def test_denoise_kernels_equal_the_host_definition(drivers, plane_files, case, build_kind):
    w, h, name, demodulate, lds, albedo, guides = DENOISE_CASES[case]
    p = V.DENOISE_SETS[name]
    r = run(drivers[build_kind], plane_files[(w, h)], w, h, "denoise", p["levels"],
            repr(p["sigma_normal"]), repr(p["sigma_depth"]), repr(p["sigma_albedo"]),
            repr(p["sigma_colour"]), demodulate, lds, albedo, guides)
    assert r["bad"] == 0 and r["pixels"] == w * h
    assert r["lds"] == min(lds, p["levels"], 2)
