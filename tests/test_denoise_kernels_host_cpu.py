"""The denoise kernels (csrc/denoise.hip) without a GPU: compiled for the host with g++ against a
stand-in for the HIP runtime -- the direct kernel one thread at a time, the LDS kernel's workgroup
as 256 threads around a barrier -- their planes equal vcrt_denoise_host's word for word. The
driver runs the launches of csrc/image_pass_plan.hpp's denoise_plan, the ones the library makes
(csrc/image_passes.cpp). This pins the kernels' logic and the library's sequencing: the tap order,
the skipped taps, the staged footprint's indexing, the fused demodulation, the flags, the grids
and the ping-pong; tests/test_gpu_denoise.py pins the device's arithmetic."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkancomputeraytracing_amd", "csrc")

# width, height, levels, the four sigmas, demodulate, leading LDS passes, albedo, guides
CASES = {
    "all-lds": (44, 20, 5, 0.5, 0.1, 0.25, 3.0, 1, 2, 1, 1),
    "all-direct": (44, 20, 5, 0.5, 0.1, 0.25, 3.0, 1, 0, 1, 1),
    "one-lds-pass": (44, 20, 3, 0.5, 0.1, 0.25, 3.0, 1, 1, 1, 1),
    "wide-no-demodulation": (70, 5, 3, 0.5, 0.1, 0.25, 3.0, 0, 2, 1, 1),
    "tiny": (3, 2, 5, 0.5, 0.1, 0.25, 3.0, 1, 2, 1, 1),
    "one-pixel": (1, 1, 1, 0.5, 0.1, 0.25, 3.0, 1, 1, 1, 1),
    "colour-only-no-guides": (44, 20, 2, 0, 0, 0, 2.0, 1, 2, 1, 0),
    "no-albedo-8": (44, 20, 8, 0.7, 0.2, 0.5, 9.0, 1, 2, 0, 1),
    "one-pass-first-and-last": (100, 37, 1, 0.7, 0.2, 0.5, 2.0, 1, 1, 1, 1),
    "two-passes-lds-last": (33, 9, 2, 0.7, 0.2, 0.5, 2.0, 1, 2, 1, 1),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("denoise") / "denoise_host_driver")
    subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-Wno-unknown-pragmas", "-x", "c++", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "tests", "denoise_host"), "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "denoise_host_driver.cpp"),
                    os.path.join(CSRC, "denoise.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("case", list(CASES))
def test_kernels_equal_the_host_definition(driver, case):
    args = CASES[case]
    res = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    words = res.stdout.split()
    r = dict(zip(words[::2], (int(v) for v in words[1::2])))
    assert r["bad"] == 0 and r["pixels"] == args[0] * args[1]
    assert r["lds"] == min(args[8], args[2], 2)
