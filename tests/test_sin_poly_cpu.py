"""The fast sine's polynomial on the CPU (vcrt_math.h sin_fast_try): a host mirror of the device
function, the same operations in the same order (double FMAs, the constants from kSinC itself),
compiled by the test and compared with sin_canonical.

Wherever the fast path accepts its value, that value must be sin_canonical's float, bit for bit:
on every fp32 input with |x| < 2^10 (2 * 0x44800000 bit patterns) and on 2^24 evenly strided bit
patterns of the rest. The GPU suite's test_sin_fast_exhaustive runs the device code itself on all
2^32 inputs; this test catches a bad coefficient without a GPU.

Accept rate (stated, and asserted as a floor): 369 073 320 of the 369 098 752 inputs with
2^-12 <= |x| < 2^10 are accepted, 0.999931 (the rest lie within 2^9 ulp of an fp32 rounding
boundary or have |r| < 2^-12); inputs below 2^-12 in magnitude always take the canonical path
(r = x), as do all inputs from 2^19 up. The Taylor form to r^19 that this polynomial replaces
accepts exactly as many below 2^10, and one input more of the 75 497 472 in [2^10, 2^19).
"""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkancomputeraytracing_amd", "csrc")

SOURCE = r"""
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>
#include "vcrt_math.h"

// the Horner steps after the first coefficient: kSinC's unused tail entries are zero
constexpr int SIN_STEPS = vcrt::kSinC[11] == 0.0 && vcrt::kSinC[12] == 0.0 ? 6 : 8;

// vcrt_math.h sin_fast_try, on the host: the same operations, constants from kSinC
static bool fast_try(float xf, float& out) {
    const double* c = vcrt::kSinC;
    const double x = (double)xf;
    const double t = __builtin_fma(x, c[0], c[1]);
    const double k = t - c[1];
    double r = __builtin_fma(-k, c[2], x);
    r = __builtin_fma(-k, c[3], r);
    const double r2 = r * r;
    double p = c[4];
    for (int j = 5; j < 5 + SIN_STEPS; ++j) p = __builtin_fma(p, r2, c[j]);
    const double s = __builtin_fma(r * r2, p, r);
    const uint64_t tb = __builtin_bit_cast(uint64_t, t);
    const uint64_t sb = __builtin_bit_cast(uint64_t, s) ^ (tb << 63);
    out = (float)__builtin_bit_cast(double, sb);
    const uint32_t below = (uint32_t)sb & 0x1FFFFFFFu;
    return __builtin_fabsf(xf) < 0x1p19f && __builtin_fabs(r) >= 0x1p-12 &&
           below - (0x10000000u - 0x200u) > 0x400u;
}

// bit patterns first, first + stride, ... (count of them): res[0] accepted, res[1] accepted
// with another float than sin_canonical's, res[2] the first such pattern
extern "C" void check(uint32_t first, uint64_t count, uint32_t stride, int threads,
                      unsigned long long* res) {
    std::atomic<unsigned long long> acc{0}, bad{0}, first_bad{~0ull};
    std::vector<std::thread> pool;
    for (int w = 0; w < threads; ++w)
        pool.emplace_back([&, w] {
            unsigned long long a = 0, b = 0, fb = ~0ull;
            const uint64_t lo = count * w / threads, hi = count * (w + 1) / threads;
            for (uint64_t i = lo; i < hi; ++i) {
                const uint32_t bits = first + (uint32_t)(i * stride);
                const float x = __builtin_bit_cast(float, bits);
                float f;
                if (!fast_try(x, f)) continue;
                ++a;
                if (__builtin_bit_cast(uint32_t, f) !=
                    __builtin_bit_cast(uint32_t, vcrt::sin_canonical(x))) {
                    ++b;
                    if (bits < fb) fb = bits;
                }
            }
            acc += a;
            bad += b;
            unsigned long long cur = first_bad.load();
            while (fb < cur && !first_bad.compare_exchange_weak(cur, fb)) {
            }
        });
    for (auto& t : pool) t.join();
    res[0] = acc;
    res[1] = bad;
    res[2] = first_bad;
}
"""


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    d = tmp_path_factory.mktemp("sin_poly")
    src, so = d / "sin_poly.cpp", d / "libsin_poly.so"
    src.write_text(SOURCE)
    flags = ["-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-ffp-contract=off",
             "-fno-fast-math", f"-I{CSRC}"]
    try:  # hardware FMA where the CPU has it (libm's fma gives the same values, slowly)
        if " fma " in open("/proc/cpuinfo").read():
            flags.append("-mfma")
    except OSError:
        pass
    subprocess.run(["g++", *flags, "-o", str(so), str(src)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.check.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                          ctypes.POINTER(ctypes.c_ulonglong)]
    lib.check.restype = None
    threads = max(1, min(16, len(os.sched_getaffinity(0))))

    def run(first, count, stride=1):
        res = (ctypes.c_ulonglong * 3)()
        lib.check(first, count, stride, threads, res)
        return res[0], res[1], res[2]
    return run


K10 = 0x44800000  # the bits of 2^10
K12M = 0x39800000  # the bits of 2^-12


def test_fast_sine_equals_canonical_below_2_10(mirror):
    """Every fp32 input with |x| < 2^10, both signs: an accepted value is the canonical float."""
    accepted = 0
    for sign in (0, 0x80000000):
        acc, bad, first = mirror(sign, K10)
        assert bad == 0, f"{bad} accepted values differ, first bit pattern {first:#010x}"
        accepted += acc
    rate = accepted / (2 * (K10 - K12M))
    print(f"accepted {accepted} of {2 * (K10 - K12M)} inputs with 2^-12 <= |x| < 2^10: {rate:.6f}")
    # |x| < 2^-12 is never accepted (r = x); above it the only rejections are the boundary
    # margin (2 * 2^9 / 2^29 = 2^-19 of uniformly spread mantissas) and |r| < 2^-12 around the
    # multiples of pi (2^-11 / pi of the arguments from 1 up): together under 2e-4 at this range
    assert rate > 0.9995


def test_fast_sine_equals_canonical_strided_rest(mirror):
    """2^24 evenly strided bit patterns of the other inputs (|x| >= 2^10, infinities, NaNs)."""
    for sign in (0, 0x80000000):
        rest = 0x80000000 - K10
        stride = rest // (1 << 23)
        acc, bad, first = mirror(sign + K10, 1 << 23, stride)
        assert bad == 0, f"{bad} accepted values differ, first bit pattern {first:#010x}"
        assert acc > 0  # 2^10 <= |x| < 2^19 is in the sample
