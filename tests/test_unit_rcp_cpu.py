"""The scatter's unit vector with one reciprocal (tracer.hip unit_of) on the CPU: a C mirror of
recip_a / div_a with fmaf, of sqrt's use and of unit_guard's integer tests, against the IEEE
division the kernel ran before (ru / sqrtf(dot(ru, ru)), every operation rounded on its own).

The device's v_rcp_f32 is accurate to one ulp, not correctly rounded, so the mirror runs every
quotient three times: with y0 = 1 / len moved by -1, 0 and +1 ulp before its Newton step. Inside
the guard (every component 0 or >= 2^-40, len in [2^-20, 2]) all three must give the bits of
x / len; outside it the mirror takes the full division, whatever the operands are.

Inputs: 2^24 random triples (uniform rand() values, a share of them scaled down to 2^-45 and with
zeros put in) and the edges: zeros in each position, 1.0, 2^-40, a length just above 2^-20, three
equal components; and out of range a numerator of 2^-110, a length of 2^-30 and the all-zero
triple (0 / 0: NaN in the reference form).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

SOURCE = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* tracer.hip recip_a, the hardware reciprocal standing `ulps` away from the rounded 1 / a */
static float recip_a(float a, int ulps) {
    const float y0 = float_of(bits_of(1.0f / a) + (uint32_t)ulps);
    return fmaf(fmaf(-a, y0, 1.0f), y0, y0);
}

static float div_a(float x, float a, float ya) {
    const float q0 = x * ya;
    const float q1 = fmaf(fmaf(-a, q0, x), ya, q0);
    return fmaf(fmaf(-a, q1, x), ya, q1);
}

/* tracer.hip unit_guard */
static int unit_guard(const float* ru, float len) {
    const uint32_t bx = bits_of(ru[0]) - 1u, by = bits_of(ru[1]) - 1u, bz = bits_of(ru[2]) - 1u;
    uint32_t m = bx < by ? bx : by;
    m = m < bz ? m : bz;
    return m >= 0x2B800000u - 1u && bits_of(len) - 0x35800000u <= 0x0A800000u;
}

/* unit_of on n triples: out[i] as the helper gives it (reciprocal moved by `ulps`), inside[i] the
   guard. Returns the number of components whose bits differ from x / len. */
uint64_t unit_check(const float* in, uint64_t n, int ulps, float* out, uint8_t* inside) {
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float* ru = in + 3 * i;
        const float dd = ru[0] * ru[0] + ru[1] * ru[1] + ru[2] * ru[2];
        const float len = sqrtf(dd);
        const int g = unit_guard(ru, len);
        const float ya = recip_a(len, ulps);
        for (int k = 0; k < 3; ++k) {
            const float full = ru[k] / len;
            const float u = g ? div_a(ru[k], len, ya) : full;
            bad += bits_of(u) != bits_of(full);
            if (out) out[3 * i + k] = u;
        }
        if (inside) inside[i] = (uint8_t)g;
    }
    return bad;
}
"""

P40, P20 = np.float32(2.0 ** -40), np.float32(2.0 ** -20)
EDGES_IN = np.array([
    [0, 0.5, 0.25], [0.5, 0, 0.25], [0.5, 0.25, 0], [0, 0, 0.75], [0, 0.75, 0], [0.75, 0, 0],
    [1, 1, 1], [1, 0, 0], [0, 0, 1], [1, 0.5, 0],
    [P40, 0.5, 0.25], [0.5, P40, 0.25], [0.5, 0.25, P40], [P40, P40, 1],
    [P20 * np.float32(1.0000002), 0, 0], [0, P20, P40], [P20, P20, 0],   # len just above 2^-20
    [0.3, 0.3, 0.3], [1 / 3, 1 / 3, 1 / 3], [P20, P20, P20], [0.999, 0.999, 0.999],
], dtype=np.float32)
EDGES_OUT = np.array([
    [2.0 ** -110, 0.5, 0.25],        # a nonzero numerator below 2^-40
    [0.5, 2.0 ** -41, 0.25],
    [2.0 ** -30, 0, 0],              # len = 2^-30
    [P20 * np.float32(0.99), 0, 0],  # len just below 2^-20
    [0, 0, 0],                       # 0 / 0: NaN
    [np.nan, 0.5, 0.5], [np.inf, 0.5, 0.5], [1.5, 1.5, 1.5],  # len NaN, inf, above 2
], dtype=np.float32)


def edges():
    """The edge triples and whether each lies inside the guard (tests/test_gpu_shading_trim.py
    feeds the same ones to the device)."""
    return (np.concatenate([EDGES_IN, EDGES_OUT]),
            np.array([True] * len(EDGES_IN) + [False] * len(EDGES_OUT)))


def random_triples(n, seed=15):
    """Uniform rand() values; every fourth triple scaled by 2^-e, e up to 45, in one to three
    components; every eighth with a zero put in."""
    rng = np.random.default_rng(seed)
    t = rng.random((n, 3), dtype=np.float32)
    small = np.arange(n) % 4 == 1
    scale = np.ldexp(np.float32(1), -rng.integers(0, 46, size=(n, 3))).astype(np.float32)
    keep = rng.random((n, 3)) < 0.5
    t[small] = (t * np.where(keep, np.float32(1), scale))[small]
    zero = np.arange(n) % 8 == 3
    z = rng.integers(0, 3, size=n)
    t[zero, z[zero]] = 0
    return np.ascontiguousarray(t)


def same_bits(a, b):
    """Equal bit for bit, NaNs equal to each other (their sign and payload are the platform's)."""
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def reference(t):
    """ru / sqrt(dot(ru, ru)) in numpy float32: correctly rounded operations, GLSL dot's order."""
    with np.errstate(all="ignore"):
        dd = t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1] + t[:, 2] * t[:, 2]
        return t / np.sqrt(dd)[:, None]


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    d = tmp_path_factory.mktemp("unit_rcp")
    src, so = d / "unit_rcp.c", d / "libunit_rcp.so"
    src.write_text(SOURCE)
    flags = ["-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"]
    try:  # hardware FMA where the CPU has it (libm's fmaf gives the same values, slowly)
        if " fma " in open("/proc/cpuinfo").read():
            flags.append("-mfma")
    except OSError:
        pass
    subprocess.run(["gcc", *flags, "-o", str(so), str(src), "-lm"], check=True)
    lib = ctypes.CDLL(str(so))
    lib.unit_check.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p,
                               ctypes.c_void_p]
    lib.unit_check.restype = ctypes.c_uint64

    def run(t, ulps, want_out=False):
        t = np.ascontiguousarray(t, dtype=np.float32)
        out = np.empty_like(t) if want_out else None
        inside = np.empty(len(t), dtype=np.uint8)
        bad = lib.unit_check(t.ctypes.data, len(t), ulps, out.ctypes.data if want_out else None,
                             inside.ctypes.data)
        return bad, out, inside.astype(bool)
    return run


@pytest.fixture(scope="module")
def triples():
    return random_triples(1 << 24)


@pytest.mark.parametrize("ulps", [-1, 0, 1])
def test_random_triples(mirror, triples, ulps):
    t = triples
    bad, _, inside = mirror(t, ulps)
    print(f"reciprocal {ulps:+d} ulp: {inside.sum()} of {len(t)} triples inside the guard, "
          f"{bad} quotients differ")
    assert bad == 0
    assert inside.sum() > len(t) * 3 // 4 and (~inside).sum() > len(t) // 100


@pytest.mark.parametrize("ulps", [-1, 0, 1])
def test_edges(mirror, ulps):
    t, want_inside = edges()
    bad, out, inside = mirror(t, ulps, want_out=True)
    assert bad == 0
    assert inside.tolist() == want_inside.tolist()
    assert same_bits(out, reference(t))
    zeros = t == 0
    assert np.all(out[zeros & inside[:, None]].view(np.uint32) == 0)  # +0, not -0
    assert np.all(np.isnan(out[t.sum(axis=1) == 0]))                  # 0 / 0 by the full division


def test_mirror_reference_agree_on_the_sample(mirror):
    """numpy's float32 sqrt and division (the GPU test's reference) against the mirror's x / len."""
    t = random_triples(1 << 16, seed=16)
    bad, out, _ = mirror(t, 0, want_out=True)
    assert bad == 0
    assert same_bits(out, reference(t))
