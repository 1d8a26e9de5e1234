"""Adaptive sampling without a GPU: the count rule of vcrt_sample_counts_host against its numpy
restatement (tests/adaptive_ref.sample_counts), bit for bit, and every argument error of
vcrt_draw_samples and vcrt_sample_counts that is checked before the renderer's state."""
import ctypes

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import adaptive_ref as AR

N = vc._native
F = np.float32
FORMAT, INIT = N.VK_ERROR_FORMAT_NOT_SUPPORTED, N.VK_ERROR_INITIALIZATION_FAILED


def params(target=0.1, min_count=0, max_count=64, size=None):
    p = N.vcrt_sample_count_params()
    p.struct_size = ctypes.sizeof(N.vcrt_sample_count_params) if size is None else size
    p.target, p.min_count, p.max_count = target, min_count, max_count
    return p


def edge_plane(target, max_count):
    """Variances around every decision of the rule for (target, max_count): 0, -0, negatives, NaN,
    both infinities, denormals, values whose t lands exactly on an integer and its fp32
    neighbours, t at, just below and above max_count, and a seeded spread."""
    k = F(1.0) / F(F(target) * F(target))
    exact = []
    for c in range(0, max_count + 2):
        v = F(F(c) / k)
        exact += [v, np.nextafter(v, F(-np.inf)), np.nextafter(v, F(np.inf))]
    rng = np.random.default_rng(20261021)
    spread = (rng.uniform(0, 1, 500) ** 4 * (max_count + 3) / float(k)).astype(F)
    special = [0.0, -0.0, -1.0, -1e30, np.nan, -np.nan, np.inf, -np.inf, 1e-45, 1e-38, 3.4e38]
    return np.concatenate([np.array(special, F), np.array(exact, F), spread]).astype(F)


@pytest.mark.parametrize("target,lo,hi", [(0.1, 0, 64), (0.05, 1, 256), (1.0, 3, 3), (0.3, 0, 9),
                                          (7.5e-3, 2, 255), (16.0, 0, 1)])
def test_count_rule_matches_numpy(target, lo, hi):
    v = edge_plane(target, hi)
    want, total = AR.sample_counts(v, target, lo, hi)
    got, got_total = vc.sample_counts_host(v, target, lo, hi, stats=True)
    assert got.dtype == np.uint16 and got.shape == v.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:6]]
    assert got_total == total
    assert got.min() >= lo and got.max() <= hi
    # the specials: 0, -0, negatives and NaN count nothing; +inf takes max_count
    assert (got[:6] == lo).all() and got[6] == hi and got[7] == lo


def test_count_rule_keeps_the_shape():
    v = np.linspace(0, 1, 44 * 20, dtype=F).reshape(20, 44)
    got = vc.sample_counts_host(v, 0.125, 0, 64)
    assert got.shape == (20, 44)
    assert np.array_equal(got, AR.sample_counts(v, 0.125, 0, 64)[0])
    # t exactly an integer is that integer: 1 / 0.125^2 = 64 exactly
    exact = np.array([0.25, 0.5, 1 / 64, 1.0], F)
    assert vc.sample_counts_host(exact, 0.125, 0, 64).tolist() == [16, 32, 1, 64]


def test_sample_counts_argument_errors():
    lib = N.lib()
    v = np.zeros(8, F)
    c = np.zeros(8, np.uint16)
    st = N.vcrt_sample_count_stats()
    for name in ("vcrt_sample_counts_host", "vcrt_sample_counts", "vcrt_sample_counts_device"):
        fn = getattr(lib, name)

        def call(p, var=v.ctypes.data, n=8, out=c.ctypes.data):
            return fn(var, n, ctypes.byref(p) if p is not None else None, out, ctypes.byref(st))

        assert call(params(size=12)) == FORMAT, name
        for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):
            assert call(params(target=bad)) == FORMAT, (name, bad)
        assert call(params(min_count=5, max_count=4)) == FORMAT, name
        assert call(params(max_count=257)) == FORMAT, name
        assert call(params(), n=0) == FORMAT, name
        assert call(None) == INIT, name
        assert call(params(), var=None) == INIT, name
        assert call(params(), out=None) == INIT, name
        assert call(params(), out=v.ctypes.data) == INIT, name
    # the GPU forms need a renderer; the host form runs
    assert lib.vcrt_sample_counts(v.ctypes.data, 8, ctypes.byref(params()), c.ctypes.data,
                                  None) == INIT
    assert lib.vcrt_sample_counts_host(v.ctypes.data, 8, ctypes.byref(params()), c.ctypes.data,
                                       None) == N.VK_SUCCESS


def test_sample_counts_python_errors():
    v = np.zeros(8, F)
    for kw in (dict(target=0), dict(target=float("nan")), dict(target=0.1, min_count=-1),
               dict(target=0.1, min_count=9, max_count=8), dict(target=0.1, max_count=257),
               dict(target="x")):
        with pytest.raises(ValueError):
            vc.sample_counts_host(v, **kw)
    with pytest.raises(ValueError):
        vc.sample_counts_host(np.zeros(0, F), 0.1)


def test_draw_samples_argument_errors_before_begin():
    lib = N.lib()
    c = np.zeros(8, np.uint16)
    s = np.zeros((8, 4), F)
    st = N.vcrt_sample_stats()
    for name in ("vcrt_draw_samples", "vcrt_draw_samples_device"):
        fn = getattr(lib, name)
        for first, max_count in ((0, 0), (0, 257), (0, 1 << 20), ((1 << 19) - 255, 256),
                                 (1 << 19, 1), (0xFFFFFFFF, 1)):
            assert fn(first, max_count, c.ctypes.data, 0, s.ctypes.data, None,
                      ctypes.byref(st)) == FORMAT, (name, first, max_count)
        # valid ranges reach the renderer's state: there is none
        for first, max_count in ((0, 1), (0, 256), ((1 << 19) - 256, 256)):
            assert fn(first, max_count, c.ctypes.data, 0, s.ctypes.data, None,
                      ctypes.byref(st)) == INIT, (name, first, max_count)
        assert fn(0, 4, None, 0, s.ctypes.data, None, None) == INIT, name
        assert fn(0, 4, c.ctypes.data, 0, None, None, None) == INIT, name
        assert fn(0, 4, c.ctypes.data, 0, s.ctypes.data, s.ctypes.data, None) == INIT, name
        # the range is judged first, whatever the planes are
        assert fn(0, 0, None, 0, None, None, None) == FORMAT, name
