"""The big list's may-hit predicate by sign bits (tracer.hip big_roots, hit_sign) against the
float compares it replaces (may_hit), restated in numpy on uint32 / float32 words. No GPU.

 may_hit(hb, cc, disc)  = !(disc < 0) && (hb < 0 || cc < 0)
 hit_sign(hb, cc, disc) = sign bit of (bits(hb) | bits(cc)) & ~bits(disc)

What the kernel can hand the predicates, and so what the value sets hold:
 * hb: any float but NaN, -0 included (a dot product of finite terms).
 * cc = RN(s - r2) with s a sum of squares (>= +0) and r2 = RN(radius^2) >= +0, or -3e38 for a
   padding member: never -0 (x - y rounds to -0 only for x = -0, y = +0), never NaN.
 * disc = RN(RN(hb hb) - RN(a cc)) with a > 0: RN(hb hb) >= +0, so the difference is never -0
   either; finite on the guarded range (a padding member's may be -inf). It is a function of hb,
   cc and a: a free triple (hb, cc, disc) is wider than anything the kernel computes.
test_never_minus_zero evaluates those two expressions over the value set and finds no -0.

On the free triples the two predicates agree except where hb is -0: there hit_sign is set for cc
>= 0, disc >= 0 and may_hit is not. For those (hb, cc) and a in {2^-20, 1, 2^60} the kernel's own
disc = RN(hb hb - a cc) is either negative (both predicates false: no disagreement in the kernel)
or +0 (cc = 0, or a cc underflows), and then candidate_t's roots are 0 <= kMinT, which `consider`
rejects.

The gate: the new one, "some member's sign bit is set", implies the old one, !(max disc < 0);
where the old one passed and the new one does not, no member is may_hit.
"""
import itertools

import numpy as np

F = np.float32
K_MIN_T = F(0.001)
SIGN = np.uint32(0x80000000)


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def may_hit(hb, cc, disc):
    with np.errstate(invalid="ignore"):
        return ~(disc < F(0)) & ((hb < F(0)) | (cc < F(0)))


def hit_sign(hb, cc, disc):
    return (((bits(hb) | bits(cc)) & ~bits(disc)) & SIGN) != 0


def candidate_t(hb, disc, a):
    """tracer.hip candidate_t in fp32: every operation rounded to float32."""
    sq = np.sqrt(disc, dtype=F)
    r1 = F(F(-hb) - sq) / a
    r2 = F(F(-hb) + sq) / a
    return np.where(r1 > K_MIN_T, r1, r2).astype(F)


DENORMAL = np.array([1], np.uint32).view(F)[0]          # 2^-149
TINY = np.finfo(F).tiny                                  # 2^-126
LARGE = F(3.0e38)
MAGNITUDES = [F(0), DENORMAL, F(DENORMAL * 12345), TINY, F(1e-30), F(1), F(2 ** 63), LARGE,
              F(np.inf)]
SIGNED = np.array([s * m for m in MAGNITUDES for s in (F(1), F(-1))], F)  # holds +0 and -0
NO_MINUS_ZERO = SIGNED[bits(SIGNED) != SIGN]
A_VALUES = [F(2.0 ** -20), F(1), F(2.0 ** 60)]


def grid(hb_set, cc_set, disc_set):
    hb, cc, disc = np.meshgrid(hb_set, cc_set, disc_set, indexing="ij")
    return hb.ravel(), cc.ravel(), disc.ravel()


def random_words(rng, n, finite=False):
    """n random float32 bit patterns, NaNs left out (finite: infinities too)."""
    w = rng.integers(0, 2 ** 32, size=2 * n + 64, dtype=np.uint64).astype(np.uint32)
    e = (w >> np.uint32(23)) & np.uint32(0xFF)
    keep = (e != 0xFF) if finite else ~((e == 0xFF) & ((w & np.uint32(0x7FFFFF)) != 0))
    w = w[keep][:n]
    assert len(w) == n
    return w.view(F)


def check_triples(hb, cc, disc):
    old, new = may_hit(hb, cc, disc), hit_sign(hb, cc, disc)
    differ = old != new
    # the one exception: hb == -0, and only towards an extra candidate
    assert np.all(bits(hb)[differ] == SIGN)
    assert np.all(new[differ] & ~old[differ])
    assert np.all((cc[differ] >= 0) & (disc[differ] >= 0))
    return hb[differ], cc[differ]


def check_extra_candidates(hb, cc):
    """The disagreeing (hb, cc) with the kernel's own disc: rejected before or by `consider`."""
    assert np.all(bits(hb) == SIGN)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in A_VALUES:
            disc = (F(hb * hb) - (a * cc).astype(F)).astype(F)
            live = ~(disc < 0)
            # disc >= 0 with hb = -0 and cc >= 0 forces RN(a cc) = +0 (cc = 0, or a product
            # that underflows: cc < 2^-129 at a = 2^-20) and disc = +0
            assert np.all((a * cc[live]).astype(F) == 0) and np.all(bits(disc[live]) == 0)
            t = candidate_t(hb[live], disc[live], a)
            assert np.all(t <= K_MIN_T), (a, t[t > K_MIN_T][:4])


def test_value_set_agrees_but_for_minus_zero_hb():
    hb, cc, disc = grid(SIGNED, NO_MINUS_ZERO, NO_MINUS_ZERO)
    dh, dc = check_triples(hb, cc, disc)
    assert len(dh) > 0  # the exception is in the set
    check_extra_candidates(dh, dc)
    # without hb = -0: no exception at all
    hb, cc, disc = grid(NO_MINUS_ZERO, NO_MINUS_ZERO, NO_MINUS_ZERO)
    assert np.array_equal(may_hit(hb, cc, disc), hit_sign(hb, cc, disc))


def test_random_bit_patterns_agree():
    rng = np.random.default_rng(13)
    n = 4_000_000
    hb, cc, disc = random_words(rng, n), random_words(rng, n), random_words(rng, n, finite=True)
    cc = np.where(bits(cc) == SIGN, F(0), cc)        # never -0 (module docstring)
    disc = np.where(bits(disc) == SIGN, F(0), disc)
    hb[: n // 64] = F(-0.0)                           # the exception, often
    dh, dc = check_triples(hb, cc, disc)
    assert len(dh) > 0
    check_extra_candidates(dh, dc)
    rest = bits(hb) != SIGN
    assert np.array_equal(may_hit(hb, cc, disc)[rest], hit_sign(hb, cc, disc)[rest])


def test_never_minus_zero():
    """cc = RN(s - r2) and disc = RN(RN(hb hb) - RN(a cc)) over the value set: no -0 word."""
    s = NO_MINUS_ZERO[NO_MINUS_ZERO >= 0]
    r2 = np.concatenate([s[np.isfinite(s)], [F(-3.0e38)]]).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        cc = (s[:, None] - r2[None, :]).astype(F).ravel()
        cc = cc[~np.isnan(cc)]
        assert not np.any(bits(cc) == SIGN)
        for a in A_VALUES:
            hb2 = (SIGNED * SIGNED).astype(F)
            disc = (hb2[:, None] - (a * cc).astype(F)[None, :]).astype(F).ravel()
            assert not np.any(bits(disc[~np.isnan(disc)]) == SIGN)


def gates(hb, cc, disc):
    """(old gate, new gate, any member may_hit) over groups of four members (last axis)."""
    with np.errstate(invalid="ignore"):
        old = ~(np.max(disc, axis=-1) < F(0))
    return old, hit_sign(hb, cc, disc).any(axis=-1), may_hit(hb, cc, disc).any(axis=-1)


def check_gates(hb, cc, disc):
    old, new, any_old = gates(hb, cc, disc)
    assert np.all(old[new])                 # the new gate implies the old one
    assert not np.any(any_old[old & ~new])  # what the tighter gate skips held no candidate
    assert np.all(new[any_old])             # and it never skips one
    return int((old & ~new).sum())


def test_gate():
    rng = np.random.default_rng(14)
    n = 1_000_000
    shape = (n, 4)
    hb = random_words(rng, 4 * n).reshape(shape)
    cc = random_words(rng, 4 * n).reshape(shape)
    disc = random_words(rng, 4 * n, finite=True).reshape(shape)
    cc = np.where(bits(cc) == SIGN, F(0), cc)
    disc = np.where(bits(disc) == SIGN, F(0), disc)
    hb[: n // 16, 0] = F(-0.0)
    # the missing second pair's defaults: hb = cc = 0, disc = -1
    hb[n // 2:, 2:], cc[n // 2:, 2:], disc[n // 2:, 2:] = F(0), F(0), F(-1)
    assert check_gates(hb, cc, disc) > 0    # the gate is strictly tighter somewhere
    # the value set, four members at a time
    vals = list(itertools.product(SIGNED[::3], NO_MINUS_ZERO[::3], NO_MINUS_ZERO[::2]))
    members = np.array(vals, F)
    idx = rng.integers(0, len(members), size=(200_000, 4))
    quad = members[idx]
    check_gates(quad[..., 0], quad[..., 1], quad[..., 2])
    # a group with no second pair never passes on the defaults alone
    d = np.array([[F(0), F(0), F(-1)]] * 4, F)[None]
    assert not gates(d[..., 0], d[..., 1], d[..., 2])[1][0]
