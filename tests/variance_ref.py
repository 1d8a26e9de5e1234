"""Variance-guided denoising restated for the tests (no tests here): include/vcrt.h
vcrt_reproject_moments, vcrt_variance and vcrt_denoise_variance in numpy float32, vectorised over
the pixels, one rounded operation per statement, the taps in the stated order; and the generated
planes the CPU and GPU tests share. It shares no code with csrc/variance.cpp or csrc/variance.hip;
both must reproduce it bit for bit."""
import numpy as np

from tests import denoise_ref as D
from tests import reproject_ref as P

F = np.float32
EPS = F(2.0 ** -10)        # the demodulation's floor on the albedo
DEPTH_EPS = F(2.0 ** -20)  # the relative depth's denominator never vanishes
VAR_EPS = F(2.0 ** -20)    # kv's denominator never vanishes
K5 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
K3 = [F(1 / 4), F(1 / 2), F(1 / 4)]
LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)

SHAPES = [(44, 20), (70, 5), (100, 37), (3, 2), (1, 1)]
# vcrt_reproject's sets, each with an alpha_moments on another side of 1 / N
MOMENTS_SETS = {name: dict(p, alpha_moments=am) for (name, p), am in
                zip(P.PARAM_SETS.items(), (0.2, 0.05, 0.5, 1.0, 0.3))}
# min_history on both sides of the generated lengths, and its two ends
VARIANCE_SETS = {
    "svgf": dict(min_history=4.0, alpha=0.2),
    "all-temporal": dict(min_history=1.0, alpha=0.6),
    "all-spatial": dict(min_history=65535.0, alpha=0.05),
    "alpha-one": dict(min_history=2.0, alpha=1.0),
}
# each term alone with the colour term, the colour term alone, none, all, and the pass counts' ends
DENOISE_SETS = {
    "normal": dict(levels=3, sigma_normal=0.5, sigma_depth=0, sigma_albedo=0, sigma_colour=0),
    "depth": dict(levels=3, sigma_normal=0, sigma_depth=0.1, sigma_albedo=0, sigma_colour=0),
    "albedo": dict(levels=3, sigma_normal=0, sigma_depth=0, sigma_albedo=0.25, sigma_colour=0),
    "colour": dict(levels=3, sigma_normal=0, sigma_depth=0, sigma_albedo=0, sigma_colour=4.0),
    "none": dict(levels=2, sigma_normal=0, sigma_depth=0, sigma_albedo=0, sigma_colour=0),
    "all": dict(levels=5, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=0.25, sigma_colour=4.0),
    "all-1": dict(levels=1, sigma_normal=0.7, sigma_depth=0.2, sigma_albedo=0.5, sigma_colour=1.5),
    "all-8": dict(levels=8, sigma_normal=0.7, sigma_depth=0.2, sigma_albedo=0.5, sigma_colour=9.0),
}

_cache = {}


def lum(v):
    """(0.2126 r + 0.7152 g) + 0.0722 b of [..., >= 3]."""
    y = LR * v[..., 0] + LG * v[..., 1]
    return y + LB * v[..., 2]


def _demodulated(colour, albedo):
    if albedo is None:
        return colour[..., :3].copy()
    return colour[..., :3] / np.fmax(albedo[..., :3], EPS)


def reproject_moments(colour, motion, hcol, hsurf, hlen, albedo, hmom, alpha, max_history,
                      depth_tolerance, alpha_moments):
    """(out [H, W, 4], out_length [H, W], out_moments [H, W, 4], accepted [H, W] bool)."""
    colour, motion = np.asarray(colour, F), np.asarray(motion, F)
    hcol, hsurf, hlen = np.asarray(hcol, F), np.asarray(hsurf, F), np.asarray(hlen, F)
    hmom = np.asarray(hmom, F)
    H, W = colour.shape[:2]
    alpha, cap, tol, am0 = F(alpha), F(max_history), F(depth_tolerance), F(alpha_moments)
    mx, my, mz, mw = (motion[..., k] for k in range(4))
    with np.errstate(all="ignore"):
        s = _demodulated(colour, None if albedo is None else np.asarray(albedo, F))
        Y = lum(s)
        Y2 = Y * Y
        valid = (mw >= 1) & (mx > -1) & (mx < F(W)) & (my > -1) & (my < F(H))
        sx, sy = np.where(valid, mx, F(0)), np.where(valid, my, F(0))
        fx, fy = np.floor(sx), np.floor(sy)
        ax, ay = sx - fx, sy - fy
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        acc = np.zeros((H, W, 3), F)
        lsum, wsum = np.zeros((H, W), F), np.zeros((H, W), F)
        m1, m2 = np.zeros((H, W), F), np.zeros((H, W), F)
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            bx = ax if dx else F(1) - ax
            by = ay if dy else F(1) - ay
            b = bx * by
            qx, qy = ix + dx, iy + dy
            inside = valid & (b != 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)  # (read only where inside)
            key, zq, lq = hsurf[cy, cx, 0], hsurf[cy, cx, 1], hlen[cy, cx]
            num = np.abs(mz - zq)
            den = np.abs(mz) + np.abs(zq)
            den = den + DEPTH_EPS
            depth_ok = (mw == 1) | (tol == 0) | (num / den <= tol)
            take = inside & (key == mw) & (lq >= 1) & depth_ok
            acc = np.where(take[..., None], acc + b[..., None] * hcol[cy, cx, :3], acc)
            lsum = np.where(take, lsum + b * lq, lsum)
            wsum = np.where(take, wsum + b, wsum)
            m1 = np.where(take, m1 + b * hmom[cy, cx, 0], m1)
            m2 = np.where(take, m2 + b * hmom[cy, cx, 1], m2)
        took = wsum > 0
        safe = np.where(took, wsum, F(1))
        h3 = acc / safe[..., None]
        L = lsum / safe
        N = np.where(took, np.minimum(L + F(1), cap), F(1)).astype(F)
        rn = F(1) / N
        a = np.maximum(alpha, rn)
        blend = h3 + a[..., None] * (colour[..., :3] - h3)
        h1, h2 = m1 / safe, m2 / safe
        am = np.maximum(am0, rn)
        M1 = np.where(took, h1 + am * (Y - h1), Y)
        M2 = np.where(took, h2 + am * (Y2 - h2), Y2)
        out = colour.copy()
        out[..., :3] = np.where(took[..., None], blend, colour[..., :3])
        mom = np.stack([M1, M2, np.fmax(M2 - M1 * M1, F(0)), N], axis=-1)
    assert out.dtype == F and mom.dtype == F and N.dtype == F
    return out, N, mom, took


def variance(moments, surface, min_history, alpha):
    """(variance [H, W], spatial [H, W] bool): the definition."""
    moments, surface = np.asarray(moments, F), np.asarray(surface, F)
    H, W = moments.shape[:2]
    mh, alpha = F(min_history), F(alpha)
    with np.errstate(all="ignore"):
        N = np.fmax(moments[..., 3], F(1))
        spatial = ~(moments[..., 3] >= mh)
        key = surface[..., 0]
        S1, S2, n = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in range(-3, 4):
            y0, y1 = max(0, -dy), min(H, H - dy)
            if y0 >= y1:
                continue
            for dx in range(-3, 4):
                x0, x1 = max(0, -dx), min(W, W - dx)
                if x0 >= x1:
                    continue
                Pp = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                counts = (key[Q] == key[Pp]) if (dx, dy) != (0, 0) else True
                S1[Pp] = np.where(counts, S1[Pp] + moments[Q][..., 0], S1[Pp])
                S2[Pp] = np.where(counts, S2[Pp] + moments[Q][..., 1], S2[Pp])
                n[Pp] = np.where(counts, n[Pp] + F(1), n[Pp])
        a1, a2 = S1 / n, S2 / n
        sv = np.fmax(a2 - a1 * a1, F(0))
        boost = mh / N
        v = np.where(spatial, sv * boost, moments[..., 2])
        rn = F(1) / N
        out = v * np.fmax(alpha, rn)
    assert out.dtype == F
    return out, spatial


def denoise_variance(colour, albedo, normal_depth, var, *, levels, sigma_normal, sigma_depth,
                     sigma_albedo, sigma_colour, demodulate):
    """(out [H, W, 4], out_variance [H, W]): the definition."""
    colour, var = np.asarray(colour, F), np.asarray(var, F)
    H, W = colour.shape[:2]
    k_n, k_z, k_a = (D.scale(s) for s in (sigma_normal, sigma_depth, sigma_albedo))
    on_n = normal_depth is not None and k_n != 0
    on_z = normal_depth is not None and k_z != 0
    on_a = albedo is not None and k_a != 0
    on_c = F(sigma_colour) != 0
    sc2 = F(F(sigma_colour) * F(sigma_colour))
    demod = bool(demodulate) and albedo is not None
    with np.errstate(all="ignore"):
        s = _demodulated(colour, albedo if demod else None)
        v = np.fmax(var, F(0))
        for level in range(levels):
            step = 1 << level
            kv = yl = None
            if on_c:
                gsum, gw = np.zeros((H, W), F), np.zeros((H, W), F)
                for dy in range(-1, 2):
                    y0, y1 = max(0, -dy), min(H, H - dy)
                    if y0 >= y1:
                        continue
                    for dx in range(-1, 2):
                        x0, x1 = max(0, -dx), min(W, W - dx)
                        if x0 >= x1:
                            continue
                        Pp = (slice(y0, y1), slice(x0, x1))
                        Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                        h3 = K3[dx + 1] * K3[dy + 1]
                        gsum[Pp] = gsum[Pp] + h3 * v[Q]
                        gw[Pp] = gw[Pp] + h3
                g = gsum / gw
                den = sc2 * g
                den = den + VAR_EPS
                kv = F(1) / den
                yl = lum(s)
            acc = np.zeros((H, W, 3), F)
            wsum, vacc = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in range(-2, 3):
                oy = step * dy
                y0, y1 = max(0, -oy), min(H, H - oy)
                if y0 >= y1:
                    continue
                for dx in range(-2, 3):
                    ox = step * dx
                    x0, x1 = max(0, -ox), min(W, W - ox)
                    if x0 >= x1:
                        continue
                    Pp = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    h = K5[dx + 2] * K5[dy + 2]
                    X = np.zeros((y1 - y0, x1 - x0), F)
                    if on_n:
                        X = D._sum_sq(normal_depth[Pp], normal_depth[Q], 3) * k_n
                    tz = F(0)
                    if on_z:
                        zp, zq = normal_depth[Pp][..., 3], normal_depth[Q][..., 3]
                        num = zp - zq
                        den = np.abs(zp) + np.abs(zq)
                        den = den + DEPTH_EPS
                        rz = num / den
                        tz = (rz * rz) * k_z
                    X = X + tz
                    ta = F(0)
                    if on_a:
                        ta = D._sum_sq(albedo[Pp], albedo[Q], 4) * k_a
                    X = X + ta
                    tl = F(0)
                    if on_c:
                        dl = yl[Pp] - yl[Q]
                        tl = (dl * dl) * kv[Pp]
                    X = X + tl
                    e = F(1) - np.fmin(X, F(1))
                    w = h * (e * e)
                    acc[Pp] = acc[Pp] + w[..., None] * s[Q]
                    wsum[Pp] = wsum[Pp] + w
                    vacc[Pp] = vacc[Pp] + (w * w) * v[Q]
            s = acc / wsum[..., None]
            v = vacc / (wsum * wsum)
        out = np.empty((H, W, 4), F)
        out[..., :3] = s * np.fmax(albedo[..., :3], EPS) if demod else s
        out[..., 3] = colour[..., 3]
    assert out.dtype == F and v.dtype == F
    return out, v


def planes(w, h):
    """The generated planes of a shape, made once, read-only, as a dict: reproject_ref's five
    (blocks of surfaces with a block of sky, key 1; lengths 0 .. 65535, so on both sides of any
    min_history), denoise_ref's albedo (at and below eps) and normal_depth, `hmom` history
    moments, `moments` an out_moments-like plane whose lengths lie on both sides of 4,
    `surface` this frame's keys, and `var` a variance plane of 0, tiny, large and negative
    values."""
    if (w, h) in _cache:
        return _cache[(w, h)]
    colour, motion, hcol, hsurf, hlen = P.planes(w, h)
    _, albedo, nd = D.planes(w, h)
    rng = np.random.default_rng(77000 + 1000 * w + h)
    hm1 = rng.uniform(0.0, 2.0, (h, w)).astype(F)
    hmom = np.zeros((h, w, 4), F)
    hmom[..., 0] = hm1
    hmom[..., 1] = (hm1 * hm1 + rng.uniform(0.0, 0.5, (h, w))).astype(F)
    hmom[..., 2:] = rng.uniform(-1, 1, (h, w, 2))  # not read
    m1 = rng.uniform(0.0, 2.0, (h, w)).astype(F)
    moments = np.zeros((h, w, 4), F)
    moments[..., 0] = m1
    moments[..., 1] = (m1 * m1 + rng.uniform(-0.01, 0.5, (h, w))).astype(F)
    moments[..., 2] = np.fmax(moments[..., 1] - m1 * m1, F(0))
    moments[..., 3] = rng.choice(np.asarray([1, 1, 2, 3, 3.5, 4, 5, 31, 32], F), (h, w))
    surface = np.array(hsurf)
    var = rng.choice(np.asarray([0, 0, 1e-12, 1e-4, 0.01, 0.3, 2.0, 1e6, -0.5], F),
                     (h, w)).astype(F)
    var = (var * rng.uniform(0.5, 1.0, (h, w))).astype(F)
    out = dict(colour=colour, motion=motion, hcol=hcol, hsurf=hsurf, hlen=hlen, albedo=albedo,
               nd=nd, hmom=hmom, moments=moments, surface=surface, var=var)
    for a in out.values():
        assert np.isfinite(a).all() or a is motion
        a.setflags(write=False)
    _cache[(w, h)] = out
    return out


def _frozen(key, make):
    if key not in _cache:
        out = make()
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def moments_reference(w, h, name, with_albedo=True):
    p = planes(w, h)
    return _frozen(("m", w, h, name, with_albedo), lambda: reproject_moments(
        p["colour"], p["motion"], p["hcol"], p["hsurf"], p["hlen"],
        p["albedo"] if with_albedo else None, p["hmom"], **MOMENTS_SETS[name]))


def variance_reference(w, h, name):
    p = planes(w, h)
    return _frozen(("v", w, h, name), lambda: variance(p["moments"], p["surface"],
                                                       **VARIANCE_SETS[name]))


def denoise_reference(w, h, name, demodulate=1, with_albedo=True, with_guides=True):
    p = planes(w, h)
    return _frozen(("d", w, h, name, demodulate, with_albedo, with_guides),
                   lambda: denoise_variance(p["colour"], p["albedo"] if with_albedo else None,
                                            p["nd"] if with_guides else None, p["var"],
                                            demodulate=demodulate, **DENOISE_SETS[name]))
