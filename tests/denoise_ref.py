"""The denoiser's definition (include/vcrt.h vcrt_denoise) restated in numpy float32: the
edge-avoiding a-trous filter, one rounded operation per line, vectorised over the pixels and
looping over the passes and the 25 taps in the stated order (dy outer, dx inner, ascending). It
shares no code with csrc/denoise.cpp or csrc/denoise.hip; both must reproduce it bit for bit."""
import numpy as np

F = np.float32
EPS = F(2.0 ** -10)        # the demodulation's floor on the albedo
DEPTH_EPS = F(2.0 ** -20)  # the relative depth's denominator never vanishes
K5 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
# vcrt_default_denoise_params: the choice recorded in profiles/denoise_defaults.json
DEFAULTS = dict(levels=5, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.125,
                sigma_colour=0.75, demodulate=1)


# (width, height): 44 x 20 has both edges partial against any workgroup shape; at 3 x 2 with five
# levels every off-centre tap of the later passes is outside the frame; 1 x 1; 70 x 5 is wider
# than a wave's row segment and two workgroups of the LDS kernel wide
SHAPES = [(44, 20), (3, 2), (1, 1), (70, 5)]
# each term alone, none (the plain a-trous blur), all together, and the pass counts' two ends
PARAM_SETS = {
    "normal": dict(levels=3, sigma_normal=0.5, sigma_depth=0, sigma_albedo=0, sigma_colour=0),
    "depth": dict(levels=3, sigma_normal=0, sigma_depth=0.1, sigma_albedo=0, sigma_colour=0),
    "albedo": dict(levels=3, sigma_normal=0, sigma_depth=0, sigma_albedo=0.25, sigma_colour=0),
    "colour": dict(levels=3, sigma_normal=0, sigma_depth=0, sigma_albedo=0, sigma_colour=2.0),
    "none": dict(levels=2, sigma_normal=0, sigma_depth=0, sigma_albedo=0, sigma_colour=0),
    "all": dict(levels=5, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=0.25, sigma_colour=3.0),
    "all-1": dict(levels=1, sigma_normal=0.7, sigma_depth=0.2, sigma_albedo=0.5, sigma_colour=1.5),
    "all-8": dict(levels=8, sigma_normal=0.7, sigma_depth=0.2, sigma_albedo=0.5, sigma_colour=9.0),
}
_planes = {}


def planes(width, height):
    """Seeded finite test planes (colour, albedo, normal_depth), float32 [H, W, 4], read-only:
    6 x 6 blocks of constant guides plus a little noise, so that the edge-stopping weights take
    values all over [0, 1]; a block of sky (depth and coverage 0), albedo channels at and below
    the demodulation's floor, and a random alpha."""
    if (width, height) not in _planes:
        rng = np.random.default_rng(1000 * width + height)
        by, bx = (height + 5) // 6, (width + 5) // 6

        def blocks(channels, lo, hi, noise):
            b = rng.uniform(lo, hi, (by, bx, channels))
            full = np.repeat(np.repeat(b, 6, axis=0), 6, axis=1)[:height, :width]
            return (full + rng.normal(0, noise, full.shape)).astype(F)

        albedo = np.clip(blocks(4, 0.05, 1.0, 0.03), 0, 1).astype(F)
        nd = blocks(4, -1.0, 1.0, 0.05)
        nd[..., 3] = blocks(1, 1.0, 9.0, 0.02)[..., 0]
        sky = rng.random((by, bx)) < 0.25
        sky = np.repeat(np.repeat(sky, 6, axis=0), 6, axis=1)[:height, :width]
        nd[sky] = 0
        albedo[sky, 3] = 0
        albedo[rng.random((height, width)) < 0.05, 0] = 0          # below the floor
        albedo[rng.random((height, width)) < 0.05, 1] = F(2.0 ** -10)  # at it
        colour = (albedo * blocks(4, 0.2, 1.5, 0.0) + rng.normal(0, 0.15, albedo.shape)).astype(F)
        colour[..., 3] = rng.random((height, width)).astype(F)
        for p in (colour, albedo, nd):
            assert np.isfinite(p).all()
            p.setflags(write=False)
        _planes[(width, height)] = (colour, albedo, nd)
    return _planes[(width, height)]


_reference = {}


def reference(width, height, name, demodulate, with_albedo=True, with_guides=True):
    """denoise() of planes(width, height) under PARAM_SETS[name], computed once and read-only."""
    key = (width, height, name, demodulate, with_albedo, with_guides)
    if key not in _reference:
        colour, albedo, nd = planes(width, height)
        out = denoise(colour, albedo if with_albedo else None, nd if with_guides else None,
                      demodulate=demodulate, **PARAM_SETS[name])
        out.setflags(write=False)
        _reference[key] = out
    return _reference[key]


def scale(sigma):
    """k = 1 / sigma^2 in fp32: the product, then the division; 0 for sigma 0."""
    s = F(sigma)
    if s == 0:
        return F(0)
    s2 = F(s * s)
    return F(F(1) / s2)


def _sum_sq(p, q, channels):
    """sum over the channels of (p - q)^2, left to right."""
    acc = None
    for c in range(channels):
        d = p[..., c] - q[..., c]
        dd = d * d
        acc = dd if acc is None else acc + dd
    return acc


def denoise(colour, albedo=None, normal_depth=None, *, levels, sigma_normal, sigma_depth,
            sigma_albedo, sigma_colour, demodulate):
    """colour, albedo, normal_depth: float32 [H, W, 4] (the guides may be None). Returns the
    filtered plane float32 [H, W, 4]."""
    colour = np.asarray(colour, F)
    H, W = colour.shape[:2]
    k_n, k_z, k_a, k_c = (scale(s) for s in (sigma_normal, sigma_depth, sigma_albedo,
                                             sigma_colour))
    on_n = normal_depth is not None and k_n != 0
    on_z = normal_depth is not None and k_z != 0
    on_a = albedo is not None and k_a != 0
    demod = bool(demodulate) and albedo is not None
    with np.errstate(all="ignore"):
        if demod:
            floor = np.fmax(albedo[..., :3], EPS)
            s = colour[..., :3] / floor
        else:
            s = colour[..., :3].copy()
        kl = k_c
        for level in range(levels):
            step = 1 << level
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            for dy in range(-2, 3):
                oy = step * dy
                y0, y1 = max(0, -oy), min(H, H - oy)
                if y0 >= y1:
                    continue  # the whole row of taps is outside the frame
                for dx in range(-2, 3):
                    ox = step * dx
                    x0, x1 = max(0, -ox), min(W, W - ox)
                    if x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))                      # the pixels p
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))  # their taps q
                    h = K5[dx + 2] * K5[dy + 2]
                    X = np.zeros((y1 - y0, x1 - x0), F)  # the normal term's place: +0 when off
                    if on_n:
                        dn = _sum_sq(normal_depth[P], normal_depth[Q], 3)
                        X = dn * k_n
                    tz = F(0)
                    if on_z:
                        zp, zq = normal_depth[P][..., 3], normal_depth[Q][..., 3]
                        num = zp - zq
                        den = np.abs(zp) + np.abs(zq)
                        den = den + DEPTH_EPS
                        rz = num / den
                        rz2 = rz * rz
                        tz = rz2 * k_z
                    X = X + tz
                    ta = F(0)
                    if on_a:
                        da = _sum_sq(albedo[P], albedo[Q], 4)
                        ta = da * k_a
                    X = X + ta
                    tl = F(0)
                    if kl != 0:
                        dl = _sum_sq(s[P], s[Q], 3)
                        tl = dl * kl
                    X = X + tl
                    e = F(1) - np.fmin(X, F(1))
                    ee = e * e
                    w = h * ee
                    ws = w[..., None] * s[Q]
                    acc[P] = acc[P] + ws
                    wsum[P] = wsum[P] + w
            s = acc / wsum[..., None]
            kl = F(kl * F(4))
        out = np.empty((H, W, 4), F)
        out[..., :3] = s * floor if demod else s
        out[..., 3] = colour[..., 3]
    assert out.dtype == F and s.dtype == F
    return out
