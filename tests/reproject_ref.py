"""Temporal accumulation restated for the tests (no tests here): include/vcrt.h vcrt_reproject in
numpy float32, vectorised over the pixels, one rounded operation per statement; and the generated
planes the CPU and GPU tests share."""
import numpy as np

F = np.float32
DEPTH_EPS = F(2.0 ** -20)
DEFAULTS = dict(alpha=0.6, max_history=32.0, depth_tolerance=0.1)
SHAPES = [(44, 20), (70, 5), (100, 37), (3, 2), (1, 1)]
PARAM_SETS = {
    "defaults": dict(DEFAULTS),
    "long-history": dict(alpha=0.2, max_history=32.0, depth_tolerance=0.1),
    "no-depth-test": dict(alpha=0.1, max_history=8.0, depth_tolerance=0.0),
    "tight": dict(alpha=0.5, max_history=3.0, depth_tolerance=0.01),
    "alpha-one": dict(alpha=1.0, max_history=65535.0, depth_tolerance=0.25),
}

_cache = {}


def reproject(colour, motion, hcol, hsurf, hlen, alpha, max_history, depth_tolerance, taps=None):
    """(out [H, W, 4], out_length [H, W], accepted [H, W] bool): the definition. taps: a list
    that receives each tap's masks (inside, key_ok, length_ok, depth_ok)."""
    colour, motion = np.asarray(colour, F), np.asarray(motion, F)
    hcol, hsurf, hlen = np.asarray(hcol, F), np.asarray(hsurf, F), np.asarray(hlen, F)
    H, W = colour.shape[:2]
    alpha, cap, tol = F(alpha), F(max_history), F(depth_tolerance)
    mx, my, mz, mw = (motion[..., k] for k in range(4))
    with np.errstate(all="ignore"):
        valid = (mw >= 1) & (mx > -1) & (mx < F(W)) & (my > -1) & (my < F(H))
        sx, sy = np.where(valid, mx, F(0)), np.where(valid, my, F(0))
        fx, fy = np.floor(sx).astype(F), np.floor(sy).astype(F)
        ax, ay = (sx - fx).astype(F), (sy - fy).astype(F)
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        acc = np.zeros((H, W, 3), F)
        lsum, wsum = np.zeros((H, W), F), np.zeros((H, W), F)
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            bx = ax if dx else (F(1) - ax).astype(F)
            by = ay if dy else (F(1) - ay).astype(F)
            b = (bx * by).astype(F)
            qx, qy = ix + dx, iy + dy
            inside = valid & (b != 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)  # (read only where inside)
            key, zq, lq = hsurf[cy, cx, 0], hsurf[cy, cx, 1], hlen[cy, cx]
            num = np.abs((mz - zq).astype(F))
            den = ((np.abs(mz) + np.abs(zq)).astype(F) + DEPTH_EPS).astype(F)
            depth_ok = (mw == 1) | (tol == 0) | ((num / den).astype(F) <= tol)
            take = inside & (key == mw) & (lq >= 1) & depth_ok
            if taps is not None:
                taps.append((inside, key == mw, lq >= 1, depth_ok))
            hq = hcol[cy, cx, :3]
            acc = np.where(take[..., None], (acc + (b[..., None] * hq).astype(F)).astype(F), acc)
            lsum = np.where(take, (lsum + (b * lq).astype(F)).astype(F), lsum)
            wsum = np.where(take, (wsum + b).astype(F), wsum)
        took = wsum > 0
        safe = np.where(took, wsum, F(1))
        h3 = (acc / safe[..., None]).astype(F)
        L = (lsum / safe).astype(F)
        N = np.minimum((L + F(1)).astype(F), cap).astype(F)
        a = np.maximum(alpha, (F(1) / N).astype(F)).astype(F)
        blend = (h3 + (a[..., None] * (colour[..., :3] - h3).astype(F)).astype(F)).astype(F)
    out = colour.copy()
    out[..., :3] = np.where(took[..., None], blend, colour[..., :3])
    return out, np.where(took, N, F(1)).astype(F), took


def planes(w, h):
    """colour, motion, hcol, hsurf, hlen of the shape, generated once, read-only: a history of a
    few surfaces in blocks, a motion field around the identity with every special case the
    definition names sprinkled over it."""
    if (w, h) in _cache:
        return _cache[(w, h)]
    rng = np.random.default_rng(1000 * w + h)
    n = w * h
    colour = rng.uniform(0.0, 2.0, (h, w, 4)).astype(F)
    hcol = rng.uniform(0.0, 2.0, (h, w, 4)).astype(F)
    y, x = np.mgrid[0:h, 0:w]
    # surfaces in 5 x 3 blocks: keys 1 (the sky) .. 4, a depth per key with a little noise
    key = (1 + ((x // 5) + 2 * (y // 3)) % 4).astype(F)
    depth = np.where(key == 1, F(0), key * F(3.0) + rng.uniform(-0.05, 0.05, (h, w))).astype(F)
    hsurf = np.zeros((h, w, 4), F)
    hsurf[..., 0], hsurf[..., 1] = key, depth
    hsurf[..., 2:] = rng.uniform(-1, 1, (h, w, 2))  # not read
    hlen = rng.choice(np.asarray([0, 1, 1.5, 2, 7, 8, 31, 32, 65535], F), (h, w)).astype(F)
    motion = np.zeros((h, w, 4), F)
    motion[..., 0] = x + rng.uniform(-1.5, 1.5, (h, w))
    motion[..., 1] = y + rng.uniform(-1.5, 1.5, (h, w))
    # the key and depth of the surface near the target, so that most taps agree
    tx = np.clip(np.rint(motion[..., 0]), 0, w - 1).astype(np.int64)
    ty = np.clip(np.rint(motion[..., 1]), 0, h - 1).astype(np.int64)
    motion[..., 3] = key[ty, tx]
    motion[..., 2] = depth[ty, tx] * rng.choice(np.asarray([1, 1, 1, 1.005, 1.05, 1.5], F), (h, w))
    flat = motion.reshape(n, 4)
    xs, ys = x.reshape(-1).astype(F), y.reshape(-1).astype(F)
    special = [
        lambda i: (F(-1.0), ys[i]), lambda i: (F(-1.5), ys[i]), lambda i: (F(w), ys[i]),
        lambda i: (F(w + 0.5), ys[i]), lambda i: (xs[i], F(-1.0)), lambda i: (xs[i], F(-7.0)),
        lambda i: (xs[i], F(h)), lambda i: (xs[i], F(h + 3.25)),             # outside, every side
        lambda i: (F(-0.25), ys[i]), lambda i: (F(-0.75), F(-0.5)),          # partial taps
        lambda i: (F(w - 1 + 0.5), ys[i]), lambda i: (F(w - 0.25), F(h - 0.5)),
        lambda i: (xs[i], F(-0.125)), lambda i: (xs[i], F(h - 1 + 0.875)),
        lambda i: (xs[i], ys[i]), lambda i: (xs[i], F(ys[i] + 0.5)),          # integers: b == 0
        lambda i: (F(xs[i] + 0.25), ys[i]), lambda i: (F(0), F(0)),
        lambda i: (F(w - 1), F(h - 1)),
        lambda i: (F(np.nan), ys[i]), lambda i: (xs[i], F(np.nan)),
        lambda i: (F(np.inf), ys[i]), lambda i: (F(-np.inf), ys[i]),
        lambda i: (xs[i], F(np.inf)), lambda i: (xs[i], F(-np.inf)),
        lambda i: (F(1e30), ys[i]), lambda i: (xs[i], F(-1e30)), lambda i: (F(1e30), F(1e30)),
    ]
    order = rng.permutation(n)
    k = 0
    for rep in range(max(1, min(3, n // len(special)))):
        for fn in special:
            i = order[k % n]
            flat[i, 0], flat[i, 1] = fn(i)
            k += 1
    rest = order[k % n:] if k < n else order
    # the other words: invalid pixels, odd keys and depths
    for j, i in enumerate(rest[:max(1, len(rest) // 6)]):
        m = j % 8
        if m == 0:
            flat[i, 3] = 0                     # invalid
        elif m == 1:
            flat[i, 3] = F(np.nan)
        elif m == 2:
            flat[i, 3] = F(0.5)
        elif m == 3:
            flat[i, 3] = F(np.inf)             # valid, matches nothing
        elif m == 4:
            flat[i, 3] = F(1e30)
        elif m == 5:
            flat[i, 2] = F(np.nan)             # the depth test fails
        elif m == 6:
            flat[i, 2] = F(np.inf)
        else:
            flat[i, 3] = F(-3)
    out = (colour, motion, hcol, hsurf, hlen)
    for v in out:
        v.setflags(write=False)
    _cache[(w, h)] = out
    return out


def reference(w, h, name):
    k = ("ref", w, h, name)
    if k not in _cache:
        out = reproject(*planes(w, h), **PARAM_SETS[name])
        for v in out:
            v.setflags(write=False)
        _cache[k] = out
    return _cache[k]
