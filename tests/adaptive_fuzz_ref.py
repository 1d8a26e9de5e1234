"""Shared inputs of the adaptive-sampling fuzz tests (no tests here): the generated scenes of
tests/query_fuzz_ref.py, as the 44 x 20 frames of tests/frame_fuzz_ref.py, for vcrt_draw_samples
(tracer.hip part 15) and the variance chain behind it (vcrt_reproject_moments, vcrt_variance,
vcrt_sample_counts, vcrt_denoise_variance).

* count_plane(rng, w, h, max_count, hits): a seeded count plane for a frame of any size: a
  background of 0 .. 6, a whole tile of zeros next to a tile of non-zeros, a stripe of words above
  max_count with 65535 among them, the residues 1, 2, 3 mod 4, a few heavy pixels at max_count.
* case(name, oracle): frame_fuzz_ref.frame(name) -- scene, environment, camera, lens -- with the
  seeded depth, max_count, first index and two such planes (round one; round two, accumulated).
* reference(oracle, c): tests/adaptive_ref.draw_samples of both rounds, computed once.
* listed_prediction(oracle, c, plane): what stats.listed_rays must be, from the host builders.
* history(c, surface), reference_chain(oracle, c): the variance chain's seeded history and its
  reference on the host up to the counts, with the case's target.
tests/test_adaptive_fuzz_cpu.py holds the conditions on these inputs;
tests/test_gpu_adaptive_fuzz.py runs them on the GPU.
"""
import math
import zlib

import numpy as np

import vulkancomputeraytracing_amd as vc
from tests import adaptive_ref as AR
from tests import frame_fuzz_ref as FF
from tests import motion_ref as M
from tests import variance_ref as V

F = np.float32
W, H = FF.W, FF.H
SEED = 20261023
CASE_NAMES = FF.CASE_NAMES
LIMIT = 1 << 19                  # first + max_count may reach it (vcrt.h)
DEPTHS = (1, 2, 3, 8)
MAX_COUNTS = (5, 9, 32, 64)
FIRST_KINDS = ("zero", "seven", "limit")   # limit: round two ends exactly at LIMIT
LENGTHS = (0, 1, 3, 8)           # history lengths per 5 x 3 block: both sides of min_history 4

# Seeded draws that are replaced, each with its reason.
DEPTH = {
    # the eye is in the middle of a glass sphere whose camera looks at a sphere that reaches into
    # it: at the drawn depth 2, and at 3, every path has exactly max_depth segments (glass,
    # then a hit), none ends early; at 8 they average 4.2
    "fuzz-inside-5": 8,
}
MAX_COUNT = {}
FIRST = {}
# The chain's target where sqrt(median / 4) of the reference variance does not spread the counts.
TARGET = {}

# The cases whose frame passes' planes hold NaN (test_frame_fuzz_cpu.NAN_CASES): no chain there.
FRAME_NAN_CASES = ("edge-nan-centre",)

# The variance chain's parameters (the defaults of the sequence tests in test_gpu_variance.py,
# min_history 4 between the generated lengths). The history's surface is this frame's own, so
# its depths are this camera's: a previous camera that stands elsewhere (`through`) shares the
# keys but no depth, and its cases run with the depth test off (a tolerance of 0).
CHAIN = dict(moments=dict(alpha=0.2, max_history=32.0, depth_tolerance=0.02, alpha_moments=0.2),
             variance=dict(min_history=4.0, alpha=0.2),
             denoise=dict(levels=3, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.125,
                          sigma_colour=4.0, demodulate=1))
# Previous states of the chain that replace the case's own, each with its reason.
_OTHER_KEYS = ("orbit: a camera inside the scene projects nearly every point onto a pixel where "
               "this frame's surface holds another sphere's key, so less than 4 % of the pixels "
               "take the history and over 98 % take the spatial estimate")
CHAIN_PREV = {name: _OTHER_KEYS for name in (
    "fuzz-cluster-6", "fuzz-line-3", "fuzz-line-15", "fuzz-line-21", "fuzz-line-27",
    "fuzz-big-4", "shape-G16", "shape-G192")}
CHAIN_N0 = 3       # two uniform rounds of three samples
CHAIN_MOST = 9     # sample_counts(target, 0, 9)

_cache = {}


def first_of(kind, max_count):
    return {"zero": 0, "seven": 7, "limit": LIMIT - 2 * max_count}[kind]


def quanta(plane, max_count):
    return (AR.clamp_counts(plane, max_count) + AR.Q - 1) // AR.Q


def count_plane(rng, w, h, max_count, hits=None, heavy=6):
    """A count plane [h, w] uint16 with, as far as the frame has room for them (a 44 x 20 frame
    has: tests/test_adaptive_fuzz_cpu.py):
    a background of 0 .. 6; one whole 8 x 8 tile of zeros and beside it a tile without a zero;
    a stripe of three words above max_count, 65535 the first; three pixels of 1, 2 and 3
    samples; three to `heavy` pixels at max_count, on `hits` (a mask [h, w]) where it has any
    free pixel. A later part never overwrites an earlier one. Last, where the item count came
    out a multiple of 64, one free pixel moves between one quantum and two: the last wave of
    vcrt_trace_samples then claims past the item table's end."""
    plane = rng.integers(0, 7, (h, w)).astype(np.uint16)
    taken = np.zeros((h, w), bool)
    tx_n, ty_n = (w + 7) // 8, (h + 7) // 8
    tiles = None
    if tx_n >= 2 and w >= 8 and h >= 8:   # a zero tile that lies whole inside the frame
        tx, ty = int(rng.integers(0, min(w // 8, tx_n - 1))), int(rng.integers(0, h // 8))
        tiles = (tx, ty), (tx + 1, ty)
    elif tx_n >= 2:
        tx, ty = int(rng.integers(0, tx_n - 1)), int(rng.integers(0, ty_n))
        tiles = (tx, ty), (tx + 1, ty)
    elif ty_n >= 2:
        ty = int(rng.integers(0, ty_n - 1))
        tiles = (0, ty), (0, ty + 1)
    if tiles is not None:
        (zx, zy), (nx, ny) = tiles
        z = (slice(8 * zy, 8 * zy + 8), slice(8 * zx, 8 * zx + 8))
        nb = (slice(8 * ny, 8 * ny + 8), slice(8 * nx, 8 * nx + 8))
        plane[z] = 0
        plane[nb] = rng.integers(1, 7, plane[nb].shape)
        taken[z] = taken[nb] = True
    # the stripe: the first seeded place whose pixels are free
    n = min(3, w)
    words = [65535, max_count + 1, max_count + 1 + int(rng.integers(0, 1000))][:n]
    for _ in range(200):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w - n + 1))
        if not taken[y, x:x + n].any():
            plane[y, x:x + n] = words
            taken[y, x:x + n] = True
            break
    free = np.flatnonzero(~taken)
    if len(free) >= 3:
        at = rng.choice(free, 3, replace=False)
        plane.reshape(-1)[at] = (1, 2, 3)
        taken.reshape(-1)[at] = True
    free = ~taken
    cand = np.flatnonzero(free & hits) if hits is not None and (free & hits).any() \
        else np.flatnonzero(free)
    k = min(int(rng.integers(3, heavy + 1)), len(cand))
    if k:
        at = rng.choice(cand, k, replace=False)
        plane.reshape(-1)[at] = max_count
        taken.reshape(-1)[at] = True
    free = np.flatnonzero(~taken)
    if int(quanta(plane, max_count).sum()) % 64 == 0 and len(free) and max_count >= 5:
        p = free[0]
        plane.reshape(-1)[p] = 5 if quanta(plane.reshape(-1)[p], max_count) <= 1 else 1
    plane.setflags(write=False)
    return plane


# ---------------------------------------------------------------------------------- the cases

def case(name, oracle):
    """One case: frame_fuzz_ref.frame(name) (scene, env, cam, lens, prev, ...) plus depth,
    max_count, first_kind, start (round one's first index; `first` stays the frame fuzz's),
    planes (two count planes), hits (the pixels whose first frame sample hits a sphere) and
    sdesc: the RenderDesc of the renderer the GPU test opens, the frame's at the seeded depth
    (`desc` stays the frame fuzz's)."""
    key = ("case", name)
    if key in _cache:
        return _cache[key]
    f = FF.frame(name, oracle)
    rng = np.random.default_rng([SEED, zlib.crc32(name.encode())])
    depth = int(rng.choice(DEPTHS))
    max_count = int(rng.choice(MAX_COUNTS))
    kind = str(rng.choice(FIRST_KINDS))
    depth, max_count, kind = DEPTH.get(name, depth), MAX_COUNT.get(name, max_count), \
        FIRST.get(name, kind)
    _, _, _, s, _ = FF.sample_hits(oracle, f)
    hits = (s.reshape(H * W, f["n"])[:, 0] >= 0).reshape(H, W)
    planes = tuple(count_plane(rng, W, H, max_count, hits) for _ in range(2))
    desc = vc.RenderDesc(width=W, height=H, samples_per_pixel=4, max_depth=depth, device=0,
                         lens_radius=f["lens"], **f["cam"])
    c = dict(f, depth=depth, max_count=max_count, first_kind=kind,
             start=first_of(kind, max_count), planes=planes, hits=hits, sdesc=desc)
    _cache[key] = c
    return c


def reference(oracle, c):
    """(one, two): adaptive_ref.draw_samples' (sums, mean, stats) of round one and of round two
    accumulated into round one's sums, computed once, read-only."""
    key = ("ref", c["name"])
    if key not in _cache:
        sc, desc, m = c["scene"], c["sdesc"], c["max_count"]
        one = AR.draw_samples(oracle, sc, desc, c["planes"][0], c["start"], m, sparse=True)
        two = AR.draw_samples(oracle, sc, desc, c["planes"][1], c["start"] + m, m, sums=one[0],
                              sparse=True)
        for r in (one, two):
            r[0].setflags(write=False)
            r[1].setflags(write=False)
        _cache[key] = (one, two)
    return _cache[key]


def listed_prediction(oracle, c, plane, max_count=None):
    """stats.listed_rays of draw_samples on `plane`: 0 for a lens renderer or a frame without
    lists, else the sum of n_p over the pixels whose 4 x 4 quarter has a list word (its low four
    bits not 15), as frame_fuzz_ref.routes finds the words from scene.primary_sphere_lists."""
    rt = FF.routes(oracle, c)
    if c["lens"] > 0 or rt["words"] is None:
        return 0
    n = AR.clamp_counts(plane, c["max_count"] if max_count is None else max_count)
    return int(n[(rt["words"] & 15) != 15].sum())


# ---------------------------------------------------------------------------- the variance chain

def in_chain(c, nan_cases=()):
    """The cases where the frame fuzz runs its consumers."""
    return c["prev"] in ("orbit", "through") and c["name"] not in FRAME_NAN_CASES and \
        c["name"] not in nan_cases


def chain_prev(c):
    return "orbit" if c["name"] in CHAIN_PREV else c["prev"]


def chain_previous(oracle, c):
    """(prev_desc, prev_scene) of the chain's motion pass: the case's previous state, or
    CHAIN_PREV's orbit."""
    if c["name"] in CHAIN_PREV:
        return FF._orbit(FF.pinhole(c), 3.0), None
    return FF.previous(oracle, c)[:2]


def chain_motion(oracle, c):
    """motion_ref.frame_motion of the chain's previous state."""
    if c["name"] not in CHAIN_PREV:
        return FF.reference(oracle, c)["motion"]
    key = ("motion", c["name"])
    if key not in _cache:
        _cache[key] = M.frame_motion(oracle, c["scene"], FF.pinhole(c),
                                     *chain_previous(oracle, c))
    return _cache[key]


def moments_params(c):
    return dict(CHAIN["moments"], depth_tolerance=0.0) if chain_prev(c) == "through" \
        else CHAIN["moments"]


def history(c, surface):
    """The seeded history of reproject_moments: frame_fuzz_ref.colour_planes()'s colour, this
    frame's surface, lengths of LENGTHS per block of 5 x 3 pixels, moments as variance_ref's."""
    rng = np.random.default_rng([SEED + 1, zlib.crc32(c["name"].encode())])
    blocks = rng.choice(np.asarray(LENGTHS, F), ((H + 2) // 3, (W + 4) // 5))
    length = np.ascontiguousarray(np.repeat(np.repeat(blocks, 3, axis=0), 5, axis=1)[:H, :W])
    m1 = rng.uniform(0.0, 2.0, (H, W)).astype(F)
    mom = np.zeros((H, W, 4), F)
    mom[..., 0] = m1
    mom[..., 1] = (m1 * m1 + rng.uniform(0.0, 0.5, (H, W))).astype(F)
    return dict(colour=np.array(FF.colour_planes()[1]), surface=np.array(surface),
                length=length.astype(F), moments=mom)


def uniform_rounds(oracle, c):
    """Two uniform rounds of CHAIN_N0 samples from index 0: (sums, mean, stats) of the second."""
    n0 = np.full((H, W), CHAIN_N0, np.uint16)
    one = AR.draw_samples(oracle, c["scene"], c["sdesc"], n0, 0, CHAIN_N0)
    return AR.draw_samples(oracle, c["scene"], c["sdesc"], n0, CHAIN_N0, CHAIN_N0, sums=one[0])


def target_of(var):
    """sqrt(median / 4) of the positive variances: half of those pixels ask for at most 4."""
    pos = np.asarray(var, np.float64)[np.asarray(var) > 0]
    return float(F(math.sqrt(float(np.median(pos)) / 4.0))) if pos.size else 0.1


def reference_chain(oracle, c):
    """The chain on the host from the references of its inputs: dict of mean, out, moments,
    accepted, variance, spatial, target, counts. Computed once."""
    key = ("chain", c["name"])
    if key not in _cache:
        ref = FF.reference(oracle, c)
        feat, mot = ref["features"], chain_motion(oracle, c)
        _, mean, _ = uniform_rounds(oracle, c)
        hist = history(c, mot["surface"])
        out, length, mom, took = V.reproject_moments(
            mean, mot["motion"], hist["colour"], hist["surface"], hist["length"], feat["albedo"],
            hist["moments"], **moments_params(c))
        var, spatial = V.variance(mom, mot["surface"], **CHAIN["variance"])
        target = TARGET.get(c["name"], target_of(var))
        counts, total = AR.sample_counts(var, target, 0, CHAIN_MOST)
        _cache[key] = dict(mean=mean, out=out, moments=mom, accepted=took, variance=var,
                           spatial=spatial, target=target, counts=counts, total=total)
    return _cache[key]
