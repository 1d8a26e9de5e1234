"""Shared code of the reference-shader tests (no tests here).

* RefShader: ctypes binding of oracle/_ref/libref_shader.so, the reference's compute shader
  compiled as C++ by `make -C oracle ref` (oracle/ref_shader_abi.h). Present only where the
  reference is; load() returns None elsewhere.
* The fixture tests/golden/reference_shader.npz (written by make_reference_shader_fixture.py from
  that library): load_fixture(), and the accessors of its frame and ray cases.
* canon_bits() / digests(): bit patterns with every NaN made one pattern (NaN against NaN counts
  as equal, as in test_gpu_fuzz._same_bits_or_both_nan), and SHA-256 prefixes of blocks of them:
  what the fixture stores for the frames and the rays' radiance.
"""
import ctypes
import hashlib
import os

import numpy as np

from tests.oracle_py import ORACLE_DIR, SPHERE_DTYPE

LIB = os.path.join(ORACLE_DIR, "_ref", "libref_shader.so")
CLI = os.path.join(ORACLE_DIR, "_ref", "ref_shader_cli")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "reference_shader.npz")

RAY_SCENES = ("three", "final", "mixed")
RAY_DEPTHS = (1, 10, 50)
RAY_CLASSES = "ABCDEFG"      # class H (non-finite rays, zero directions) is outside the contract
PIXEL_BLOCK = 64             # pixels per digest of a pixel-list frame case
DIGEST_BYTES = 16
QNAN = np.uint32(0x7FC00000)


class RefConfig(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("spp", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("lookfrom", ctypes.c_float * 3), ("lookat", ctypes.c_float * 3),
                ("vup", ctypes.c_float * 3), ("vfov", ctypes.c_float)]


def canon_bits(a):
    """uint32 bit patterns of float32 `a`, every NaN replaced by one quiet NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = QNAN
    return b


def digests(a, block):
    """SHA-256 prefixes [nblocks, 16] uint8 of canon_bits(a) cut into blocks of `block` rows
    (a is [n, ...]; the last block may be short)."""
    b = canon_bits(a)
    n = len(b)
    out = [hashlib.sha256(b[i:i + block].tobytes()).digest()[:DIGEST_BYTES]
           for i in range(0, n, block)]
    return np.frombuffer(b"".join(out), np.uint8).reshape(len(out), DIGEST_BYTES).copy()


def class_digests(a, classes):
    """One digest per ray class, in RAY_CLASSES order."""
    return np.concatenate([digests(a[classes == c], 1 << 30) for c in RAY_CLASSES])


def differing_blocks(got, want):
    return np.nonzero((np.asarray(got) != np.asarray(want)).any(axis=1))[0]


class RefShader:
    def __init__(self, path=LIB):
        self.lib = L = ctypes.CDLL(path)
        vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
        L.ref_default_world.restype = i32
        L.ref_default_world.argtypes = [vp, i32]
        L.ref_default_config.restype = None
        L.ref_default_config.argtypes = [ctypes.POINTER(RefConfig)]
        L.ref_render_pixels.restype = ctypes.c_int64
        L.ref_render_pixels.argtypes = [ctypes.POINTER(RefConfig), vp, i32, vp, i32, vp, vp]
        L.ref_ray_color.restype = i32
        L.ref_ray_color.argtypes = [vp, i32, vp, vp, i32, vp]
        L.ref_hit_scan.restype = i32
        L.ref_hit_scan.argtypes = [vp, i32, vp, vp, f32, f32, vp, vp, vp]
        L.ref_rand.restype = f32
        L.ref_rand.argtypes = [f32, f32]

    @staticmethod
    def _scene(scene):
        """(keepalive array, pointer, n); None = the reference's own array."""
        if scene is None:
            return None, None, 0
        sc = np.ascontiguousarray(scene, dtype=SPHERE_DTYPE)
        return sc, sc.ctypes.data, len(sc)

    def default_world(self):
        n = self.lib.ref_default_world(None, 0)
        arr = np.zeros(n, dtype=SPHERE_DTYPE)
        self.lib.ref_default_world(arr.ctypes.data, n)
        return arr

    def default_config(self):
        c = RefConfig()
        self.lib.ref_default_config(ctypes.byref(c))
        return c

    def render_pixels(self, cfg, cam, scene, xy):
        """cfg = (w, h, spp, depth), cam = 10 floats (lookfrom, lookat, vup, vfov):
        (rgba [n, 4] float32, undefined returns per pixel [n] int32)."""
        c = RefConfig()
        c.width, c.height, c.spp, c.max_depth = (int(v) for v in cfg)
        cam = np.asarray(cam, np.float32)
        c.lookfrom[:], c.lookat[:], c.vup[:] = cam[0:3].tolist(), cam[3:6].tolist(), cam[6:9].tolist()
        c.vfov = float(cam[9])
        keep, ptr, n = self._scene(scene)
        xy = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        rgba = np.zeros((len(xy), 4), np.float32)
        undef = np.zeros(len(xy), np.int32)
        r = self.lib.ref_render_pixels(ctypes.byref(c), ptr, n, xy.ctypes.data, len(xy),
                                       rgba.ctypes.data, undef.ctypes.data)
        if r < 0:
            raise ValueError(f"ref_render_pixels: {r}")
        assert r == int(undef.sum())
        return rgba, undef

    def ray_color(self, scene, O, D, depth):
        keep, ptr, n = self._scene(scene)
        O = np.ascontiguousarray(O, np.float32)
        D = np.ascontiguousarray(D, np.float32)
        rgb = np.zeros((len(O), 3), np.float32)
        undef = np.zeros(len(O), bool)
        f = self.lib.ref_ray_color
        po, pd, pc = O.ctypes.data, D.ctypes.data, rgb.ctypes.data
        for i in range(len(O)):
            undef[i] = f(ptr, n, po + 12 * i, pd + 12 * i, depth, pc + 12 * i) != 0
        return rgb, undef

    def hit_scan(self, scene, O, D, min_t, max_t):
        """max_t a scalar or [n]: (accepted [n] bool, t [n], sphere [n] int32, normal [n, 3])."""
        keep, ptr, n = self._scene(scene)
        O = np.ascontiguousarray(O, np.float32)
        D = np.ascontiguousarray(D, np.float32)
        T = np.broadcast_to(np.asarray(max_t, np.float32), (len(O),))
        acc = np.zeros(len(O), bool)
        t = np.zeros(len(O), np.float32)
        idx = np.zeros(len(O), np.int32)
        nrm = np.zeros((len(O), 3), np.float32)
        f = self.lib.ref_hit_scan
        po, pd = O.ctypes.data, D.ctypes.data
        for i in range(len(O)):
            acc[i] = f(ptr, n, po + 12 * i, pd + 12 * i, float(min_t), float(T[i]),
                       t.ctypes.data + 4 * i, idx.ctypes.data + 4 * i,
                       nrm.ctypes.data + 12 * i) != 0
        return acc, t, idx, nrm

    def rand(self, x, y):
        return self.lib.ref_rand(float(x), float(y))


_lib = None


def load():
    """The library, or None where oracle/_ref was not built (no reference on this machine)."""
    global _lib
    if _lib is None and os.path.exists(LIB):
        _lib = RefShader()
    return _lib


# ---- the fixture ------------------------------------------------------------------------------

_fixture = None


def load_fixture():
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
        for v in _fixture.values():
            v.setflags(write=False)
    return _fixture


def frame_names(fx):
    return [str(s) for s in fx["frame_names"]]


def _frame_pixels(fx, k):
    """(xy [n, 2] int32, pixels per digest, whole frame?) of frame case k. A listed case stores its
    pixels sorted by y * w + x, as the uint16 steps between them (the first from 0)."""
    w, h = int(fx["frame_cfg"][k][0]), int(fx["frame_cfg"][k][1])
    name = str(fx["frame_names"][k])
    if f"steps_{name}" in fx:
        lin = np.cumsum(fx[f"steps_{name}"].astype(np.int64))
        return np.stack([lin % w, lin // w], axis=1).astype(np.int32), PIXEL_BLOCK, False
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.int32), w, True


def frame_case(fx, name):
    """dict of a frame case: cfg (w, h, spp, depth), cam [10], scene (array, or None for the
    final scene), xy [n, 2] int32 (every pixel row by row for a whole-frame case), block (pixels
    per digest), digests, undefined [n]. The cases' digests and undefined-return counts lie one
    after the other in frame_digests and frame_undefined (absent while the fixture is made)."""
    names = frame_names(fx)
    k = names.index(name)
    w, h, spp, depth = (int(v) for v in fx["frame_cfg"][k])
    si = int(fx["frame_scene"][k])
    scene = None if si < 0 else fx["scenes"][si][:int(fx["scene_len"][si])]
    xy, block, whole = _frame_pixels(fx, k)
    out = dict(name=name, cfg=(w, h, spp, depth), cam=fx["frame_cam"][k], scene=scene, xy=xy,
               block=block, whole=whole)
    if "frame_digests" in fx:
        p0 = d0 = 0
        for j in range(k):
            pj, bj, _ = _frame_pixels(fx, j)
            p0, d0 = p0 + len(pj), d0 + -(-len(pj) // bj)
        out["digests"] = fx["frame_digests"][d0:d0 + -(-len(xy) // block)]
        out["undefined"] = fx["frame_undefined"][p0:p0 + len(xy)].astype(np.int32)
    return out


def cam_kwargs(cam):
    cam = np.asarray(cam, np.float32)
    return dict(lookfrom=tuple(float(v) for v in cam[0:3]), lookat=tuple(float(v) for v in cam[3:6]),
                vup=tuple(float(v) for v in cam[6:9]), vfov=float(cam[9]))


def ray_scene(oracle, fx, name):
    """A ray scene rebuilt from the project's own generators, checked against the SHA-256 the
    fixture recorded for it."""
    from tests import ray_query_ref as R
    sc = np.ascontiguousarray(R.scene_of(oracle, name), dtype=SPHERE_DTYPE)
    sha = hashlib.sha256(sc.tobytes()).digest()[:DIGEST_BYTES]
    want = fx["ray_scene_sha"][RAY_SCENES.index(name)].tobytes()
    assert sha == want, f"scene {name} is not the fixture's"
    return sc


def ray_case(fx, scene):
    """dict of the ray results on one scene: rgb[depth] (class digests), undefined[depth] [n]
    bool, accepted [n] bool, t [n] uint32 bits, sphere [n], normal (class digests), T [n] float32
    (the occlusion reach) and occluded [n] bool."""
    s, n = RAY_SCENES.index(scene), len(fx["ray_O"])

    def flags(a):
        return np.unpackbits(a)[:n].astype(bool)

    return dict(rgb={d: fx["ray_rgb"][s, i] for i, d in enumerate(RAY_DEPTHS)},
                undefined={d: flags(fx["ray_undefined"][s, i]) for i, d in enumerate(RAY_DEPTHS)},
                accepted=flags(fx["ray_accepted"][s]), t=fx["ray_t"][s],
                sphere=fx["ray_sphere"][s].astype(np.int32), normal=fx["ray_normal"][s],
                T=fx["ray_T"][s].view(np.float32), occluded=flags(fx["ray_occluded"][s]))
