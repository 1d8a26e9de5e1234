"""Regenerates tests/golden/reference_shader.npz: results of the reference's compute shader,
compiled as C++ from the reference's own files (`make -C oracle ref` ->
oracle/_ref/libref_shader.so, see oracle/ref_shader_abi.h), recorded as DATA.

Run where oracle/_ref exists (the build container; the GPU box has no reference):
    python tests/golden/make_reference_shader_fixture.py
    python tests/golden/make_reference_shader_fixture.py --cli-cases FILE   # input of ref_shader_cli
    python tests/golden/make_reference_shader_fixture.py --cli-check FILE   # its output, checked

The fixture holds configurations, test scenes of our own, pixel coordinates, rays and result bit
patterns -- no program text. To stay below the largest golden file, the frames' pixels and the
rays' radiance are stored as SHA-256 prefixes of their bit patterns (one per frame row, per 64
listed pixels, per ray class; every NaN made one pattern first), the per-pixel counts of
ray_color's undefined return and the first-hit records in full.

Every frame is the reference's own accumulation: a sequential fp32 sum over the samples, divided
by their number (one accumulation quantum per pixel on our side).

Frame cases (scene: the final scene = the reference's own array, or one of `scenes`):
  ref            the reference's configuration, 1280x720, 1 spp, depth 50: 4000 seeded pixels and
                 the four corners (1280 and 720 are multiples of 16: its dispatch skips nothing)
  small, odd     96x54 4 spp depth 10; 33x21 7 spp (the jitter pairs rand(i,i), rand(i+1,i+1)
                 overlap) depth 3 -- whole frames, rows and columns >= 16*floor(dim/16) included
  aspect4/0      64x16 (integer aspect ratio 4) and 21x33 (ratio 0: a zero-width viewport)
  depth0/1       40x24 at depth 0 and 1
  mat_*          material ids 0, 4, 2.7 and -1; glass 0.5, 1.0 and 0, glass 1.5 everywhere; metal
                 fuzz 0 and 2;
                 Lambertian 0; a colour above 1; a negative and a zero radius; a NaN centre;
                 two spheres in one place (their roots tie)
  cam_*          the camera on its target, vup parallel to the view, vfov 170 and 0.5, the
                 camera inside the glass sphere, and looking up at the sky
Ray cases: 56 rays of each class A-G of tests/ray_query_ref.ray_batch on the scenes three, final
and mixed: ray_color at depths 1, 10, 50; the hit scan at (0.001, 1e5) and at the occlusion
tests' per-ray reaches (occlusion_ref.reach_of). Five rays more are aimed by hand at the boundaries
of hit_sphere's root test (edge_rays: a root equal to min_t, two roots that tie), results in full.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import occlusion_ref, oracle_py, ray_query_ref as R  # noqa: E402
from tests import reference_shader_ref as RS  # noqa: E402
from tests.oracle_py import SPHERE_DTYPE  # noqa: E402

DEFAULT_CAM = (13.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 20.0)
RAYS_PER_CLASS = 56
SCENE_ROWS = 25
MIN_T = np.float32(0.001)
INFINITY = np.float32(1e5)


def base_rows():
    """The scene of test_gpu_fuzz.test_edge_inputs_bitwise: ground, the big three, 20 small."""
    rows = [((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), 1, 1.0),
            ((0.0, 1.0, 0.0), 1.0, (1.0, 1.0, 1.0), 3, 1.5),
            ((-4.0, 1.0, 0.0), 1.0, (0.4, 0.2, 0.1), 1, 1.0),
            ((4.0, 1.0, 0.0), 1.0, (0.7, 0.6, 0.5), 2, 0.0)]
    rng = np.random.default_rng(7)
    for i in range(20):
        rows.append(((float(rng.uniform(-6, 6)), 0.2, float(rng.uniform(-6, 6))), 0.2,
                     tuple(float(v) for v in rng.uniform(0, 1, 3)), 1 + i % 3, 0.5))
    return rows


def spheres(rows):
    a = np.zeros(len(rows), dtype=SPHERE_DTYPE)
    for k, (c, r, col, mat, p) in enumerate(rows):
        a[k]["center"], a[k]["radius"], a[k]["colour"] = c, r, col
        a[k]["texture"] = (mat, p, 0.0)
    return a


def material_scenes():
    """name -> spheres. Every variant changes the base scene where the frame sees it."""
    base = spheres(base_rows())
    mat = base["texture"][:, 0].copy()
    out = {}
    for name, ident in (("mat_id0", 0.0), ("mat_id4", 4.0), ("mat_id2p7", 2.7), ("mat_idm1", -1.0)):
        s = base.copy()
        s["texture"][2, 0] = ident                   # the big Lambertian
        s["texture"][4::4, 0] = ident                # five of the small spheres
        out[name] = s
    for name, p in (("mat_glass0p5", 0.5), ("mat_glass1", 1.0), ("mat_glass0", 0.0)):
        s = base.copy()
        s["texture"][mat == 3, 1] = p
        out[name] = s
    for name, p in (("mat_fuzz0", 0.0), ("mat_fuzz2", 2.0)):
        s = base.copy()
        s["texture"][mat == 2, 1] = p
        out[name] = s
    s = base.copy()
    s["texture"][1:, 0], s["texture"][1:, 1] = 3.0, 1.5   # glass everywhere but the ground:
    out["mat_allglass"] = s                               # many exits through the sqrt'd cosine
    s = base.copy()
    s["texture"][1:, 1][mat[1:] == 1] = 0.0          # every Lambertian but the ground
    out["mat_lambert0"] = s
    s = base.copy()
    s["colour"][0], s["colour"][2] = (1.2, 1.2, 1.2), (1.5, 2.0, 1.2)
    out["mat_bright"] = s
    extra = {"mat_negradius": ((1.0, 0.5, 1.0), -0.5, (1.0, 0.0, 0.0), 1, 1.0),
             "mat_zeroradius": ((1.0, 0.5, 1.0), 0.0, (1.0, 0.0, 0.0), 2, 0.0),
             "mat_nancentre": ((float("nan"), 1.0, 0.0), 0.5, (1.0, 0.0, 0.0), 1, 1.0)}
    for name, row in extra.items():
        out[name] = np.concatenate([base, spheres([row])])
    # a second sphere in the big Lambertian's place, later in the list: the roots tie and the
    # comparison `max_t <= root` keeps the earlier one
    out["mat_twins"] = np.concatenate([base, spheres([((-4.0, 1.0, 0.0), 1.0, (0.1, 0.3, 1.0), 2,
                                                       0.1)])])
    return base, out


def edge_rays():
    """Rays aimed by hand at the two boundaries of hit_sphere's root test, every number exact in
    fp32 (so the boundary is met whatever the order of the operations). With r = 2^-11 and
    c = r + min_t (both multiples of 2^-33 below 2^-9: the sum is exact), the ray (0, (0,0,1))
    meets the sphere ((0,0,c), r) at the near root c - r == min_t exactly: a = 1, half_b = -c,
    fl(c^2) - r^2 and the discriminant r^2 are exact. `root <= min_t` rejects it and the far root
    c + r is taken. Two spheres in one place ((5,0,0), 1) tie at t = 4 for the ray (0, (1,0,0)):
    `max_t <= root` keeps the first. Returns (scene, O, D, T); T: the occlusion reaches, on the
    far root (strictly: not occluded) and one ulp above it (occluded), on the tie's root, 1e5."""
    r = np.float32(2.0 ** -11)
    c = np.float32(r + MIN_T)
    assert float(c) == float(r) + float(MIN_T) and np.float32(c - r) == MIN_T
    far = np.float32(c + r)  # one rounded addition, as hit_sphere's (-half_b + sqrtd) / a
    scene = spheres([((0.0, 0.0, float(c)), float(r), (0.8, 0.6, 0.4), 1, 0.9),
                     ((5.0, 0.0, 0.0), 1.0, (1.0, 0.1, 0.1), 1, 0.8),
                     ((5.0, 0.0, 0.0), 1.0, (0.1, 0.1, 1.0), 2, 0.1)])
    O = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, -1], [0, 0, 0]], np.float32)
    D = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 1], [0, 1, 0]], np.float32)
    T = np.array([far, np.nextafter(far, np.float32(1)), 4.0, 1e5, 1e5], np.float32)
    return scene, O, D, T


def cameras():
    d = list(DEFAULT_CAM)

    def cam(**kw):
        c = list(d)
        for k, v in kw.items():
            i = {"lookfrom": 0, "lookat": 3, "vup": 6}.get(k)
            if i is None:
                c[9] = v
            else:
                c[i:i + 3] = v
        return tuple(c)

    return {"cam_on_target": cam(lookat=d[0:3]),
            "cam_vup_parallel": cam(vup=(13.0, 2.0, 3.0)),
            "cam_fov170": cam(vfov=170.0),
            "cam_fov0p5": cam(vfov=0.5),
            "cam_in_glass": cam(lookfrom=(0.0, 1.0, 0.25), lookat=(4.0, 0.5, 2.0), vfov=70.0),
            "cam_sky": cam(lookfrom=(0.0, 3.0, 0.0), lookat=(0.3, 60.0, 0.2), vfov=40.0)}


def frame_cases():
    """[(name, (w, h, spp, depth), cam, scene name or None for final, xy or None for whole)]."""
    rng = np.random.default_rng(20261019)
    xy = np.stack([rng.integers(0, 1280, 4000), rng.integers(0, 720, 4000)], axis=1)
    corners = np.array([[0, 0], [1279, 0], [0, 719], [1279, 719]])
    cases = [("ref", (1280, 720, 1, 50), DEFAULT_CAM, None, np.concatenate([corners, xy])),
             ("small", (96, 54, 4, 10), DEFAULT_CAM, None, None),
             ("odd", (33, 21, 7, 3), DEFAULT_CAM, None, None),
             ("aspect4", (64, 16, 2, 10), DEFAULT_CAM, None, None),
             ("aspect0", (21, 33, 2, 10), DEFAULT_CAM, None, None),
             ("depth0", (40, 24, 2, 0), DEFAULT_CAM, None, None),
             ("depth1", (40, 24, 2, 1), DEFAULT_CAM, None, None)]
    _, mats = material_scenes()
    for name in mats:
        cases.append((name, (48, 27, 4, 10), DEFAULT_CAM, name, None))
    for name, cam in cameras().items():
        cases.append((name, (48, 27, 4, 10), cam, "base", None))
    return cases


def ray_subset(oracle):
    O, D, C = R.ray_batch(oracle)
    rng = np.random.default_rng(5)
    idx = np.concatenate([np.sort(rng.choice(np.nonzero(C == c)[0], RAYS_PER_CLASS, replace=False))
                          for c in RS.RAY_CLASSES])
    return idx, O[idx], D[idx], C[idx]


def build(lib, oracle):
    fx = {}
    base, mats = material_scenes()
    scene_names = ["base"] + list(mats)
    table = np.zeros((len(scene_names), SCENE_ROWS), dtype=SPHERE_DTYPE)
    lens = np.zeros(len(scene_names), np.int16)
    for k, s in enumerate([base] + [mats[n] for n in scene_names[1:]]):
        table[k, :len(s)], lens[k] = s, len(s)
    fx["scenes"], fx["scene_len"], fx["scene_names"] = table, lens, np.array(scene_names)

    cases = frame_cases()
    fx["frame_names"] = np.array([c[0] for c in cases])
    fx["frame_cfg"] = np.array([c[1] for c in cases], np.int32)
    fx["frame_cam"] = np.array([c[2] for c in cases], np.float32)
    fx["frame_scene"] = np.array([-1 if c[3] is None else scene_names.index(c[3]) for c in cases],
                                 np.int16)
    for name, cfg, cam, sname, xy in cases:
        if xy is not None:  # sorted by y * w + x, stored as the steps between them
            lin = np.sort(np.asarray(xy)[:, 1].astype(np.int64) * cfg[0] + np.asarray(xy)[:, 0])
            steps = np.diff(lin, prepend=0)
            assert steps.max() < 65536
            fx[f"steps_{name}"] = steps.astype(np.uint16)
    digs, undefs = [], []
    for name in fx["frame_names"]:  # through the accessor the tests use
        c = RS.frame_case(fx, str(name))
        rgba, undef = lib.render_pixels(c["cfg"], c["cam"], c["scene"], c["xy"])
        assert (RS.canon_bits(rgba[:, 3]) == 0x3F800000).all()
        digs.append(RS.digests(rgba[:, :3], c["block"]))
        assert undef.max() <= 255
        undefs.append(undef.astype(np.uint8))
    fx["frame_digests"], fx["frame_undefined"] = np.concatenate(digs), np.concatenate(undefs)

    idx, O, D, C = ray_subset(oracle)
    fx["ray_index"], fx["ray_O"], fx["ray_D"], fx["ray_class"] = idx.astype(np.int16), O, D, C
    per = {k: [] for k in ("scene_sha", "rgb", "undefined", "accepted", "t", "sphere", "normal",
                           "T", "occluded")}
    for sname in RS.RAY_SCENES:
        sc = np.ascontiguousarray(R.scene_of(oracle, sname), dtype=SPHERE_DTYPE)
        per["scene_sha"].append(np.frombuffer(
            hashlib.sha256(sc.tobytes()).digest()[:RS.DIGEST_BYTES], np.uint8))
        colours = [lib.ray_color(sc, O, D, depth) for depth in RS.RAY_DEPTHS]
        per["rgb"].append(np.stack([RS.class_digests(rgb, C) for rgb, _ in colours]))
        per["undefined"].append(np.stack([np.packbits(u) for _, u in colours]))
        acc, t, sphere, normal = lib.hit_scan(sc, O, D, MIN_T, INFINITY)
        per["accepted"].append(np.packbits(acc))
        per["t"].append(RS.canon_bits(t))
        per["sphere"].append(sphere.astype(np.int16))
        per["normal"].append(RS.class_digests(normal, C))
        T = occlusion_ref.reach_of(t)[0]   # from the reference's own first hits
        occ, _, _, _ = lib.hit_scan(sc, O, D, MIN_T, T)
        per["T"].append(T.view(np.uint32))
        per["occluded"].append(np.packbits(occ))
    for k, v in per.items():
        fx[f"ray_{k}"] = np.stack(v)

    sc, O, D, T = edge_rays()  # a handful: results in full
    fx["edge_scene"], fx["edge_O"], fx["edge_D"], fx["edge_T"] = sc, O, D, T
    colours = [lib.ray_color(sc, O, D, depth) for depth in RS.RAY_DEPTHS]
    fx["edge_rgb"] = np.stack([RS.canon_bits(rgb) for rgb, _ in colours])
    fx["edge_undefined"] = np.stack([u for _, u in colours]).astype(np.uint8)
    acc, t, sphere, normal = lib.hit_scan(sc, O, D, MIN_T, INFINITY)
    fx["edge_t"], fx["edge_sphere"] = RS.canon_bits(t), sphere.astype(np.int16)
    fx["edge_normal"] = RS.canon_bits(normal)
    fx["edge_occluded"] = lib.hit_scan(sc, O, D, MIN_T, T)[0].astype(np.uint8)
    # the boundaries are met: far root, tie to the lower index, then a plain hit and a miss
    assert t[0] == np.float32(sc[0]["center"][2] + sc[0]["radius"]) and t[2] == 4.0
    assert sphere.tolist() == [0, 0, 1, 0, -1] and acc.tolist() == [1, 1, 1, 1, 0]
    assert fx["edge_occluded"].tolist() == [0, 1, 0, 1, 0]

    rng = np.random.default_rng(11)
    xs = [(float(i), float(i)) for i in range(24)] + [(1023.0, 1023.0), (1024.0, 1024.0)]
    xs += [tuple(v) for v in rng.uniform(-12, 12, (20, 2)).astype(np.float32).tolist()]
    xs += [tuple(v) for v in (rng.normal(size=(18, 2)) * 1000).astype(np.float32).tolist()]
    fx["rand_xy"] = np.array(xs, np.float32)
    fx["rand_bits"] = RS.canon_bits(np.array([lib.rand(x, y) for x, y in fx["rand_xy"]],
                                             np.float32))
    return fx


# ---- the stand-alone driver's input and the check of its output ---------------------------------

def _hex(a):
    return " ".join(f"{int(v):08x}" for v in np.ascontiguousarray(a, np.float32).view(np.uint32).ravel())


def _world_cmd(sc):
    if sc is None:
        return ["world -1"]
    sc = np.ascontiguousarray(sc, dtype=SPHERE_DTYPE)
    flat = sc.view(np.float32).reshape(len(sc), 10)
    return [f"world {len(sc)}"] + [_hex(r) for r in flat]


def cli_cases(fx, oracle):
    lines = []
    for name in RS.frame_names(fx):
        c = RS.frame_case(fx, name)
        lines += _world_cmd(c["scene"])
        w, h, spp, depth = c["cfg"]
        head = f"frame {w} {h} {spp} {depth} {_hex(c['cam'])}"
        if c["whole"]:
            lines.append(head + " -1")
        else:
            lines.append(head + f" {len(c['xy'])} " + " ".join(str(int(v)) for v in c["xy"].ravel()))
    O, D = fx["ray_O"], fx["ray_D"]
    for sname in RS.RAY_SCENES:
        lines += _world_cmd(RS.ray_scene(oracle, fx, sname))
        for depth in RS.RAY_DEPTHS:
            lines += [f"ray {depth} {_hex(O[i])} {_hex(D[i])}" for i in range(len(O))]
        T = RS.ray_case(fx, sname)["T"]
        lines += [f"scan {_hex(O[i])} {_hex(D[i])} {_hex(MIN_T)} {_hex(INFINITY)}"
                  for i in range(len(O))]
        lines += [f"scan {_hex(O[i])} {_hex(D[i])} {_hex(MIN_T)} {_hex(T[i])}"
                  for i in range(len(O))]
    O, D, T = fx["edge_O"], fx["edge_D"], fx["edge_T"]
    lines += _world_cmd(fx["edge_scene"])
    for depth in RS.RAY_DEPTHS:
        lines += [f"ray {depth} {_hex(O[i])} {_hex(D[i])}" for i in range(len(O))]
    lines += [f"scan {_hex(O[i])} {_hex(D[i])} {_hex(MIN_T)} {_hex(INFINITY)}" for i in range(len(O))]
    lines += [f"scan {_hex(O[i])} {_hex(D[i])} {_hex(MIN_T)} {_hex(T[i])}" for i in range(len(O))]
    lines += [f"rand {_hex(v)}" for v in fx["rand_xy"]]
    return "\n".join(lines) + "\n"


def cli_check(fx, text):
    """The driver's output for cli_cases(), compared with the fixture record for record."""
    rows = [ln.split() for ln in text.splitlines()]
    pos = 0

    def take(n, tag):
        nonlocal pos
        part = rows[pos:pos + n]
        assert len(part) == n and all(r[0] == tag for r in part), (tag, pos)
        pos += n
        return part

    def f32(words):
        return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)

    for name in RS.frame_names(fx):
        c = RS.frame_case(fx, name)
        part = take(len(c["xy"]), "p")
        rgb = np.stack([f32(r[1:4]) for r in part])
        assert np.array_equal(RS.digests(rgb, c["block"]), c["digests"]), name
        assert np.array_equal(np.array([int(r[5]) for r in part]), c["undefined"]), name
    C, n = fx["ray_class"], len(fx["ray_O"])
    for sname in RS.RAY_SCENES:
        rc = RS.ray_case(fx, sname)
        for depth in RS.RAY_DEPTHS:
            part = take(n, "c")
            rgb = np.stack([f32(r[1:4]) for r in part])
            assert np.array_equal(RS.class_digests(rgb, C), rc["rgb"][depth]), sname
            und = np.array([int(r[4]) for r in part], bool)
            assert np.array_equal(und, rc["undefined"][depth]), sname
        part = take(n, "h")
        assert np.array_equal(np.array([int(r[1]) for r in part], bool), rc["accepted"]), sname
        assert np.array_equal(RS.canon_bits(f32([r[2] for r in part])), rc["t"]), sname
        assert np.array_equal(np.array([int(r[3]) for r in part]), rc["sphere"]), sname
        nrm = np.stack([f32(r[4:7]) for r in part])
        assert np.array_equal(RS.class_digests(nrm, C), rc["normal"]), sname
        part = take(n, "h")
        assert np.array_equal(np.array([int(r[1]) for r in part], bool), rc["occluded"]), sname
    n = len(fx["edge_O"])
    for i, depth in enumerate(RS.RAY_DEPTHS):
        part = take(n, "c")
        assert np.array_equal(RS.canon_bits(np.stack([f32(r[1:4]) for r in part])), fx["edge_rgb"][i])
        assert [int(r[4]) for r in part] == fx["edge_undefined"][i].tolist()
    part = take(n, "h")
    assert np.array_equal(RS.canon_bits(f32([r[2] for r in part])), fx["edge_t"])
    assert [int(r[3]) for r in part] == fx["edge_sphere"].tolist()
    assert np.array_equal(RS.canon_bits(np.stack([f32(r[4:7]) for r in part])), fx["edge_normal"])
    part = take(n, "h")
    assert [int(r[1]) for r in part] == fx["edge_occluded"].tolist()
    part = take(len(fx["rand_xy"]), "r")
    assert np.array_equal(RS.canon_bits(f32([r[1] for r in part])), fx["rand_bits"])
    assert pos == len(rows), "trailing output"
    return pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli-cases")
    ap.add_argument("--cli-check")
    args = ap.parse_args()
    oracle = oracle_py.load()
    if args.cli_cases:
        with open(args.cli_cases, "w") as f:
            f.write(cli_cases(RS.load_fixture(), oracle))
        return
    if args.cli_check:
        with open(args.cli_check) as f:
            print(f"{cli_check(RS.load_fixture(), f.read())} records equal the fixture")
        return
    lib = RS.load()
    if lib is None:
        sys.exit("oracle/_ref/libref_shader.so is missing: run `make -C oracle ref` first")
    fx = build(lib, oracle)
    np.savez_compressed(RS.FIXTURE, **fx)
    size = os.path.getsize(RS.FIXTURE)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)
                  if f != os.path.basename(RS.FIXTURE))
    print(f"{RS.FIXTURE}: {size} bytes (largest other golden file: {largest})")
    assert size <= largest, "the fixture must not be the largest golden file"
    for name in RS.frame_names(fx):
        c = RS.frame_case(fx, name)
        print(f"  {name:18s} undefined returns {int(c['undefined'].sum()):6d} of "
              f"{len(c['xy']) * c['cfg'][2]} samples")


if __name__ == "__main__":
    main()
