"""The query fuzz cases without a GPU (tests/query_fuzz_ref.py): conditions on the inputs and the
references alone, so that a green run of tests/test_gpu_query_fuzz.py means something. The shape
cases hit the hierarchy and big-list shapes they are named for; the numpy first hit agrees with
the oracle on every case; every batch has the composition its classes promise; and mutants of
the references -- the mistakes a scan kernel can make -- change the answers of enough rays that
the bitwise comparison on the GPU would see them.

Measured (python -m pytest tests/test_query_fuzz_cpu.py -s prints them):
  hierarchy first hits, share of the contract's rays: 0.220 (fuzz-inside-29) .. 0.830 (fuzz-big-2)
  rays changed by each mutant, summed over the 59 cases / in the cases the floor names:
    (a) ties to the later index         5337 / edge-duplicates 1196
    (b) root <= min_t as <              1856 (the 32 searched rays of 58 cases)
    (c) max_t <= root, T <= root as <  11200
    (d) no far root                    32155
    (e) normal / |radius|               1259 / fuzz cases with shells 1219
    (f) last n % 4 spheres skipped      4567
    (g) last quarter of the small ones  8803
    (h) occlusion at 1e5, not T        35314 / scaled cases above 100: 1840
"""
import numpy as np
import pytest

from vulkancomputeraytracing_amd import scene as S
from tests import query_fuzz_ref as F
from tests import ray_query_ref as R

MIN_T, INFINITY = R.MIN_T, R.INFINITY


tables_of, bounded = F.tables_of, F.bounded


def big_by_rule(scene):
    """vcrt.h: radius > 8 x the median and > 5% of the centres' extent."""
    r = np.abs(scene["radius"])
    c = scene["center"].astype(np.float64)
    extent = np.sqrt(((c.max(axis=0) - c.min(axis=0)) ** 2).sum())
    return int((r > max(8.0 * float(np.sort(r)[len(r) // 2]), 0.05 * extent)).sum())


def hierarchy_spheres(t):
    idx = t["index"][t["nbig"]:].ravel()
    return idx[idx >= 0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------- the shape cases

@pytest.mark.parametrize("g", F.SHAPE_G)
def test_shape_g_cases_report_their_group_count(g):
    c = F.case(f"shape-G{g}")
    t = tables_of(c)
    assert len(t["index"]) - t["nbig"] == g
    assert t["nbig"] == 1 and S.cull_slab(c["scene"]) is not None
    assert len(c["scene"]) == F.SHAPE_G[g] + 1


@pytest.mark.parametrize("name", [n for n in F.CASE_NAMES if n.startswith("shape-big")])
def test_shape_big_cases_report_their_big_list(name):
    c = F.case(name)
    k = int(name.removesuffix("-nofill")[len("shape-big"):])
    t = tables_of(c)
    assert big_by_rule(c["scene"]) == k
    assert len(t["index"]) - t["nbig"] == 48
    assert t["nbig"] == (k + 3) // 4
    members = int((t["index"][:t["nbig"]] >= 0).sum())
    if name.endswith("-nofill"):   # one partly filled big group
        assert members == k and t["nbig"] == 1
    else:                          # free slots taken by the largest small spheres
        assert members == 4 * t["nbig"]
    # the big spheres are where the rule says: in the big groups
    r = np.abs(c["scene"]["radius"])
    assert set(np.nonzero(r > 8 * np.median(r))[0]) <= set(t["index"][:t["nbig"]].ravel())


def test_edge_cases_are_what_they_are_named_for():
    assert tables_of(F.case("edge-15")) is None and len(F.case("edge-15")["scene"]) == 15
    assert tables_of(F.case("edge-16")) is not None and len(F.case("edge-16")["scene"]) == 16
    for name in ("edge-nan-centre", "edge-huge-radius"):
        c = F.case(name)
        assert not bounded(c["scene"]) and tables_of(c) is None and len(c["scene"]) >= 16
    for name, radius in (("edge-zero-radius", 0.0), ("edge-tiny-radius", 2.0 ** -45)):
        c = F.case(name)   # bounded, with tables, outside kFlagRadiiSafe (|radius| < 2^-40)
        assert bounded(c["scene"]) and tables_of(c) is not None
        assert (c["scene"]["radius"] == np.float32(radius)).sum() == 1
        assert (np.abs(c["scene"]["radius"]) < 2.0 ** -40).sum() == 1
    line = F.case("edge-line-one-radius")["scene"]
    assert len(set(line["radius"])) == 1 and len(set(line["center"][:, 1])) == 1
    assert tables_of(F.case("edge-line-one-radius"))["nbig"] == 0
    dup = F.case("edge-duplicates")["scene"]
    assert len(dup) == 80
    for k in ("center", "radius"):
        assert np.array_equal(dup[k][:40], dup[k][40:][::-1])
    assert not np.array_equal(dup["colour"][:40], dup["colour"][40:][::-1])


def test_case_list(oracle):
    cases = F.scene_cases(oracle)
    assert len(cases) == len(set(F.CASE_NAMES)) == 59
    assert all(16 <= len(c["scene"]) <= 1500 or c["name"] == "edge-15" for c in cases)
    for kind, seeds in F.FUZZ_SEEDS.items():
        mine = [c for c in cases if c["family"] == "fuzz" and c["kind"] == kind]
        assert len(mine) == len(seeds) == 5 and sum(c["bright"] for c in mine) == 1
    scales = sorted(c["scale"] for c in cases if c["kind"] == "scaled")
    assert scales[0] < 0.02 and scales[-1] > 500
    g = {len(t["index"]) - t["nbig"] for t in map(tables_of, cases) if t is not None}
    print("hierarchy group counts:", sorted(g))
    assert set(F.SHAPE_G) <= g


# --------------------------------------------------------------- the references on the cases

@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_first_hit_agrees_with_the_oracle(oracle, name):
    """A ray hits something exactly when ray_color at depth 1 is (0, 0, 0)
    (tests/test_ray_query_cpu.py, on every new case)."""
    c = F.case(name, oracle)
    O, D, C = F.rays(c)
    ref = F.reference(oracle, c)
    fin = ref["finite"]
    rgb, segs = R.oracle_paths(oracle, c["scene"], O, D, 1)
    assert np.all(segs == 1)
    hit = (rgb == 0).all(axis=1)
    assert np.array_equal(hit[fin], (ref["sphere"] >= 0)[fin])
    miss = fin & ~hit
    assert np.all(ref["t"][miss] == INFINITY) and np.all(ref["normal"][miss] == 0)
    # the rays outside the contract are class H, at most 2% of the batch
    assert np.array_equal(~fin, C == "H") and (~fin).sum() <= 0.02 * len(O)
    # NaN in a contract ray's record: only where the scene holds one or divides by a zero radius
    nan = np.isnan(ref["t"][fin]).sum() + np.isnan(ref["normal"][fin]).any(axis=1).sum()
    if name not in ("edge-nan-centre", "edge-zero-radius"):
        assert nan == 0
        assert np.all((ref["t"][fin & hit] > MIN_T) & (ref["t"][fin & hit] < INFINITY))
    if name == "edge-nan-centre":  # in the reference's arithmetic every ray hits that sphere
        assert nan > 1000


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_batch_composition(oracle, name):
    c = F.case(name, oracle)
    O, D, C = F.rays(c)
    ref = F.reference(oracle, c)
    fin = ref["finite"]
    assert len(O) == 1537 == 64 * 24 + 1
    assert "".join(C) == "".join(k * F.SIZES[k] for k in "ABCDEFGH")
    assert sum(F.SIZES[k] for k in "FGH") <= 0.10 * len(O) and F.SIZES["H"] <= 0.02 * len(O)
    # in class order the waves of A..E are guarded whole: they take the culled scan
    guard = F.guarded(O, D)
    a = (D.astype(np.float64) ** 2).sum(axis=1)
    ae = np.isin(C, list("ABCDE"))
    assert guard[ae].all() and np.all((a[ae] > 2.0 ** -19) & (a[ae] < 2.0 ** 59))
    assert np.all(np.abs(O[ae]) < 2.0 ** 29)
    # (C) zero components; the first half on a centre's (or box face's) coordinate, bit for bit
    dc, oc = D[C == "C"], O[C == "C"]
    assert np.all((dc == 0).sum(axis=1) >= 1) and np.all((dc == 0).sum(axis=1) <= 2)
    cen, rad = c["scene"]["center"], np.abs(c["scene"]["radius"])
    for axis in range(3):
        own = set(bits(cen[:, axis])) | set(bits(cen[:, axis] + rad)) | set(bits(cen[:, axis] - rad))
        on = (dc[: len(dc) // 2, axis] == 0)
        assert all(b in own for b in bits(oc[: len(dc) // 2, axis])[on])
        plain = set(bits(cen[:, axis]))
        assert sum(b in plain for b in bits(oc[: len(dc) // 2, axis])[on]) >= 0.6 * on.sum()
    # (D) starts inside spheres: every ray hits
    assert np.all(ref["sphere"][C == "D"] >= 0)
    # (F) either side of each bound of the guard
    f = a[C == "F"]
    of = np.abs(O[C == "F"]).max(axis=1).astype(np.float64)
    for v, bound in ((f, 2.0 ** -20), (f, 2.0 ** 60), (of, 2.0 ** 30)):
        assert ((v > bound * 0.99) & (v <= bound)).sum() >= 5
        assert ((v > bound) & (v < bound * 1.01)).sum() >= 5
    g = np.abs(O[C == "G"]).max(axis=1)
    assert (g > 2.0 ** 30).sum() >= 10 and (g <= 2.0 ** 30).sum() >= 10
    # hierarchy first hits
    t = tables_of(c)
    if t is not None:
        share = (np.isin(ref["sphere"], hierarchy_spheres(t)) & fin).sum() / fin.sum()
        print(f"{name}: hierarchy first hits {share:.3f}")
        assert share >= 0.15
    # both answers of the occlusion query occur, at the per-ray reach and at the default one
    for key in ("occ", "occ_default"):
        if name != "edge-nan-centre":
            assert 0.05 * fin.sum() <= ref[key][fin].sum() <= 0.95 * fin.sum(), key


# ------------------------------------------------------------------------------- sensitivity

def scan(scene, O, D, T=None, *, reverse=False, min_lt=False, max_lt=False, far_root=True,
         abs_radius=False, skip=()):
    """hit_sphere over the list (functions.glsl:14-40, 77-81) as ray_query_ref.first_hit (T
    None: the closest hit) and occlusion_ref.occluded_ref (T [n]: any hit below T) state it,
    with the switches of the mutants: (t, sphere, normal, occluded)."""
    O, D = np.asarray(O, np.float32), np.asarray(D, np.float32)
    n = len(O)
    ox, oy, oz = O[:, 0], O[:, 1], O[:, 2]
    dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]
    closest = T is None
    max_t = np.full(n, INFINITY, np.float32) if closest else np.asarray(T, np.float32)
    best = np.full(n, -1, np.int32)
    normal = np.zeros((n, 3), np.float32)
    occ = np.zeros(n, bool)
    below = (lambda x, y: x < y) if min_lt else (lambda x, y: x <= y)
    beyond = (lambda x, y: x < y) if max_lt else (lambda x, y: x <= y)
    order = range(len(scene) - 1, -1, -1) if reverse else range(len(scene))
    with np.errstate(all="ignore"):
        a = (dx * dx + dy * dy) + dz * dz
        for i in order:
            if i in skip:
                continue
            cx, cy, cz = (np.float32(v) for v in scene[i]["center"])
            r = np.float32(scene[i]["radius"])
            ocx, ocy, ocz = ox - cx, oy - cy, oz - cz
            half_b = (ocx * dx + ocy * dy) + ocz * dz
            cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - r * r
            disc = half_b * half_b - a * cc
            cand = ~(disc < 0)
            if not cand.any():
                continue
            sq = np.sqrt(disc)
            root = (-half_b - sq) / a
            far = cand & (below(root, MIN_T) | beyond(max_t, root))
            root2 = (-half_b + sq) / a
            root = np.where(far, root2, root)
            if far_root:
                take = cand & ~(far & (below(root2, MIN_T) | beyond(max_t, root2)))
            else:
                take = cand & ~far
            occ |= take
            if not closest or not take.any():
                continue
            max_t = np.where(take, root, max_t)
            best = np.where(take, np.int32(i), best)
            px, py, pz = root * dx + ox, root * dy + oy, root * dz + oz
            rr = np.abs(r) if abs_radius else r
            nr = np.stack([(px - cx) / rr, (py - cy) / rr, (pz - cz) / rr], axis=1)
            normal = np.where(take[:, None], nr, normal)
    return max_t, best, normal.astype(np.float32), occ


def _changed(base, got):
    """Rays whose record (first hit) or bit (occlusion) differs."""
    if len(base) == 1:
        return base[0] != got[0]
    return (bits(base[0]) != bits(got[0])) | (base[1] != got[1]) | \
        (bits(base[2]) != bits(got[2])).any(axis=1)


def test_mutants_of_the_references_are_visible(oracle):
    """Each mistake changes at least 10 contract rays over the cases (each named one at least 3
    in the cases the floor names): a kernel that made it would fail the GPU comparison."""
    total = {m: 0 for m in "abcdefgh"}
    named = {"a": 0, "e": 0, "h": 0}
    min_t_rays = 0
    for c in F.scene_cases(oracle):
        sc = c["scene"]
        O, D, C = F.rays(c)
        ref = F.reference(oracle, c)
        fin = ref["finite"]
        n = len(sc)
        # the copy above, unmutated, is the references
        hit0 = scan(sc, O, D)
        assert np.array_equal(bits(hit0[0]), bits(ref["t"])) and \
            np.array_equal(hit0[1], ref["sphere"]) and \
            np.array_equal(bits(hit0[2]), bits(ref["normal"])), c["name"]
        occ0 = scan(sc, O, D, ref["T"])[3]
        assert np.array_equal(occ0, ref["occ"]), c["name"]
        hit0, occ0 = hit0[:3], (occ0,)
        small = np.nonzero(F.geometry(sc)["ok"] &
                           (np.abs(sc["radius"]) <= 8 * F.geometry(sc)["rmed"]))[0]
        mutants = {"a": dict(reverse=True), "b": dict(min_lt=True), "c": dict(max_lt=True),
                   "d": dict(far_root=False), "e": dict(abs_radius=True),
                   "f": dict(skip=set(range(n - n % 4, n))),
                   "g": dict(skip=set(small[len(small) - len(small) // 4:].tolist()))}
        for m, kw in mutants.items():
            got = scan(sc, O, D, **kw)[:3]
            ch = _changed(hit0, got)
            if m == "b":
                min_t_rays += int(((ref["t"] != MIN_T) & fin & (got[0] == MIN_T)).sum())
            if m not in "ae":  # (ties and normals are no matter of the any-hit query)
                ch = ch | _changed(occ0, (scan(sc, O, D, ref["T"], **kw)[3],))
            k = int((ch & fin).sum())
            total[m] += k
            if (m == "a" and c["name"] == "edge-duplicates") or \
                    (m == "e" and c["family"] == "fuzz" and F.geometry(sc)["shells"]):
                named[m] += k
        h = int(((ref["occ"] != ref["occ_default"]) & fin).sum())
        total["h"] += h
        if c["kind"] == "scaled" and c["scale"] > 100:
            named["h"] += h
    print("changed rays per mutant:", total, "in the named cases:", named,
          "rays with a root of exactly min_t:", min_t_rays)
    assert all(v >= 10 for v in total.values()), total
    assert all(v >= 3 for v in named.values()), named
