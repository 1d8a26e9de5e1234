"""The nine statistics kernels (VCRT_DEBUG_STATS=1: the *_stats instantiations of trace_impl with
kStats = true) held to the product kernels' bar, and their counters pinned.

Every frame rendered here is, with no tolerance anywhere, the oracle's image bit for bit (NaN
positions coinciding) with the oracle's segment count, from the kernel named product symbol +
"_stats", in the static order (cost_order 0: capi.cpp trace_frame keeps the cost order off for
g.debug_stats == 1). On every such frame `counter_violations` checks the identities below; they are
derived from the kernel text (csrc/tracer.hip trace_impl, `P` = the rank's in-frame pixels, G, K, T,
KT = accumulate_quantum, _chunk, _tail, _tail_chunk of the frame's stats, spp = the launch's
samples; debug[] describes the last launch only).

The per-wave counters (PhaseTicks, st_*) credit a wave-uniform amount to the wave's first active
lane (`credit`), or each lane's own amount to the lane (the camera trace's list_sum and root_sum),
and are summed over the lanes after the loop, so a counter is the wave's whole count whichever
lanes were idle when it moved (a lane that is `done` skips everything after `if (done) continue`,
so the code after it runs with part of the wave and reduces by ballots, not by xor butterflies).

 waves          debug[7] += 1 by lane 0 of every wave after the loop:
                debug[7] == grid_blocks * block_threads / 64.
 blocks         ++pt.blk_fetches and region kBlock sit together behind the `b == ~0u` break of the
                fetch loop: one per block taken. A queue hands out k < nq exactly once each, so
                debug[34] == kBlock == total_blocks = local_tiles * (ceil((spp - T) / K) +
                (ceil(T / KT) if T)) (capi.cpp: g.nchunks, g.tail_nchunks; trace_frame's
                total_blocks).
 quanta         pt.quanta += popc(ballot(fin)) at the loop top. fin is set in shade_and_advance once
                per finished quantum (sample == sample_end, or sample & quantum_mask == 0) and
                cleared by the retire; items hold whole quanta and a stolen range starts on a
                quantum boundary, so debug[39] == P * ceil(spp / G) (== P on the direct path).
 retire         pt.retire_iters += (ballot(fin) != 0) and region kRetire inside `if (fin)`, the same
                condition: debug[38] == kRetire.
 camera entries ++pt.cam_entries and region kCam both under `if (__ballot(cam_now))`:
                debug[24] == kCam.
 camera loops   region kCamListTrip / kCamRootTrip at the top of every trip of the listed-pair /
                root loop, which the wave runs as often as its busiest lane (iters, roots);
                pt.list_trips / pt.root_trips add that maximum per entry:
                debug[27] == kCamListTrip, debug[29] == kCamRootTrip (flat kernels).
 iterations     region kIter at the top of every trip of the persistent loop; ++st_iters after the
                loop's only exit (`if (live == 0) break`), so a wave counts one more kIter than
                st_iters: kIter == debug[0] + debug[7].
 items          pt.items_cur += popc(ballot(got)); got is set once per in-frame item slot handed out
                and once per steal; region kSteal counts every trip of the steal loop (one steal at
                most): P * ipp <= debug[35] <= P * ipp + kSteal, ipp = items per pixel.
 live lanes     st_active += popc(ballot(!done)) per counted iteration. In the four kernels that are
                not flat every lane that is not done holds an item after the fetch loop (it ends
                when no lane needs one) and scans once: debug[1] == segments. In the flat kernels a
                lane may wait for a deferred fetch and a camera ray is traced in the camera phase
                before the lane's main scan of the same iteration: camera-phase segments are
                debug[25], main-scan segments at most debug[1] and at least the main-scan hits
                debug[31]: debug[25] + debug[31] <= segments <= debug[1] + debug[25].
 linear scans   tally(w_halves, 2 * ceil(n / 4)) once per iteration that scans, and every counted
                iteration scans: group_tests == debug[0] * ceil(n / 4) (LDS, SMEM).
 bounds         popcounts of ballots and per-entry maxima against their lane sums:
                debug[1] <= 64 debug[0]; debug[31] <= debug[1]; debug[25] <= debug[26] <= 64
                debug[24]; debug[27] <= debug[28] <= 64 debug[27]; debug[29] <= debug[30] <= 64
                debug[29]; sphere_tests == segments * nspheres (capi.cpp vcrt_draw_next_frame).
 LDS-table scan debug[36], [37] = pt.group_entries, pt.node_entries (flat_drain kinds 1 and 2,
                kFmt == 0 only). With the group footprint (kGroupsOnly) kinds 2 and 3 never run and
                nothing adds to n_bounds: debug[36] > 0, debug[37] == 0, bound_tests == 0,
                kLevelNodes == 0 < kLevelGroups on every frame where the host says the footprint
                is in effect (vcrt_cull_group_footprint's eligible, camera-ray lists on); else
                the node level runs: debug[37] > 0, bound_tests > 0, kLevelGroups == 0 <
                kLevelNodes. The other kernels leave both 0.

The camera fast trace has a reference outside the kernel, the host's per-quarter sphere lists
(vcrt_primary_sphere_lists): a camera ray enters it (cam_now) when it is `fresh` at the camera
phase, its quarter has a list (info & 15 != 15) and it is in the guarded range, and runs
ceil((info & 15) / 2) trips of the listed-pair loop. A ray is fresh there when it starts an item (or
a stolen range) or follows a sample that ended in the main scan's sky shading (defer_ray: the
next fetch sets it up). A sample that ends in the camera phase's shading starts its successor
inside shade_and_advance and that ray goes straight through the same iteration's main scan, so
with several samples per item the listed pixels give bounds only,
    ipp * L <= debug[25] <= spp * L,   ipp * S <= debug[28] <= spp * S
(L = listed in-frame pixels, S = their sum of ceil((info & 15) / 2)), exact when every sample is
its own item (chunk 1, quantum 1): debug[25] == spp * L and debug[28] == spp * S.
"""
import math

import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import group_footprint_ref as G
from tests.stats_layout import dbg, region
from tests.test_gpu_group_footprint import CASES as G_CASES
from tests.test_gpu_lens import assert_same
from tests.test_gpu_parity import culling_torture_scene
from vulkancomputeraytracing_amd.scene import (builtin_scene, cull_group_footprint,
                                               primary_sphere_lists)

pytestmark = pytest.mark.gpu
N = vc._native

# every switch a case may set, cleared first so that a case sees its own settings only
ENV = ("VCRT_DEBUG_STATS", "VCRT_STAGE_TABLES", "VCRT_CULL_LANE_TABLES", "VCRT_ACCUM_RING",
       "VCRT_GROUP_FOOT", "VCRT_PRIMARY_LISTS", "VCRT_WORK_ORDER", "VCRT_SLAB", "VCRT_ITEM_ORDER")

THREE = ("three", 37, 23, 3, 5)          # ragged edges; one quantum per pixel: the direct path
FINAL = ("final", 44, 20, 8, 6)          # both frame edges partial, two quanta of G = 4 per pixel
STRESS = ("stress4096", 24, 16, 4, 4)
TORTURE_CAM = dict(lookfrom=(6, 2.5, 5), lookat=(0, 0.6, 0), vfov=45)

SCENES = {
    "torture": culling_torture_scene,
    "grid128": G.grid128, "grid129": G.grid129, "sliced": G.tiny_grid,
}

ceil_div = lambda a, b: -(-a // b)  # noqa: E731


def scene_arrays(oracle, scene):
    """(what the renderer gets, what the oracle gets) for a scene name."""
    if scene in ("bright", "overflow"):
        sc = oracle.bright_scene(3.0 if scene == "bright" else 1e20)
        return sc, sc
    if scene in SCENES:
        sc = SCENES[scene]()
        return sc, sc
    return scene, oracle.scene(scene)


_want = {}


def reference(oracle, scene, w, h, spp_total, depth, part, cam, frame_spp=0):
    """The oracle's (image, segments), computed once per image: it depends on the quantum alone."""
    key = (scene, w, h, spp_total, depth, part["quantum"], frame_spp, tuple(sorted(cam.items())))
    if key not in _want:
        cfg = oracle.config(w, h, spp_total, depth, frame_spp=frame_spp, **part, **cam)
        _want[key] = oracle.render(cfg, scene_arrays(oracle, scene)[1])
    return _want[key]


def kind_of(kernel):
    if kernel in ("vcrt_trace_lds_stats", "vcrt_trace_smem_stats"):
        return "linear"
    return "flat" if "cull_flat" in kernel else "culled"


def counter_violations(st, pixels, spp, segments, listed=None, foot=False):
    """The identities of the module docstring that one stats-build launch breaks (a list of
    strings, empty when all hold). pixels: the rank's in-frame pixels; segments: the oracle's for
    those pixels and samples; listed: (L, S) of the camera-ray lists, for a flat kernel's frame;
    foot: the frame takes its groups from the group footprint (the LDS-table kernel only)."""
    bad = []

    def check(ok, what):
        if not ok:
            bad.append(what)

    d = st["debug"]
    g, k, t, kt = (st["accumulate_quantum"], st["accumulate_chunk"], st["accumulate_tail"],
                   st["accumulate_tail_chunk"])
    ipp = ceil_div(spp - t, k) + (ceil_div(t, kt) if t else 0)
    kind = kind_of(st["kernel"])
    groups4 = ceil_div(st["nspheres"], 4)
    check(d[7] == st["grid_blocks"] * st["block_threads"] // 64,
          f"waves: debug[7] {d[7]} != {st['grid_blocks']} x {st['block_threads']} / 64")
    blocks = st["local_tiles"] * ipp
    check(d[34] == blocks, f"block fetches: debug[34] {d[34]} != {blocks}")
    check(region(st, "kBlock") == blocks, f"kBlock {region(st, 'kBlock')} != {blocks}")
    quanta = pixels * ceil_div(spp, g)
    check(d[39] == quanta, f"quanta retired: debug[39] {d[39]} != {quanta}")
    check(d[38] == region(st, "kRetire"), f"debug[38] {d[38]} != kRetire {region(st, 'kRetire')}")
    check(d[24] == region(st, "kCam"), f"debug[24] {d[24]} != kCam {region(st, 'kCam')}")
    check(region(st, "kIter") == d[0] + d[7],
          f"kIter {region(st, 'kIter')} != debug[0] + debug[7] = {d[0]} + {d[7]}")
    check(pixels * ipp <= d[35] <= pixels * ipp + region(st, "kSteal"),
          f"items: {pixels * ipp} <= debug[35] {d[35]} <= + kSteal {region(st, 'kSteal')}")
    check(region(st, "kItem") <= d[35], f"kItem {region(st, 'kItem')} > debug[35] {d[35]}")
    check(st["segments"] == segments, f"segments {st['segments']} != {segments}")
    check(st["sphere_tests"] == segments * st["nspheres"], "sphere_tests != segments * nspheres")
    if kind == "flat":
        check(d[25] + d[31] <= segments <= d[1] + d[25],
              f"flat segments: {d[25]} + {d[31]} <= {segments} <= {d[1]} + {d[25]}")
    else:
        check(d[1] == segments, f"live lanes: debug[1] {d[1]} != segments {segments}")
        check(d[24] == d[25] == d[26] == 0, "camera counters outside the flat kernels")
    if kind == "linear":
        check(st["group_tests"] == d[0] * groups4,
              f"group_tests {st['group_tests']} != debug[0] {d[0]} x {groups4}")
        check(st["bound_tests"] == 0, "bound_tests of a linear scan")
    check(d[1] <= 64 * d[0], "debug[1] > 64 debug[0]")
    check(d[31] <= d[1], "debug[31] > debug[1]")
    check(d[25] <= d[26] <= 64 * d[24], f"camera lanes: {d[25]} <= {d[26]} <= 64 x {d[24]}")
    check(d[27] <= d[28] <= 64 * d[27], f"listed loop: {d[27]} <= {d[28]} <= 64 x {d[27]}")
    check(d[29] <= d[30] <= 64 * d[29], f"root loop: {d[29]} <= {d[30]} <= 64 x {d[29]}")
    if kind == "flat":  # the loops' wave-level trips, counted by both mechanisms
        check(d[27] == region(st, "kCamListTrip"),
              f"debug[27] {d[27]} != kCamListTrip {region(st, 'kCamListTrip')}")
        check(d[29] == region(st, "kCamRootTrip"),
              f"debug[29] {d[29]} != kCamRootTrip {region(st, 'kCamRootTrip')}")
    if st["kernel"] == "vcrt_trace_cull_flat_stats":
        levels = f"debug[36] {d[36]}, debug[37] {d[37]}, bound_tests {st['bound_tests']}, " \
                 f"kLevelGroups {region(st, 'kLevelGroups')}, kLevelNodes " \
                 f"{region(st, 'kLevelNodes')}"
        check(d[36] > 0, "debug[36] == 0 from the LDS-table kernel")
        if foot:  # no node level, no box test
            check(d[37] == 0 and st["bound_tests"] == 0 and region(st, "kLevelNodes") == 0 and
                  region(st, "kLevelGroups") > 0, "group footprint: " + levels)
        else:
            check(d[37] > 0 and st["bound_tests"] > 0 and region(st, "kLevelNodes") > 0 and
                  region(st, "kLevelGroups") == 0, "node level: " + levels)
    else:
        check(d[36] == 0 and d[37] == 0, "debug[36], [37] from another kernel")
    if listed is not None:
        lp, ls = listed
        check(ipp * lp <= d[25] <= spp * lp, f"camera rays: {ipp * lp} <= {d[25]} <= {spp * lp}")
        check(ipp * ls <= d[28] <= spp * ls, f"listed trips: {ipp * ls} <= {d[28]} <= {spp * ls}")
        if k == 1 and g == 1:  # every sample starts an item: exact
            check(d[25] == spp * lp, f"camera rays: debug[25] {d[25]} != {spp} x {lp}")
            check(d[28] == spp * ls, f"listed trips: debug[28] {d[28]} != {spp} x {ls}")
    return bad


def listed_pixels(scene_arr, desc, mine, local_index):
    """(L, S) from the host's camera-ray sphere lists: the in-frame pixels of the rank whose 4x4
    quarter has a list, and their sum of listed pairs ceil(count / 2). None: no lists."""
    arr = builtin_scene(scene_arr) if isinstance(scene_arr, str) else scene_arr
    lists = primary_sphere_lists(arr, desc)
    if lists is None:
        return None
    y, x = np.nonzero(mine)
    quarter = 4 * (local_index[mine] // 64) + 2 * ((y % 8) // 4) + (x % 8) // 4
    cnt = lists["info"][quarter] & 15
    has = cnt != 15
    return int(has.sum()), int(((cnt[has] + 1) // 2).sum())


def group_footprint_in_effect(scene_arr, env):
    """Whether a pinhole frame of the scene takes its groups from the group footprint, from the
    host: the scene has the tables and is eligible (VCRT_GROUP_FOOT, read from the environment
    now, included), and the renderer has its camera-ray lists (capi.cpp trace_frame)."""
    arr = builtin_scene(scene_arr) if isinstance(scene_arr, str) else scene_arr
    gf = cull_group_footprint(arr)
    return gf is not None and gf["eligible"] and env.get("VCRT_PRIMARY_LISTS") != "0"


def stats_frames(oracle, monkeypatch, case, variant, kernel, env=None, cam=None, frames=1,
                 stats="1", **desc_kw):
    """Renders `case` with VCRT_DEBUG_STATS (and `env`), checks every frame's image, segments,
    kernel name, order and counters, and returns the frames' stats."""
    scene, w, h, spp, depth = case
    cam = cam or {}
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VCRT_DEBUG_STATS", stats)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    gpu_scene, _ = scene_arrays(oracle, scene)
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=variant, **cam, **desc_kw)
    world, rank = desc.world_size, desc.rank
    m = vc.tile_pixel_map(w, h, world)
    mine = m[..., 0] == rank
    out = []
    with vc.Renderer(desc, gpu_scene) as r:
        for f in range(frames):
            r.draw_next_frame()
            got, st = r.read_framebuffer(), r.stats()
            what = f"{case} v{variant} {env} {desc_kw} frame {f}"
            total = (f + 1) * spp if desc.progressive else spp
            want, segs = reference(oracle, scene, w, h, total, depth, oracle.partition(st), cam,
                                   frame_spp=spp if desc.progressive else 0)
            if world > 1:
                got, want = got.reshape(-1, 4)[m[..., 1][mine]], want[mine]
            assert_same(got, want, what)
            assert st["kernel"] == kernel + "_stats", what
            assert st["cost_order"] == 0, what
            # this launch's segments: a rank's own pixels, a progressive frame's own samples
            if world > 1:
                cfg = oracle.config(w, h, spp, depth, **oracle.partition(st), **cam)
                yx = np.argwhere(mine)
                segs = oracle.render_pixels(cfg, scene_arrays(oracle, scene)[1], yx[:, ::-1])[1]
            elif desc.progressive and f > 0:
                segs -= reference(oracle, scene, w, h, f * spp, depth, oracle.partition(st), cam,
                                  frame_spp=spp)[1]
            listed = None
            if kind_of(st["kernel"]) == "flat" and (env or {}).get("VCRT_PRIMARY_LISTS") != "0":
                listed = listed_pixels(gpu_scene, desc, mine, m[..., 1])
            foot = group_footprint_in_effect(gpu_scene, env or {})
            bad = counter_violations(st, int(mine.sum()), spp, segs, listed, foot)
            assert not bad, f"{what}: " + "; ".join(bad) + f"\ndebug {st['debug']}"
            out.append(st)
    return out


# ---- (a) every stats kernel, by name ---------------------------------------------------------

KERNELS = [
    ("lds", THREE, N.KERNEL_LDS, {}, "vcrt_trace_lds"),
    ("smem", THREE, N.KERNEL_SMEM, {}, "vcrt_trace_smem"),
    ("smem-unstaged", THREE, N.KERNEL_SMEM, {"VCRT_STAGE_TABLES": "0"}, "vcrt_trace_smem"),
    ("cull", FINAL, N.KERNEL_CULL, {}, "vcrt_trace_cull"),
    ("lane-lds", FINAL, N.KERNEL_CULL_LANE, {}, "vcrt_trace_cull_lane_lds"),
    ("lane-global", FINAL, N.KERNEL_CULL_LANE, {"VCRT_CULL_LANE_TABLES": "global"},
     "vcrt_trace_cull_lane"),
    ("flat", FINAL, N.KERNEL_CULL_FLAT, {}, "vcrt_trace_cull_flat"),
    ("auto", FINAL, N.KERNEL_AUTO, {}, "vcrt_trace_cull_flat"),
    ("flat-global", FINAL, N.KERNEL_CULL_FLAT, {"VCRT_CULL_LANE_TABLES": "global"},
     "vcrt_trace_cull_flat_global"),
    ("flat-boxes", FINAL, N.KERNEL_CULL_FLAT, {"VCRT_CULL_LANE_TABLES": "boxes"},
     "vcrt_trace_cull_flat_boxes"),
    ("stress-lane-wide", STRESS, N.KERNEL_CULL_LANE, {}, "vcrt_trace_cull_lane_lds_wide"),
    ("stress-auto", STRESS, N.KERNEL_AUTO, {}, "vcrt_trace_cull_flat_boxes"),
]


@pytest.mark.parametrize("case,variant,env,kernel", [k[1:] for k in KERNELS],
                         ids=[k[0] for k in KERNELS])
def test_every_stats_kernel(oracle, monkeypatch, case, variant, env, kernel):
    (st,) = stats_frames(oracle, monkeypatch, case, variant, kernel, env)
    if kernel == "vcrt_trace_cull_flat":  # the final scene takes the group footprint
        assert group_footprint_in_effect("final", env)
        assert dbg(st, "node_pass_entries") == 0 and st["bound_tests"] == 0


# ---- (b) modes on the LDS-table flat stats kernel ---------------------------------------------

FLAT = (N.KERNEL_CULL_FLAT, "vcrt_trace_cull_flat")


def test_progressive(oracle, monkeypatch):
    scene, w, h, _, depth = FINAL
    s1, s2 = stats_frames(oracle, monkeypatch, (scene, w, h, 4, depth), *FLAT, frames=2,
                          progressive=True)
    assert (s1["accumulated_spp"], s2["accumulated_spp"]) == (4, 8)


def test_tail_partition(oracle, monkeypatch):
    scene, w, h, _, depth = FINAL
    (st,) = stats_frames(oracle, monkeypatch, (scene, w, h, 16, depth), *FLAT, accumulate_chunk=8,
                         accumulate_tail=4, accumulate_tail_chunk=4, accumulate_quantum=4)
    assert oracle.partition(st) == dict(chunk=8, tail=4, tail_chunk=4, quantum=4)


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_shards(oracle, monkeypatch, rank):
    stats_frames(oracle, monkeypatch, FINAL, *FLAT, rank=rank, world_size=3)


@pytest.mark.parametrize("ring", ["1", "0"])
def test_accumulation_ring(oracle, monkeypatch, ring):
    """Ring on: the quanta go through the wave's LDS entries (kRetireRing); off: every quantum
    is added to global memory (kRetireGlobal). Two items of one quantum per pixel: a block of
    64 items then covers 32 pixels, which fit the 63 entries of a wave's ring (with one item
    per pixel, the rule's partition at this size, a block's 64 pixels do not and even a ring-on
    frame adds every quantum to global memory)."""
    (st,) = stats_frames(oracle, monkeypatch, FINAL, *FLAT, env={"VCRT_ACCUM_RING": ring},
                         accumulate_chunk=4, accumulate_quantum=4, accumulate_tail=-1)
    assert (st["accumulate_chunk"], st["accumulate_tail"]) == (4, 0)
    if ring == "1":
        assert st["ring_entries"] >= 8 and region(st, "kRetireRing") > 0
    else:
        assert st["ring_entries"] == 0 and region(st, "kRetireRing") == 0
        assert region(st, "kRetireGlobal") == region(st, "kRetire") > 0


def test_bright_scene_outlier_rerender(oracle, monkeypatch):
    """The outlier retire: the first render of the draw meets quantum sums past 2^12
    (kRetireNan, the only code that writes outlier_max) and the frame is rendered again with
    each pixel at its own scale. debug[] describes the last launch, the re-render, which the
    counters are checked on and which meets no outlier (kRetireNan == 0): the first render's
    entry into the path shows as scale_rerenders. Depth 12: at depth 8 the pinhole's largest
    quantum sum of this 24x16x16 frame is 2436 (the oracle's), below 2^12, and nothing is
    rendered again; at depth 12 it is 9.9e4."""
    (st,) = stats_frames(oracle, monkeypatch, ("bright", 24, 16, 16, 12), *FLAT)
    assert st["scale_rerenders"] >= 1 and st["accumulate_scale_log2"] < 32
    assert region(st, "kRetireNan") == 0 and region(st, "kRetire") > 0


def test_non_finite_quanta_enter_the_outlier_retire(oracle, monkeypatch):
    """The region counter of the outlier retire itself: with a reflect ratio of 1e20 some paths'
    attenuation overflows fp32, their quantum sums are infinite and their pixels NaN in the
    oracle too. Such a quantum takes the kRetireNan branch on every render (it records no
    maximum: no scale helps), so the last launch shows it."""
    (st,) = stats_frames(oracle, monkeypatch, ("overflow", 24, 16, 16, 8), *FLAT)
    want, _ = reference(oracle, "overflow", 24, 16, 16, 8, oracle.partition(st), {})
    assert np.isnan(want).any()
    assert region(st, "kRetireNan") > 0


def test_group_footprint_off(oracle, monkeypatch):
    (st,) = stats_frames(oracle, monkeypatch, FINAL, *FLAT, env={"VCRT_GROUP_FOOT": "0"})
    assert dbg(st, "node_pass_entries") > 0 and st["bound_tests"] > 0
    assert region(st, "kLevelNodes") > 0 and region(st, "kLevelGroups") == 0


# ---- (d) the camera fast trace against the host's lists --------------------------------------

@pytest.mark.parametrize("tables,kernel", [(None, "vcrt_trace_cull_flat"),
                                           ("global", "vcrt_trace_cull_flat_global"),
                                           ("boxes", "vcrt_trace_cull_flat_boxes")])
def test_camera_fast_trace_against_host_lists(oracle, monkeypatch, tables, kernel):
    """Every sample its own item (chunk 1, quantum 1): each camera ray starts an item, so the
    fast trace takes exactly the rays of the listed quarters and runs exactly their listed pairs
    (counter_violations: debug[25] == spp * L, debug[28] == spp * S)."""
    env = {"VCRT_CULL_LANE_TABLES": tables} if tables else {}
    (st,) = stats_frames(oracle, monkeypatch, FINAL, N.KERNEL_CULL_FLAT, kernel, env,
                         accumulate_chunk=1, accumulate_quantum=1, accumulate_tail=-1)
    assert (st["accumulate_chunk"], st["accumulate_quantum"]) == (1, 1)
    assert dbg(st, "cam_lanes") > 0 and dbg(st, "list_sum") > 0


def test_camera_lists_off(oracle, monkeypatch):
    (st,) = stats_frames(oracle, monkeypatch, FINAL, *FLAT, env={"VCRT_PRIMARY_LISTS": "0"})
    assert dbg(st, "cam_entries") == 0 and region(st, "kCam") == 0


# ---- (e) the paths existing cases claim to reach ---------------------------------------------

@pytest.mark.parametrize("case", ["sliced", "grid128", "grid129"])
def test_group_footprint_paths(oracle, monkeypatch, case):
    """tests/test_gpu_group_footprint.py's cases: the sliced push, the group level with no node
    level at exactly 128 groups, the node level at 129."""
    _, w, h, spp, depth, cam, _ = G_CASES[case]
    (st,) = stats_frames(oracle, monkeypatch, (case, w, h, spp, depth), *FLAT, cam=cam)
    if case == "sliced":
        assert region(st, "kSliceGroups") > 0
    if case == "grid129":
        assert region(st, "kLevelNodes") > 0 and region(st, "kLevelGroups") == 0
    else:
        assert region(st, "kLevelGroups") > 0 and region(st, "kLevelNodes") == 0


CULLED = [(N.KERNEL_CULL, "vcrt_trace_cull"), (N.KERNEL_CULL_LANE, "vcrt_trace_cull_lane_lds"),
          FLAT]


@pytest.mark.parametrize("variant,kernel", CULLED)
def test_torture_scene(oracle, monkeypatch, variant, kernel):
    """test_culled_scan_torture_scene (33, 21, 5, 50, 5) through the culled stats kernels. Every
    ray of it stays in the guarded range: every scan is a culled one (kScan), none falls back to
    the linear scan (measured: kScanLinear 0 in all three kernels), so this scene is no evidence
    for that path; test_linear_fallback_in_a_culled_kernel has one that is."""
    (st,) = stats_frames(oracle, monkeypatch, ("torture", 33, 21, 5, 50), variant, kernel,
                         cam=TORTURE_CAM, accumulate_chunk=5, accumulate_quantum=1)
    assert region(st, "kScan") > 0


@pytest.mark.parametrize("variant,kernel", CULLED)
def test_linear_fallback_in_a_culled_kernel(oracle, monkeypatch, variant, kernel):
    """The tiny grid of test_gpu_group_footprint's `sliced` case (coordinates scaled by 2^-24):
    its camera rays have |d|^2 below the guarded range's 2^-20, so a wave that holds one scans the
    whole list inside the culled kernel (kScanLinear), while the bounced rays, of unit length,
    take the culled scan (kScan)."""
    _, w, h, spp, depth, cam, _ = G_CASES["sliced"]
    (st,) = stats_frames(oracle, monkeypatch, ("sliced", w, h, spp, depth), variant, kernel,
                         cam=cam)
    assert region(st, "kScanLinear") > 0 and region(st, "kScan") > 0
    assert region(st, "kCam") == 0  # no camera ray is in the fast trace's guarded range


def test_steal(oracle, monkeypatch):
    """One long item per pixel: once the queues are empty, idle lanes take later quanta of the
    wave's longest item (kSteal), and every quantum still retires once."""
    (st,) = stats_frames(oracle, monkeypatch, ("final", 24, 16, 64, 6), *FLAT,
                         accumulate_chunk=64, accumulate_quantum=4, accumulate_tail=-1)
    assert region(st, "kSteal") > 0
    assert dbg(st, "items_started") > 24 * 16  # some trip of the steal loop handed a range out


# ---- (f) the product's issued-work counter ---------------------------------------------------

@pytest.mark.parametrize("variant,kernel", [(N.KERNEL_LDS, "vcrt_trace_lds"),
                                            (N.KERNEL_SMEM, "vcrt_trace_smem")])
def test_product_group_tests_bound(oracle, monkeypatch, variant, kernel):
    """No stats: the linear scans tally ceil(n / 4) group tests per wave-iteration, an iteration
    scans between 1 and 64 segments."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    scene, w, h, spp, depth = THREE
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0,
                         kernel_variant=variant)
    with vc.Renderer(desc, scene) as r:
        r.draw_next_frame()
        st = r.stats()
    _, segs = reference(oracle, scene, w, h, spp, depth, oracle.partition(st), {})
    assert st["kernel"] == kernel and st["segments"] == segs
    groups4 = ceil_div(st["nspheres"], 4)
    assert math.ceil(segs / 64) * groups4 <= st["group_tests"] <= segs * groups4


# ---- (g) VCRT_DEBUG_STATS=2: the product kernels with a debug buffer -------------------------

def test_debug_stats_2_runs_the_product_kernel(oracle, monkeypatch):
    scene, w, h, spp, depth = FINAL
    desc = vc.RenderDesc(width=w, height=h, samples_per_pixel=spp, max_depth=depth, device=0)
    frames = []
    for value in (None, "2"):
        for name in ENV:
            monkeypatch.delenv(name, raising=False)
        if value:
            monkeypatch.setenv("VCRT_DEBUG_STATS", value)
        with vc.Renderer(desc, scene) as r:
            r.draw_next_frame()
            frames.append((r.read_framebuffer(), r.stats()))
    (want, st0), (got, st2) = frames
    assert_same(got, want, "VCRT_DEBUG_STATS=2 against the product frame")
    assert st2["segments"] == st0["segments"]
    assert st2["kernel"] == st0["kernel"] and "_stats" not in st2["kernel"]
    want_o, segs = reference(oracle, scene, w, h, spp, depth, oracle.partition(st0), {})
    assert_same(want, want_o, "the product frame against the oracle")
    assert st0["segments"] == segs

