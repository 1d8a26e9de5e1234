"""SceneGenerator surface (reference: SceneGenerator.cpp:10-56, globals.glsl:29-518).

Scenes are numpy structured arrays with the GLSL ``struct sphere`` layout
(structures.glsl:10-16): center[3], radius, colour[3], texture[3] -- 40 bytes per sphere.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N

SPHERE_DTYPE = np.dtype([
    ("center", np.float32, (3,)),
    ("radius", np.float32),
    ("colour", np.float32, (3,)),
    ("texture", np.float32, (3,)),
])
assert SPHERE_DTYPE.itemsize == ctypes.sizeof(N.vcrt_sphere) == 40

SCENES = {
    "final": N.SCENE_FINAL,        # 481 generated + big three + ground = 485
    "three": N.SCENE_THREE,        # big three + ground (globals.glsl:513-517)
    "red": N.SCENE_RED,            # red Lambertian sphere + ground (BASELINE config 1)
    "stress4096": N.SCENE_STRESS4096,  # 4096 generated + big three + ground = 4100
}


def builtin_scene(name_or_id) -> np.ndarray:
    """Spheres of a built-in scene, in world[] order."""
    sid = SCENES[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
    lib = N.lib()
    n = lib.vcrt_scene_builtin(sid, None, 0)
    if n < 0:
        raise N.VcrtError("vcrt_scene_builtin", n)
    arr = np.zeros(n, dtype=SPHERE_DTYPE)
    got = lib.vcrt_scene_builtin(sid, arr.ctypes.data_as(ctypes.POINTER(N.vcrt_sphere)), n)
    assert got == n
    return arr


def scene_generator_text() -> str:
    """The SceneGenerator executable's stdout, byte for byte."""
    lib = N.lib()
    n = lib.vcrt_scene_generator_text(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.vcrt_scene_generator_text(buf, n + 1)
    return buf.raw[:n].decode()


def make_spheres(rows) -> np.ndarray:
    """Build a scene from (center(3), radius, colour(3), material id, param) tuples."""
    arr = np.zeros(len(rows), dtype=SPHERE_DTYPE)
    for i, (c, r, col, mat, param) in enumerate(rows):
        arr[i]["center"] = c
        arr[i]["radius"] = r
        arr[i]["colour"] = col
        arr[i]["texture"] = (mat, param, 0.0)
    return arr


def cull_tables(spheres: np.ndarray) -> dict | None:
    """The culled scans' tables for `spheres` (host computation, no GPU): ``nbig`` big-sphere
    groups tested for every ray, then ``G`` hierarchy groups. ``geom`` [nbig + G, 16] pair-SoA
    groups and ``index`` [nbig + G, 4] world[] indices (-1 = padding), big groups first;
    ``bound`` [G/2, 12] hierarchy group-pair boxes, ``node`` [G/16, 12] node-pair boxes
    (node i = hierarchy groups 8i..8i+7), ``top`` chunk-pair boxes (entry i = hierarchy
    groups 64i..64i+63), ``margin`` the box-test constants (max |centre|, r_max^2, max |box
    coordinate|, 0). None when culling does not apply (< 16 spheres, unbounded)."""
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    lib = N.lib()
    ptr = spheres.ctypes.data
    nbig = ctypes.c_int32(0)
    g = lib.vcrt_cull_tables(ptr, len(spheres), None, None, None, None, None,
                             ctypes.byref(nbig), None, 0)
    if g == 0:
        return None
    nb = nbig.value
    geom = np.zeros((nb + g, 16), np.float32)
    bound = np.zeros((g // 2, 16), np.float32)
    node = np.zeros((g // 16, 16), np.float32)
    nt = (g + 63) // 64
    top = np.zeros(((nt + (nt & 1)) // 2, 16), np.float32)
    index = np.zeros((nb + g, 4), np.int32)
    margin = np.zeros(4, np.float32)
    got = lib.vcrt_cull_tables(ptr, len(spheres), geom.ctypes.data, bound.ctypes.data,
                               node.ctypes.data, top.ctypes.data, index.ctypes.data,
                               ctypes.byref(nbig), margin.ctypes.data, nb + g)
    assert got == g
    return {"nbig": nb, "geom": geom, "bound": bound, "node": node, "top": top, "index": index,
            "margin": margin}


def cull_slab(spheres: np.ndarray) -> tuple[np.float32, np.float32] | None:
    """The shared y slab of `spheres`' culling tables (host computation, no GPU): (lo.y, hi.y)
    when every group, node and chunk box with members has that same y extent bit for bit, so the
    flat scans evaluate the y planes once per ray; None otherwise, without culling tables, or
    with VCRT_SLAB=0 in the environment."""
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    lohi = np.zeros(2, np.float32)
    if N.lib().vcrt_cull_slab(spheres.ctypes.data, len(spheres), lohi.ctypes.data) == 0:
        return None
    return lohi[0], lohi[1]


def cull_footprint(spheres: np.ndarray) -> dict | None:
    """The footprint tables of `spheres`' node level (host computation, no GPU), as the LDS-table
    flat scan gets them: ``tables`` [4, N] uint32 node masks (x: lo <= cell, hi >= cell; then z),
    ``x`` / ``z`` the cells' (scale, offset) -- cell(X) = trunc(clamp(fma(X, scale, offset), 0,
    N - 1)) in fp32 --, ``y`` the y extent of the node boxes with members, ``k2`` twice their
    largest finite K and ``always`` the mask of nodes every ray keeps. None without culling
    tables. Independent of VCRT_SLAB."""
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    lib = N.lib()
    n = lib.vcrt_cull_footprint(spheres.ctypes.data, len(spheres), None, None, None)
    if n == 0:
        return None
    tables = np.zeros((4, n), np.uint32)
    par = np.zeros(8, np.float32)
    always = ctypes.c_uint32(0)
    lib.vcrt_cull_footprint(spheres.ctypes.data, len(spheres), tables.ctypes.data,
                            par.ctypes.data, ctypes.byref(always))
    return {"tables": tables, "x": par[0:2].copy(), "z": par[2:4].copy(), "y": par[4:6].copy(),
            "k2": par[6], "always": int(always.value)}


def cull_group_footprint(spheres: np.ndarray) -> dict | None:
    """The group-level footprint tables of `spheres` (host computation, no GPU), which take the
    node level's place in the LDS-table flat scan on eligible scenes: ``tables`` [4, N, 4] uint32,
    128-bit group masks, low word first (x: lo <= cell, hi >= cell; then z), ``n`` = N, ``x`` /
    ``z`` the cells' (scale, offset), ``y`` the y extent of the boxes with members, ``k2`` twice
    the group boxes' largest finite K, ``always`` [4] uint32 the groups every ray keeps, and
    ``eligible``: at most 128 groups, one y extent in every group box with members (whatever
    VCRT_SLAB says) and VCRT_GROUP_FOOT not 0. None without tables (no culling, more than 128
    groups)."""
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    lib = N.lib()
    n = lib.vcrt_cull_group_footprint(spheres.ctypes.data, len(spheres), None, None, None, None)
    if n == 0:
        return None
    tables = np.zeros((4, n, 4), np.uint32)
    par = np.zeros(8, np.float32)
    always = np.zeros(4, np.uint32)
    eligible = ctypes.c_int32(0)
    lib.vcrt_cull_group_footprint(spheres.ctypes.data, len(spheres), tables.ctypes.data,
                                  par.ctypes.data, always.ctypes.data, ctypes.byref(eligible))
    return {"tables": tables, "n": n, "x": par[0:2].copy(), "z": par[2:4].copy(),
            "y": par[4:6].copy(), "k2": par[6], "always": always,
            "eligible": bool(eligible.value)}


def primary_lists(spheres: np.ndarray, desc) -> dict | None:
    """The flat scan's camera-ray lists (host computation, no GPU; csrc/primary.cpp) for
    `spheres` and a RenderDesc: ``info`` [4 x local tiles] uint32, entry 4 lt + 2 qy + qx for the
    4x4-pixel quarter (qx, qy) of local tile lt (offset << 4 | count, count 15 = no list), and
    ``ids`` uint16 hierarchy group indices. None without culling tables."""
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    lib = N.lib()
    d = desc.to_c()
    n = lib.vcrt_primary_lists(spheres.ctypes.data, len(spheres), ctypes.byref(d), None, 0,
                               None, 0)
    if n < 0:
        return None
    from .renderer import tiles_for_rank
    nt = 4 * len(tiles_for_rank(desc.width, desc.height, desc.world_size, desc.rank))
    info = np.zeros(nt, np.uint32)
    ids = np.zeros(max(n, 1), np.uint16)
    got = lib.vcrt_primary_lists(spheres.ctypes.data, len(spheres), ctypes.byref(d),
                                 info.ctypes.data, nt, ids.ctypes.data, len(ids))
    assert got == n
    return {"info": info, "ids": ids[:n]}


def primary_sphere_lists(spheres: np.ndarray, desc) -> dict | None:
    """The camera fast trace's per-sphere lists (host computation, no GPU; csrc/primary.cpp):
    ``info`` [4 x local tiles] uint32 (first pair << 4 | spheres, 15 = no list) and ``rec``
    [pairs, 12] float32 camera-relative pair records (ocx0 ocx1 ocy0 ocy1 ocz0 ocz1 cc0 cc1
    index0 index1 0 0, the indices as int32 bits). None without culling tables."""
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    lib = N.lib()
    d = desc.to_c()
    n = lib.vcrt_primary_sphere_lists(spheres.ctypes.data, len(spheres), ctypes.byref(d), None,
                                      0, None, 0)
    if n < 0:
        return None
    from .renderer import tiles_for_rank
    nt = 4 * len(tiles_for_rank(desc.width, desc.height, desc.world_size, desc.rank))
    info = np.zeros(nt, np.uint32)
    rec = np.zeros((max(n, 1), 12), np.float32)
    got = lib.vcrt_primary_sphere_lists(spheres.ctypes.data, len(spheres), ctypes.byref(d),
                                        info.ctypes.data, nt, rec.ctypes.data, rec.size)
    assert got == n
    return {"info": info, "rec": rec[:n]}


def table_from_bytes(name: str, raw: np.ndarray):
    """The bytes of a scene table (`_native.SCENE_TABLES`) as a flat array of its words, or for
    "scalars" a dict of the vcrt_scene_scalars fields (arrays as tuples; floats as np.float32, so
    two dicts compare equal exactly when the bytes do, NaN aside)."""
    _, dtype = N.SCENE_TABLES[name]
    if name != "scalars":
        return np.frombuffer(raw.tobytes(), dtype=dtype).copy()
    s = N.vcrt_scene_scalars.from_buffer_copy(raw.tobytes())
    out = {}
    for field, ctype in N.vcrt_scene_scalars._fields_:
        v = getattr(s, field)
        if hasattr(v, "__len__"):
            out[field] = tuple(np.float32(x) if ctype._type_ is ctypes.c_float else int(x)
                               for x in v)
        else:
            out[field] = np.float32(v) if ctype is ctypes.c_float else int(v)
    return out


def refit_table(grouping_of: np.ndarray, values: np.ndarray, name: str):
    """One device table as a refit computes it (host computation, no GPU;
    vcrt_scene_table_host): the grouping set_scene(grouping_of) chooses, filled with `values`
    (same count) -- what Renderer.update_spheres(values) leaves on the device of a renderer whose
    scene was set to `grouping_of`. With values == grouping_of, what set_scene uploads. The form
    of Renderer.scene_table; None when the table does not exist."""
    grouping_of = np.ascontiguousarray(grouping_of, dtype=SPHERE_DTYPE)
    values = np.ascontiguousarray(values, dtype=SPHERE_DTYPE)
    if len(values) != len(grouping_of):
        raise ValueError("values and grouping_of must hold the same number of spheres")
    tid, _ = N.SCENE_TABLES[name]
    lib = N.lib()
    n = lib.vcrt_scene_table_host(grouping_of.ctypes.data, values.ctypes.data, len(values), tid,
                                  None, 0)
    if n <= 0:
        return None
    buf = np.zeros(n, np.uint8)
    lib.vcrt_scene_table_host(grouping_of.ctypes.data, values.ctypes.data, len(values), tid,
                              buf.ctypes.data, n)
    return table_from_bytes(name, buf)


def refit_camera_lists(grouping_of: np.ndarray, values: np.ndarray, desc) -> dict | None:
    """primary_lists and primary_sphere_lists over refitted tables (refit_table's), in the form
    of Renderer.camera_lists: group_info, ids, sphere_info, rec. None without culling tables."""
    grouping_of = np.ascontiguousarray(grouping_of, dtype=SPHERE_DTYPE)
    values = np.ascontiguousarray(values, dtype=SPHERE_DTYPE)
    lib = N.lib()
    d = desc.to_c()
    args = (grouping_of.ctypes.data, values.ctypes.data, len(values), ctypes.byref(d))
    nids = lib.vcrt_refit_primary_lists(*args, None, 0, None, 0)
    npairs = lib.vcrt_refit_primary_sphere_lists(*args, None, 0, None, 0)
    if nids < 0 or npairs < 0:
        return None
    from .renderer import tiles_for_rank
    nt = 4 * len(tiles_for_rank(desc.width, desc.height, desc.world_size, desc.rank))
    ginfo, sinfo = np.zeros(nt, np.uint32), np.zeros(nt, np.uint32)
    ids = np.zeros(max(nids, 1), np.uint16)
    rec = np.zeros((max(npairs, 1), 12), np.float32)
    lib.vcrt_refit_primary_lists(*args, ginfo.ctypes.data, nt, ids.ctypes.data, len(ids))
    lib.vcrt_refit_primary_sphere_lists(*args, sinfo.ctypes.data, nt, rec.ctypes.data, rec.size)
    return {"group_info": ginfo, "ids": ids[:nids], "sphere_info": sinfo, "rec": rec[:npairs]}
