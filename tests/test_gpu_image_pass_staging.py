"""The host forms of the five image passes share one pool of staging planes (csrc/pass_staging.hpp,
RendererState.staging), kept and grown only. One renderer runs reproject,
reproject_moments, variance, denoise and denoise_variance in turn on host planes, at the largest
shape of variance_ref.SHAPES, then the smallest, then the largest again; every output equals the
corresponding *_host function's bit for bit. A plane left at a stale size, an output sharing a
buffer with an input, or one call reading what the call before it left behind would show here."""
import numpy as np
import pytest

import vulkancomputeraytracing_amd as vc
from tests import denoise_ref as D
from tests import reproject_ref as P
from tests import variance_ref as V
from tests.test_gpu_variance import host_renderer, same

pytestmark = pytest.mark.gpu

LARGEST = max(V.SHAPES, key=lambda s: s[0] * s[1])
SMALLEST = min(V.SHAPES, key=lambda s: s[0] * s[1])
REPROJECT = P.PARAM_SETS[next(iter(P.PARAM_SETS))]
MOMENTS = V.MOMENTS_SETS[next(iter(V.MOMENTS_SETS))]
VARIANCE = V.VARIANCE_SETS[next(iter(V.VARIANCE_SETS))]
DENOISE = D.PARAM_SETS["all"]
DENOISE_VARIANCE = V.DENOISE_SETS["all"]


def host_definitions(w, h):
    """The five passes' outputs by the host definitions, for the planes the sequence takes."""
    colour, motion, hcol, hsurf, hlen = P.planes(w, h)
    p = V.planes(w, h)
    dc, da, dn = D.planes(w, h)
    return dict(
        reproject=vc.reproject_host(colour, motion, hcol, hsurf, hlen, **REPROJECT),
        moments=vc.reproject_moments_host(p["colour"], p["motion"], p["hcol"], p["hsurf"],
                                          p["hlen"], p["hmom"], albedo=p["albedo"], **MOMENTS),
        variance=vc.variance_host(p["moments"], p["surface"], **VARIANCE),
        denoise=vc.denoise_host(dc, da, dn, **DENOISE),
        denoise_variance=vc.denoise_variance_host(p["colour"], p["var"], albedo=p["albedo"],
                                                  normal_depth=p["nd"], **DENOISE_VARIANCE))


def test_the_host_forms_in_turn_over_a_shrinking_and_growing_frame():
    want = {shape: host_definitions(*shape) for shape in (LARGEST, SMALLEST)}
    with host_renderer() as r:
        for turn, (w, h) in enumerate((LARGEST, SMALLEST, LARGEST)):
            what = f"turn {turn}, {w}x{h}: "
            colour, motion, hcol, hsurf, hlen = P.planes(w, h)
            p = V.planes(w, h)
            dc, da, dn = D.planes(w, h)
            ref = want[(w, h)]

            out, hist = r.reproject(colour, motion, dict(colour=hcol, surface=hsurf, length=hlen),
                                    surface=hsurf, **REPROJECT)
            same(out, ref["reproject"][0], what + "reproject")
            same(hist["length"], ref["reproject"][1], what + "reproject, length")

            out, hist = r.reproject_moments(
                p["colour"], p["motion"],
                dict(colour=p["hcol"], surface=p["hsurf"], length=p["hlen"], moments=p["hmom"]),
                surface=p["hsurf"], albedo=p["albedo"], **MOMENTS)
            same(out, ref["moments"][0], what + "reproject_moments")
            same(hist["length"], ref["moments"][1], what + "reproject_moments, length")
            same(hist["moments"], ref["moments"][2], what + "reproject_moments, moments")

            var = r.variance(dict(moments=p["moments"], surface=p["surface"]), **VARIANCE)
            same(var, ref["variance"], what + "variance")

            out = r.denoise(dc, dict(albedo=da, normal_depth=dn), **DENOISE)
            same(out, ref["denoise"], what + "denoise")

            out, out_var = r.denoise_variance(p["colour"], p["var"],
                                              dict(albedo=p["albedo"], normal_depth=p["nd"]),
                                              **DENOISE_VARIANCE)
            same(out, ref["denoise_variance"][0], what + "denoise_variance")
            same(out_var, ref["denoise_variance"][1], what + "denoise_variance, variance")
