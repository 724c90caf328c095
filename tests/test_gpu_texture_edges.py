"""The texture code against the oracle at its numerical edges: every probe of tests/texture_probes.py through every route
that has texture code of its own.

  pool-fast      k_trace_pool_f64, RT_ARITH_FAST, the linear loop: texture_value_deferred over the LDS copy of the texture
                 table, a plain sphere's (u, v) from sphere_uv_f32 and certified (or redone in f64) by the image lookup,
                 Noise through coop_noise_turbulence, the Checkered's side from sines_product_negative's floor parity
  pool-fast-bvh  the same over the tree: the texture table in global memory.  The tree's forms are PRIMS_ANY; an unwrapped
                 plain sphere keeps the f32 (u, v) arm there too (prim_hit_record: flags == 0), a wrapped or moving one never had it
  pool-exact     RT_ARITH_REFERENCE: f64 (u, v) only, the Cody-Waite reduction in sines_product_negative
  v1-fast/exact  k_trace_f64: texture_value_full (sin_sign, perlin_turbulence per lane, LDS gradients for table 0)
  guides         the albedo plane of render_guides against denoise_model.oracle_guides: texture_value_full without LDS
                 gradients, one ray per pixel through the pixel's centre

A probe renders with max_depth = 1 over black, so a pixel is sqrt(mean of the first hits' texture values): nothing averages
a wrong value away.  The raw frames are compared, not tone-mapped ones.  tests/test_texture_probes_cpu.py checks on the CPU
that each probe reaches its edge, that the oracle's frame moves when the guarded code is broken, and that CASES below is
the probes' table."""
import numpy as np
import pytest

import denoise_model
import texture_probes as P

pytestmark = pytest.mark.gpu
abi = P.abi
TOL = 1e-3          # the project's per-channel tolerance (tests/test_gpu_variants.py)
TIGHT = 1e-9        # what f64 against f64 with the same draws achieves on the bulk

CASES = [(name, route) for name, probe in P.PROBES.items() for route in probe.routes]


@pytest.fixture(scope="module")
def reference(orc):
    """Oracle frames and oracle guide planes, one per (probe, with fillers): computed once, never written to."""
    frames, guides = {}, {}

    def frame(name, fillers):
        key = (name, fillers)
        if key not in frames:
            probe = P.PROBES[name]
            ref, segments = P.oracle_frame(orc, probe, probe.build(fillers=fillers))
            ref.setflags(write=False)
            frames[key] = (ref, segments)
        return frames[key]

    def guide(name):
        if name not in guides:
            probe = P.PROBES[name]
            shape = P.guide_shape(probe)
            guides[name] = denoise_model.oracle_guides(orc, probe.build(), P.camera(orc, probe, shape), shape[0], shape[1])
        return guides[name]
    return frame, guide


def _assert_frame(kind, name, route, exact, got, ref):
    """The comparison of a probe's kind.  Prints its figures first (pytest -s shows them)."""
    assert np.isfinite(got).all()
    d = np.abs(got - ref).max(axis=-1)
    beyond_tol, beyond_tight = int((d > TOL).sum()), float((d > TIGHT).mean())
    print("%s %s: max |delta| %.3g, %d pixels beyond TOL, share beyond TIGHT %.3g" % (name, route, d.max(), beyond_tol, beyond_tight))
    # every probe, every route: no pixel beyond TOL.  For the image probes that is the whole point: a mis-selected texel of
    # a random image moves a pixel by 0.02 .. 0.3, and the only legitimate disagreement is an exact (u, v) within an ulp
    # or two of a cell boundary (~1e-12 per lookup), so no share of pixels is allowed to differ
    assert beyond_tol == 0, "max |delta| = %g" % d.max()
    if exact:       # the reference's own arithmetic: nothing beyond TIGHT
        assert beyond_tight == 0.0, "share of pixels beyond %g: %g" % (TIGHT, beyond_tight)
    elif kind == "image":
        pass        # a texel's value is a byte / 255: same texel, same value; the square root of the mean adds roundings only
    elif name == "noise_big_argument":
        # TOL only: the fast flavour contracts scale * z + 10 * turb into an FMA, which moves an argument of 8e5 by an ulp,
        # ~1e-10; the colour moves as much, and the square root of a pixel near black lifts that past TIGHT
        pass
    else:
        assert beyond_tight < 1e-3, "share of pixels beyond %g: %g" % (TIGHT, beyond_tight)


@pytest.mark.parametrize("name,route", CASES, ids=lambda x: str(x))
def test_probe_matches_oracle(rt, orc, gpu, reference, name, route):
    probe = P.PROBES[name]
    w, h, spp = probe.shape
    frame_ref, guide_ref = reference
    cam = P.camera(orc, probe)
    if route == "guides":
        shape = P.guide_shape(probe)    # (the image probes: one pixel narrower and lower, see there)
        scene = rt.Scene(probe.build())
        try:
            got = scene.render_guides(P.camera(orc, probe, shape), P.params(probe, shape))
        finally:
            scene.close()
        ref = guide_ref(name)
        assert np.array_equal(got["obj_id"], ref["obj_id"])
        _assert_frame(probe.kind, name, route, False, got["albedo"], ref["albedo"])
        return
    r = P.ROUTES[route]
    bvh = r.closest_hit == abi.RT_HIT_BVH
    bundle = probe.build(fillers=bvh)
    scene = rt.Scene(bundle, closest_hit=r.closest_hit, kernel=r.kernel, arithmetic=r.arithmetic)
    try:
        variant = scene.variant()
        got = scene.render_frame(cam, P.params(probe))
        stats = scene.last_stats()
    finally:
        scene.close()
    # the route is the one meant
    want = dict(kernel=int(r.kernel == abi.RT_KERNEL_V1), textured=1, specular=0, use_bvh=int(bvh), exact=r.exact)
    assert {k: variant[k] for k in want} == want
    if bvh:
        assert variant["bvh_nodes_in_lds"] == 1     # seven to nine primitives: a small tree (its kernel is the PRIMS_ANY form)
    else:
        assert variant["prims_class"] == (2 if name in ("image_wrapped", "image_moving") else int(name.startswith("image_")))
    assert variant["has_moving"] == int(name == "image_moving")
    if probe.kind == "noise":       # table 0's gradients in LDS unless a table is shuffled
        assert variant["perlin_in_lds"] == int(name != "noise_two_tables_shuffled")
    ref, ref_segments = frame_ref(name, bvh)
    assert stats.samples == w * h * spp
    assert int(stats.segments) == ref_segments == w * h * spp       # one segment per sample at max_depth = 1
    _assert_frame(probe.kind, name, route, bool(r.exact), got, ref)
    assert got.std() > 0.05
