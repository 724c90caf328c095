"""What keeps tests/test_gpu_ray_probes.py honest, without a GPU: every probe of tests/ray_probes.py against the oracle and
against an exact rational model of the reference's rules (ray_probes.q_*: fractions.Fraction over the doubles' exact
values, no rounding anywhere; an independent restatement, not the oracle's code).  Per probe:

  the ray is the one meant      the camera yields (o, d) bit for bit for every pixel and sample; a fan, exactly zero where meant
  the edge is reached           the decisive quantity sits ON the edge in exact arithmetic, and the oracle's hit, miss and
                                primitive are the rational model's under the reference's inclusive rules
  no rounding decides           every intermediate of the decisive quantity is representable in f64 (a probe that cannot meet
                                this runs on the RT_ARITH_REFERENCE routes only and says so)
  the frame shows the decision  with the decisive coordinate one ulp on the other side the oracle's frame moves by more than TOL
  no non-finite hit             no primitive of the scene answers any ray of the probe with a non-finite t
  the table is covered          CASES of the GPU test is the table's product, every edge class is there on every route"""
import ctypes as C
import math

import numpy as np
import pytest

import denoise_model
import ray_probes as P
import test_gpu_ray_probes as G
import texture_probes as T

abi = P.abi
TOL = 1e-3          # the project's per-channel tolerance (tests/test_gpu_variants.py)
NAMES = list(P.PROBES)


def _rays(probe, alt=False):
    """-> (origin, unique directions [N, 3], time) of the probe's frame AND of its guide plane."""
    cam = probe.camera(alt)
    _, _, _, dirs, time = T.primary_rays(cam, probe.params())
    w, h, _ = probe.guide_shape()
    pixel = np.arange(w * h)
    u, v = (pixel % w + 0.5) / (w - 1), (pixel // w + 0.5) / (h - 1)
    ulc, hor, ver, org = (np.array(x[:]) for x in (cam.upper_left_corner, cam.horizontal, cam.vertical, cam.origin))
    gdirs = ((ulc[None, :] + u[:, None] * hor[None, :]) - v[:, None] * ver[None, :]) - org[None, :]
    assert np.all(time == cam.time_a) and (cam.time_a + cam.time_b) * 0.5 == cam.time_a
    return dirs, np.unique(np.concatenate([dirs, gdirs]), axis=0), float(cam.time_a)


# ---- the table ---------------------------------------------------------------------------------------------------------------
# edge class -> the kernel forms (prims_class) it must be rendered in on the pool-fast route
REQUIRED = {
    "rect_plane_a0": {0}, "rect_plane_a1": {0}, "rect_corner": {0}, "rect_outside_ulp": {0}, "rect_tmin": {0}, "rect_tmin_below": {0},
    "rect_back_face": {0}, "rect_front_face": {0}, "rect_coplanar": {0},
    "rect_plane_a0_wrapped": {2}, "rect_plane_a1_wrapped": {2}, "rect_corner_wrapped": {2}, "rect_outside_ulp_wrapped": {2},
    "rect_tmin_wrapped": {2}, "rect_tmin_below_wrapped": {2}, "rect_back_face_wrapped": {2}, "rect_front_face_wrapped": {2},
    "rect_coplanar_wrapped": {2},
    "sphere_tangent": {1, 2}, "sphere_tangent_d2": {1, 2}, "sphere_tangent_d3": {1, 2}, "sphere_inside": {1, 2}, "sphere_surface": {1, 2},
    "sphere_neg_radius": {1, 2}, "moving_sphere": {2},
    "box_entry": {2}, "box_rotated": {2}, "box_inside": {2}, "box_near_tmin": {2}, "box_tie": {2},
    "diel_head_on": {1}, "diel_critical": {0}, "diel_ior_1": {1}, "diel_ior_below_1": {1}, "diel_translate": {2},
    "metal_normal": {1}, "metal_back_face": {0}, "metal_fuzz_1": {1},
}
# ... and the classes that cannot run everywhere: a rounding decides in f64 (RT_ARITH_REFERENCE routes), or the class is the tree's
RESTRICTED = {"sphere_root_tmin": P.EXACT_ROUTES, "sphere_root_below": P.EXACT_ROUTES, "box_tie_side": P.EXACT_ROUTES,
              "bvh_f32_box": P.TREE_ROUTES, "bvh_flat_box": P.TREE_ROUTES, "bvh_global": P.TREE_ROUTES}


def test_the_table_is_covered():
    assert G.CASES == P.CASES and len(set(P.CASES)) == len(P.CASES)
    assert set(P.ALL_ROUTES) == {"pool-fast", "pool-fast-bvh", "pool-exact", "v1-fast", "v1-exact", "guides"}
    assert P.ROUTES["pool-exact"].exact and P.ROUTES["v1-exact"].exact
    classes = {}
    for probe in P.PROBES.values():
        classes.setdefault(probe.cls, []).append(probe)
    assert set(classes) == set(REQUIRED) | set(RESTRICTED)
    for cls, forms in REQUIRED.items():
        for route in P.ALL_ROUTES:      # every route, and on the pooled linear route every form that can hold the class
            assert any(route in p.routes for p in classes[cls]), (cls, route)
        assert {p.form for p in classes[cls] if "pool-fast" in p.routes} == forms, cls
    for cls, routes in RESTRICTED.items():
        for p in classes[cls]:
            assert p.routes == tuple(routes), p.name
    for probe in P.PROBES.values():
        assert probe.__doc__ and ".rs:" in probe.__doc__, probe.name      # names the reference line it pins
        w, h, spp = probe.shape
        assert (w, h, spp) in ((8, 8, 4), (64, 8, 4))
        if probe.rounding:
            assert "RT_ARITH_REFERENCE routes only" in probe.__doc__, probe.name
        if probe.tie:
            assert probe.depth == 1 and set(probe.tie[0]) <= set(P.SLAB_ROUTES), probe.name


def test_every_probe_selects_the_kernel_form_it_is_described_with(rt):
    for name, probe in P.PROBES.items():
        got = rt.classify(probe.bundle())
        assert got["prims_class"] == probe.form and got["textured"] == 0, name
        assert got["has_moving"] == int(probe.cls == "moving_sphere"), name


def test_the_guide_reference_is_denoise_models(orc):
    """ray_probes.oracle_guides differs from denoise_model.oracle_guides in the scan only (linear for every scene): where
    the model scans linearly too, and where no two hits tie, the planes are the same."""
    for name in ("rect_plane_a0[xy,tr]", "box_entry[z,rot90]", "sphere_tangent[spheres]", "rect_corner[xz]"):
        probe = P.PROBES[name]
        w, h, _ = probe.guide_shape()
        want = denoise_model.oracle_guides(orc, probe.bundle(), probe.camera(), w, h)
        got = P.oracle_guides(orc, probe)
        for plane in ("obj_id", "normal", "position"):
            assert np.array_equal(got[plane], want[plane]), (name, plane)
        assert (got["obj_id"] >= 0).any()


# ---- per probe ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_the_ray_is_the_one_meant(name):
    probe = P.PROBES[name]
    for alt in (False, True):
        s = probe.spec(alt)
        cam = probe.camera(alt)
        o, d = tuple(float(x) for x in s["o"]), tuple(float(x) for x in s["d"])
        assert tuple(cam.origin[:]) == o and cam.lens_radius == 0.0 and cam.time_a == cam.time_b == s["time"]
        assert tuple(cam.upper_left_corner[i] - cam.origin[i] for i in range(3)) == d      # ulc - origin is d, bit for bit
        dirs, unique, _ = _rays(probe, alt)
        w, h, spp = probe.shape
        assert len(dirs) == w * h * spp
        if s["fan"] is None:
            assert tuple(cam.horizontal[:]) == tuple(cam.vertical[:]) == (0.0, 0.0, 0.0)
            assert len(unique) == 1 and tuple(unique[0]) == d       # every pixel, every sample, and the guides' rays
        else:
            fan = tuple(s["fan"][1])
            assert sum(1 for x in fan if x != 0.0) == 1
            other = cam.vertical if s["fan"][0] == "h" else cam.horizontal
            assert tuple(other[:]) == (0.0, 0.0, 0.0)
            for i in range(3):
                if fan[i] == 0.0:       # off the fan's axis: d's own component, an exact zero where d has one
                    assert np.all(unique[:, i] == d[i])
                    assert d[i] != 0.0 or not np.signbit(unique[:, i]).any()
            assert any(d[i] == 0.0 and fan[i] == 0.0 for i in range(3))
            assert len(unique) >= w


@pytest.mark.parametrize("name", NAMES)
def test_the_edge_is_reached_and_no_rounding_decides(orc, name):
    probe = P.PROBES[name]
    s = probe.spec()
    edge = s["check"]()
    assert edge.on, "the rational model does not find the ray on the edge"
    exact = all(P.representable(x) for x in edge.exact)
    if probe.rounding:      # says so in its docstring (test_the_table_is_covered) and runs on the exact routes only
        assert not exact and set(probe.routes) <= set(P.EXACT_ROUTES)
    else:
        assert exact, [float(x) for x in edge.exact if not P.representable(x)]
    if s["ulp"] is not None:       # alt is the NEIGHBOURING double
        x0, x1 = s["ulp"]
        assert x0 != x1 and P.nxt(x0, x1) == x1
        a = probe.spec(alt=True)
        changed = [(p0.p[:], p1.p[:]) for p0, p1 in zip(s["prims"], a["prims"]) if p0.p[:] != p1.p[:] or p0.center_b[:] != p1.center_b[:]]
        assert (tuple(s["o"]) != tuple(a["o"])) + bool(changed) == 1 and tuple(s["d"]) == tuple(a["d"])


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_decides_as_the_rational_model(orc, name):
    """Hit, miss and primitive of every ray of the probe and of its alt: orc_scene_hit_time's linear scan against q_scene."""
    probe = P.PROBES[name]
    lib = orc.lib()
    hit = orc.OrcHit()
    for alt in (False, True):
        s = probe.spec(alt)
        bundle = probe.bundle(alt)
        prims = [bundle.primitives[i] for i in range(bundle.desc.n_primitives)]
        _, unique, time = _rays(probe, alt)
        if len(unique) > 64:        # a fan: its two ends, and an even spread between them
            unique = unique[np.unique(np.linspace(0, len(unique) - 1, 48).astype(int))]
        scene = lib.orc_scene_build(C.byref(bundle.desc), 0, 1)
        try:
            seen = set()
            for d in unique:
                ok = lib.orc_scene_hit_time(scene, orc.d3(s["o"]), orc.d3(d), time, P.T_MIN, math.inf, C.byref(hit))
                best, t = P.q_scene(prims, s["o"], tuple(d), time)
                assert bool(ok) == (best is not None), (alt, tuple(d))
                if ok:
                    assert hit.obj_id == best + 1, (alt, tuple(d))
                    if P.representable(t):
                        assert hit.t == float(t)
                seen.add(best)
        finally:
            lib.orc_scene_free(scene)
        if s["fan"] is not None and not alt:
            assert len(seen) > 1        # across the fan the in-plane coordinate leaves the rect on the other axis


@pytest.mark.parametrize("name", NAMES)
def test_no_primitive_answers_with_a_non_finite_t(orc, name):
    """The reference's comparisons are all false on NaN, so it accepts 0 / 0 and x * inf hits; box_slab_t and the tree are
    documented as open there (rt_trace_common.h).  No probe may form such a ray, for any primitive of its scene."""
    probe = P.PROBES[name]
    lib = orc.lib()
    hit = orc.OrcHit()
    for alt in (False, True):
        s = probe.spec(alt)
        bundle = probe.bundle(alt, fillers=True)
        _, unique, time = _rays(probe, alt)
        if bundle.desc.n_primitives > 100:
            unique = unique[:1]
        o = orc.d3(s["o"])
        for d in unique:
            dd = orc.d3(d)
            for i in range(bundle.desc.n_primitives):
                if lib.orc_hit_primitive_time(C.byref(bundle.primitives[i]), o, dd, time, P.T_MIN, math.inf, C.byref(hit)):
                    assert math.isfinite(hit.t) and np.isfinite(hit.point[:]).all(), (alt, i, tuple(d))


@pytest.mark.parametrize("name", NAMES)
def test_the_frame_shows_the_decision(orc, name):
    probe = P.PROBES[name]
    w, h, spp = probe.shape
    frame, segments = P.oracle_frame(orc, probe)
    other, _ = P.oracle_frame(orc, probe, alt=True)
    assert np.isfinite(frame).all() and np.isfinite(other).all()
    assert np.abs(frame - other).max() > TOL
    if probe.depth == 1:
        assert segments == w * h * spp
    else:
        assert w * h * spp < segments <= probe.depth * w * h * spp
    # the far fillers of the RT_HIT_BVH route change nothing
    with_fillers, seg2 = P.oracle_frame(orc, probe, fillers=True)
    assert np.array_equal(with_fillers, frame) and seg2 == segments
