"""The fixed-point pixel sums of the pooled variants that keep two items in flight (rt_trace_pool_kernel.hip, OVERLAP;
rt_device_types.h: sum_scale) on the device, across the radiance range the host accepts for them and beyond it.

The rule (rt_plan.cpp: scene_radiance_bound, sum_exponent; tests/test_fixed_point_sums.py checks it on the host): a scene
whose radiance bound E is below 2^30 sums its samples as integers of 2^(e-52), e <= 31; a brighter one keeps the f64 sums
of the RT_ARITH_REFERENCE copy.  Every fixed-sum path is run through that range — the mixed linear variant, the BVH with
its nodes in LDS, the BVH with its nodes in global memory and the delivering launch of the tile stream — on a scene whose
dark pixels are of the order of the quantum; and a frame that looks into an emitter at the top of a power of two, where an
overflow of the sums or a stray exponent field would show.
"""
import numpy as np
import pytest

import scenes_py as S
from test_fixed_point_sums import dark_under_bright

pytestmark = pytest.mark.gpu
abi = S.abi
TOL = 1e-3
CAP = 2.0 ** 30      # rt_plan.cpp: kSumsBoundCap
EMISSIONS = [2.0 ** 4, 2.0 ** 20, CAP * (1 - 1e-15), CAP, 2.0 ** 33, 2.0 ** 39]


def with_spheres(bundle, n, seed=5):
    """n small spheres of the walls' material on the floor of the box: more than 48 primitives take the BVH, more than
    2048 a tree too large for LDS (the walk reads the direction-ordered node copies in global memory)."""
    rng = np.random.default_rng(seed)
    prims = list(bundle.primitives)[:bundle.desc.n_primitives]
    for i in range(n):
        c = (float(rng.uniform(20, 535)), float(rng.uniform(4, 60)), float(rng.uniform(20, 535)))
        prims.append(abi.sphere(c, 3.0, 2, len(prims) + 1))
    return abi.SceneBundle(prims, list(bundle.materials), list(bundle.textures), bundle.desc.background)


PATHS = {   # name -> (extra spheres, render through the tile stream, expected use_bvh, expected bvh_nodes_in_lds)
    "linear": (0, False, 0, 0),
    "bvh_lds": (44, False, 1, 1),
    "bvh_global": (2100, False, 1, 0),
    "delivering": (0, True, 0, 0),
}


def render(rt, bundle, camera, params, arithmetic, tiles):
    scene = rt.Scene(bundle, arithmetic=arithmetic)
    try:
        variant = scene.variant()
        if not tiles:
            return variant, scene.render_frame(camera, params)
        frame = np.full((params.height, params.width, 3), np.nan)
        for r, c, tw, th, t in scene.render_tiles(camera, params):
            frame[r:r + th, c:c + tw] = t
        return variant, frame
    finally:
        scene.close()


@pytest.mark.parametrize("path", sorted(PATHS))
def test_dark_walls_under_a_bright_light(rt, orc, gpu, path):
    """A light of E over walls of albedo 0.45 2^-12 / E: every once-bounced sample is 1.1e-4, whatever E.  Below the cap
    the frame is within the quantum of the oracle's f64 sums; from the cap on it is the RT_ARITH_REFERENCE frame."""
    extra, tiles, use_bvh, in_lds = PATHS[path]
    w, h, spp = 24, 24, 32
    params = abi.render_params(w, h, spp, tiles_w=3, tiles_h=2)
    for emission in EMISSIONS:
        bundle, cam = dark_under_bright(emission)
        if extra:
            bundle = with_spheres(bundle, extra)
        camera = S.camera_for(cam, w, h)
        bound = rt.radiance_bound(bundle)
        e = rt.sum_exponent(bound, spp)
        assert (bound == 0.0) == (emission >= CAP) and (e == 0) == (bound == 0.0)
        variant, got = render(rt, bundle, camera, params, abi.RT_ARITH_FAST, tiles)
        assert (variant["prims_class"], variant["use_bvh"], variant["exact"]) == (2, use_bvh, int(e == 0)), (path, emission)
        if use_bvh:
            assert variant["bvh_nodes_in_lds"] == in_lds
        ref, _ = orc.render(bundle.desc, camera, params, use_bvh=0)
        assert np.isfinite(got).all() and ref.max() ** 2 >= 0.5 * emission     # the light is in view
        assert np.abs(got - ref).max() < TOL, (path, emission, np.abs(got - ref).max())
        radiance = np.abs(got ** 2 - ref ** 2)
        assert (radiance <= 2.0 ** (e - 53) + 1e-12 * np.maximum(1.0, ref ** 2)).all(), (path, emission, e, radiance.max())
        if e == 0:   # f64 sums: the RT_ARITH_REFERENCE copy's frame, to the last bit
            _, exact = render(rt, bundle, camera, params, abi.RT_ARITH_REFERENCE, tiles)
            assert np.array_equal(got, exact), (path, emission)


def into_the_light(emission):
    """A camera that looks into a wall-sized emitter; a box behind it makes the scene mixed-class (the linear variant
    with fixed-point sums).  Every sample of every pixel is the emission."""
    textures = [abi.solid((0.5, 0.5, 0.5)), abi.solid((emission,) * 3)]
    materials = [abi.material(abi.RT_MAT_LAMBERTIAN, 0), abi.material(abi.RT_MAT_DIFFUSE_LIGHT, 1)]
    prims = [abi.rect(abi.RT_PRIM_XY_RECT, -100.0, 100.0, -100.0, 100.0, -5.0, 1, 1),
             abi.box((-1.0, -1.0, 8.0), (1.0, 1.0, 9.0), 0, 2)]
    bundle = abi.SceneBundle(prims, materials, textures, abi.solid_background((0.0, 0.0, 0.0)))
    return bundle, dict(look_from=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), vfov=40.0, aperture=0.0, focus_distance=5.0)


@pytest.mark.parametrize("k", [4, 29])
def test_saturated_pixels_at_the_top_of_a_power_of_two(rt, gpu, k):
    """E = 2^k, 2^k (1 - 2e-6) (below the exponent's 1e-6 margin: T 2^(52-e) just under 2^52) and 2^k (1 - 5e-7) (inside
    it), at chunks of exactly 2048 samples and just above (the scale halves): a pixel is sqrt(E) to 1e-15."""
    w, h = 16, 16
    for emission in (2.0 ** k, 2.0 ** k * (1 - 2e-6), 2.0 ** k * (1 - 5e-7)):
        bundle, cam = into_the_light(emission)
        camera = S.camera_for(cam, w, h)
        scene = rt.Scene(bundle)
        try:
            variant = scene.variant()
            assert (variant["prims_class"], variant["use_bvh"], variant["exact"]) == (2, 0, 0)
            for spp in (32768, 32784):
                assert rt.sum_exponent(rt.radiance_bound(bundle), spp) <= 31
                got = scene.render_frame(camera, abi.render_params(w, h, spp))
                assert scene.last_stats().samples == w * h * spp
                rel = np.abs(got / np.sqrt(emission) - 1.0)
                assert rel.max() <= 1e-15, (emission, spp, rel.max())
        finally:
            scene.close()


def test_a_render_beyond_the_budget_is_refused(rt, gpu):
    """A bound a hair below the cap takes e = 31 at chunks of 2048 samples; the halving of longer chunks would take it to
    32, so the render is refused and names RT_ARITH_REFERENCE — which renders it."""
    w, h = 16, 16
    emission = CAP * (1 - 1e-15)
    bundle, cam = into_the_light(emission)
    camera = S.camera_for(cam, w, h)
    scene = rt.Scene(bundle)
    try:
        assert scene.variant()["exact"] == 0
        got = scene.render_frame(camera, abi.render_params(w, h, 32768))
        assert np.abs(got / np.sqrt(emission) - 1.0).max() <= 1e-15
        with pytest.raises(rt.RtError) as err:
            scene.render_frame(camera, abi.render_params(w, h, 32769))
        assert err.value.code == abi.RT_ERR_UNSUPPORTED and "RT_ARITH_REFERENCE" in str(err.value)
        with pytest.raises(rt.RtError) as err:
            scene.render_tiles(camera, abi.render_params(w, h, 32769))
        assert err.value.code == abi.RT_ERR_UNSUPPORTED
        # the refusal leaves the scene usable
        assert np.array_equal(scene.render_frame(camera, abi.render_params(w, h, 32768)), got)
    finally:
        scene.close()
    scene = rt.Scene(bundle, arithmetic=abi.RT_ARITH_REFERENCE)
    try:
        got = scene.render_frame(camera, abi.render_params(w, h, 32769))
        assert np.abs(got / np.sqrt(emission) - 1.0).max() <= 1e-12
    finally:
        scene.close()
