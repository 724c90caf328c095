"""Every compiled trace-kernel instantiation against the oracle.

rt_scene_create_ex picks one of many kernels from what a scene holds (rt_plan.cpp: select_variant; rt_variant_dispatch.h:
dispatch_variant, which every kernel file's launcher goes through): k_trace_pool_f64<PRIMS, TEXTURED, SPECULAR, BVH> (12 linear-loop forms + 4 BVH forms) and
k_trace_f64<PRIMS, TEXTURED, SPECULAR> (12 forms), each compiled twice — RT_ARITH_FAST and RT_ARITH_REFERENCE.  Template
flags add or remove whole material arms, LDS layouts, NBUF and the fixed-point sums, so each is separate code: every
one renders a scene built to reach it (tests/variant_scenes.py), after the test has checked that the scene selects it.
tests/test_variant_matrix.py checks on the CPU that CASES is exactly the set of instantiations in the compiled code.

The last part is the LDS bill: the linear-loop forms keep the whole primitive table (and the textures, the Perlin
gradients, the lens samples, the ray times) in dynamic LDS on top of their static LDS; the largest table that fits a CU
renders, one texture more is refused by every render entry point before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
abi = S.abi
TOL = 1e-3          # the north star's per-channel tolerance (tests/test_gpu_parity.py)
TIGHT = 1e-9        # what f64 against f64 with the same draws achieves on the bulk
LDS_PER_CU = 160 * 1024

# (kernel, flavour, form): form = (prims_class, textured, specular, bvh); the v1 kernel has no BVH form
CASES = [("pool", fl, form) for fl in ("fast", "exact") for form in V.SPECS] + \
        [("v1", fl, form) for fl in ("fast", "exact") for form in V.SPECS if not form[3]]


def case_id(case):
    kernel, flavour, (p, t, s, b) = case
    return "%s-%s-%s%s%s%s" % (kernel, flavour, "RSA"[p], "t" if t else "", "s" if s else "", "-bvh" if b else "")


def _render(rt, orc, bundle, cam, kernel, flavour, closest_hit, w=V.W, h=V.H, spp=V.SPP):
    camera = S.camera_for(cam, w, h)
    params = abi.render_params(w, h, spp, max_depth=V.DEPTH)
    scene = rt.Scene(bundle, closest_hit=closest_hit,
                     kernel=abi.RT_KERNEL_V1 if kernel == "v1" else abi.RT_KERNEL_POOL,
                     arithmetic=abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST)
    try:
        variant = scene.variant()
        got = scene.render_frame(camera, params)
        stats = scene.last_stats()
    finally:
        scene.close()
    ref, ref_segs = orc.render(bundle.desc, camera, params, use_bvh=V.oracle_use_bvh(bundle))
    return variant, got, stats, ref, ref_segs


def assert_parity(orc, got, stats, ref, ref_segs, w, h, spp, exact):
    assert np.isfinite(got).all()
    a, b = orc.tone_map(orc.ORC_TM_ACES, ref), orc.tone_map(orc.ORC_TM_ACES, got)
    diff = np.abs(a - b)
    assert diff.max() < TOL, "max |delta| = %g" % diff.max()
    frac = float((diff.max(axis=-1) > TIGHT).mean())
    assert frac < 1e-3, "fraction of pixels beyond %g: %g" % (TIGHT, frac)
    assert stats.samples == w * h * spp
    if exact:   # the reference's arithmetic: the oracle's own paths (tests/test_gpu_edges.py, the hall of spheres)
        assert int(stats.segments) == ref_segs
        d = np.abs(got - ref)
        assert d.max() < TOL and float((d > TIGHT).mean()) < 1e-3
    else:
        assert abs(int(stats.segments) - ref_segs) <= 4


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_variant_matches_oracle(rt, orc, gpu, case):
    kernel, flavour, form = case
    prims_class, textured, specular, bvh = form
    spec = V.SPECS[form]
    bundle, cam = V.build(form)
    closest_hit = abi.RT_HIT_BVH if bvh else abi.RT_HIT_LINEAR
    variant, got, stats, ref, ref_segs = _render(rt, orc, bundle, cam, kernel, flavour, closest_hit)
    # the scene selects the kernel it is here for
    want = dict(kernel=int(kernel == "v1"), prims_class=prims_class, textured=textured, specular=specular, use_bvh=bvh,
                exact=int(flavour == "exact"), has_moving=int(bool(spec.get("moving"))),
                perlin_in_lds=int(bool(textured and spec.get("perlin") == "identity")))
    assert {k: variant[k] for k in want} == want
    if bvh:
        assert variant["bvh_nodes_in_lds"] == 1
    if kernel == "pool":
        assert variant["blocks_per_cu"] >= 1 and variant["blocks_per_cu_lens"] >= 1
    assert_parity(orc, got, stats, ref, ref_segs, V.W, V.H, V.SPP, flavour == "exact")
    assert got.std() > 0.05   # a picture, not a flat background


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_bvh_nodes_in_global_memory(rt, orc, gpu, flavour):
    """The textured, specular BVH form over a tree too large for LDS: the walk reads the direction-ordered node copies."""
    bundle, cam = V.large_bvh_scene()
    w, h, spp = 48, 27, 4
    variant, got, stats, ref, ref_segs = _render(rt, orc, bundle, cam, "pool", flavour, abi.RT_HIT_AUTO, w, h, spp)
    assert (variant["use_bvh"], variant["bvh_nodes_in_lds"], variant["prims_class"], variant["textured"], variant["specular"],
            variant["exact"]) == (1, 0, V.SPHERES, 1, 1, int(flavour == "exact"))
    assert np.isfinite(got).all() and got.std() > 0.05
    if flavour == "exact":
        assert_parity(orc, got, stats, ref, ref_segs, w, h, spp, True)
    else:   # the hall of mirrors amplifies the fast divisions' last bits (tests/test_gpu_edges.py): the same paths, the bulk exact
        d = np.abs(got - ref)
        assert stats.samples == w * h * spp and abs(int(stats.segments) - ref_segs) <= 8
        assert np.median(d) < 1e-13 and (d > TOL).mean() < 0.02


@pytest.mark.parametrize("bvh", [0, 1])
def test_scene_without_radiance_bound_renders_with_f64_sums(rt, orc, gpu, bvh):
    """A colour above 1 on a scattering material leaves the scene without a radiance bound: the two-item (OVERLAP) forms
    with fixed-point sums cannot hold it, and RT_ARITH_FAST is rendered by the RT_ARITH_REFERENCE copy (rt_scene_create.hip)."""
    bundle, cam = V.unbounded_scene()
    variant, got, stats, ref, ref_segs = _render(rt, orc, bundle, cam, "pool", "fast", abi.RT_HIT_BVH if bvh else abi.RT_HIT_LINEAR)
    assert (variant["prims_class"], variant["use_bvh"], variant["exact"]) == (V.ANY, bvh, 1)
    assert_parity(orc, got, stats, ref, ref_segs, V.W, V.H, V.SPP, True)


# ---- the LDS bill ------------------------------------------------------------------------------------------------------

MAX_LINEAR_PRIMS = 640   # rt_plan.h: kLinearTableBytes, the linear loop's table is at most 120 KiB of 192-byte records


def lds_scene(prims_class, n_extra_textures):
    """MAX_LINEAR_PRIMS primitives of one class, a Noise over an identity Perlin table (its gradients in LDS), a MovingSphere
    where the class allows one, and n_extra_textures unused solid textures (the linear loop stages the whole table)."""
    textures = [abi.RtTexture(abi.RT_TEX_NOISE, -1, -1, -1, 0, 3, abi.D3(0.9, 0.8, 0.7), 4.0), abi.solid((0.6, 0.6, 0.55)),
                abi.solid((4.0, 3.5, 3.0))]
    textures += [abi.solid((0.1 + 0.001 * i, 0.2, 0.3)) for i in range(n_extra_textures)]
    materials = [abi.material(V.L, 0), abi.material(V.L, 1), abi.material(V.E, 2)]
    prims = []
    n = MAX_LINEAR_PRIMS
    if prims_class == V.RECTS:
        prims.append(abi.rect(abi.RT_PRIM_XZ_RECT, -6, 6, -6, 3, 0.0, 1))
        prims.append(abi.rect(abi.RT_PRIM_XZ_RECT, -1.2, 1.2, -1.5, 0.5, 2.8, 2))
        for i in range(n - len(prims)):   # small noise-textured tiles standing in a grid on the ground
            x, z = -3.0 + 0.25 * (i % 24), -2.0 + 0.25 * (i // 24)
            prims.append(abi.rect(abi.RT_PRIM_XY_RECT, x, x + 0.18, 0.0, 0.2 + 0.1 * (i % 7), z, 0))
    else:
        prims.append(abi.sphere((0.0, -1000.0, 0.0), 1000.0, 1))
        prims.append(abi.sphere((0.0, 3.2, -1.0), 0.6, 2))
        if prims_class == V.ANY:
            prims.append(abi.moving_sphere((0.8, 0.3, 1.2), (0.8, 0.9, 1.2), 0.3, 0, 0, 0.0, 1.0))
        for i in range(n - len(prims)):
            x, z = -3.0 + 0.25 * (i % 24), -2.0 + 0.25 * (i // 24)
            prims.append(abi.sphere((x, 0.1, z), 0.1, 0))
    for i, p in enumerate(prims):
        p.obj_id = i + 1
    bundle = abi.SceneBundle(prims, materials, textures, abi.sky(), perlins=[V.perlin(False)])
    return bundle


LENS_CAM = dict(look_from=(0.0, 1.6, 6.0), look_at=(0.0, 0.4, 0.0), vfov=42.0, aperture=0.3, focus_distance=6.0)
PINHOLE_CAM = dict(LENS_CAM, aperture=0.0)


def _bill(variant, lens):
    return variant["static_lds"] + (variant["dyn_lds_lens"] if lens else variant["dyn_lds"])


def _largest_fit(rt, prims_class):
    """Extra textures of the largest lds_scene whose lens render fits a CU, from the variant's own static LDS."""
    scene = rt.Scene(lds_scene(prims_class, 0), closest_hit=abi.RT_HIT_LINEAR)
    try:
        v = scene.variant()
    finally:
        scene.close()
    assert (v["prims_class"], v["textured"], v["use_bvh"], v["perlin_in_lds"], v["has_moving"]) == \
        (prims_class, 1, 0, 1, int(prims_class == V.ANY))
    room = LDS_PER_CU - _bill(v, True)
    assert room >= 0, v
    return room // 64     # rtdev::Texture is 64 bytes


@pytest.mark.parametrize("prims_class", [V.RECTS, V.SPHERES, V.ANY])
def test_largest_linear_table_that_fits_renders(rt, orc, gpu, prims_class):
    extra = _largest_fit(rt, prims_class)
    bundle = lds_scene(prims_class, extra)
    w, h, spp = 48, 27, 4
    variant, got, stats, ref, ref_segs = _render(rt, orc, bundle, LENS_CAM, "pool", "fast", abi.RT_HIT_LINEAR, w, h, spp)
    assert LDS_PER_CU - 64 < _bill(variant, True) <= LDS_PER_CU, variant
    assert variant["blocks_per_cu_lens"] == 1
    assert_parity(orc, got, stats, ref, ref_segs, w, h, spp, False)


@pytest.mark.parametrize("prims_class", [V.RECTS, V.SPHERES, V.ANY])
def test_one_texture_beyond_the_lds_is_refused_by_every_entry_point(rt, orc, gpu, prims_class):
    import torch
    assert torch.cuda.is_available(), "torch sees no GPU (the library does): no way to allocate the device buffer for this test"
    extra = _largest_fit(rt, prims_class) + 1
    bundle = lds_scene(prims_class, extra)
    w, h, spp = 48, 27, 4
    params = abi.render_params(w, h, spp, max_depth=V.DEPTH)
    lens = S.camera_for(LENS_CAM, w, h)
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_LINEAR)
    try:
        v = scene.variant()
        assert _bill(v, True) > LDS_PER_CU >= _bill(v, False), v
        assert v["blocks_per_cu_lens"] == 0 and v["blocks_per_cu"] >= 1
        dev = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        tm = abi.RtToneMap()
        tm.kind = abi.RT_TM_NONE
        calls = {
            "rt_render_frame": lambda: scene.render_frame(lens, params),
            "rt_render": lambda: scene.render_tiles(lens, params),
            "rt_render_frame_device": lambda: scene.render_frame_device(lens, params, dev.data_ptr()),
            "rt_render_frame_rgba8": lambda: scene.render_frame_rgba8(lens, params, tm),
        }
        for name, call in calls.items():
            with pytest.raises(rt.RtError) as err:
                call()
            assert err.value.code == abi.RT_ERR_UNSUPPORTED, name
            assert "LDS" in rt.lib().rt_last_error_message().decode(), name
        assert not dev.abs().sum().item()   # nothing was launched into the buffer
        # the same scene through a pinhole camera fits, and still renders what the oracle renders
        pinhole = S.camera_for(PINHOLE_CAM, w, h)
        got = scene.render_frame(pinhole, params)
        stats = scene.last_stats()
    finally:
        scene.close()
    ref, ref_segs = orc.render(bundle.desc, pinhole, params)
    assert_parity(orc, got, stats, ref, ref_segs, w, h, spp, False)
