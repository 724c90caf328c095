"""The fixed-point pixel sums of the pooled variants that keep two items in flight (rt_trace_pool_kernel.hip, OVERLAP;
rt_device_types.h: sum_scale), checked on the host against the oracle's per-sample radiances — no device needed.

The sums rest on two host rules (rt_plan.cpp): the scene's radiance bound E (rtdev_scene_radiance_bound) and the exponent e
it gives a render (rtdev_sum_exponent: sum_scale = 2^(52 - e)).  What has to hold:
  * the bound bounds every sample, so round(T 2^(52-e)) fits the kernel's 52-bit conversion and a chunk of such integers
    the 64-bit sum (a sample above the bound would turn the sum into garbage, not into a NaN);
  * the quantum 2^(e-52) stays inside the 1e-3 per-channel tolerance of RT_ARITH_FAST: a pixel's mean radiance is off by
    at most 2^(e-53), its gamma-encoded value by up to sqrt(2^(e-53));
  * outside that budget a scene keeps f64 sums (no bound) or the render is refused (RT_ERR_UNSUPPORTED).
tests/test_gpu_fixed_point.py renders the same families on the device.
"""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

import scenes_py as S
import variant_scenes as V

abi = S.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3                   # per channel, gamma-encoded (rt_abi.h: RT_ARITH_FAST)
BUDGET = 0.5 * TOL           # what the quantum may take of it: sqrt(2^(e-53)) <= 5e-4, i.e. e <= 31
MAX_CHUNKS = 64              # rt_device_types.h: RT_MAX_CHUNKS


# ---- helpers -----------------------------------------------------------------------------------------------------------

def chunk_plan(samples):
    """rt_plan.cpp: chunk_plan of the product build -> the start sample of every chunk plus the total.  (Checked against
    the library's rule in test_chunk_plan_replica_matches_the_library.)"""
    full = max(24, ((samples + 15) // 16 + 3) // 4 * 4)
    starts, at = [], 0
    while samples - at >= 2 * full and len(starts) < MAX_CHUNKS - 8:
        starts.append(at)
        at += full
    while samples - at > 8:
        starts.append(at)
        rest = samples - at
        at += full if rest >= 2 * full else (rest // 2 + 3) // 4 * 4
        if len(starts) >= MAX_CHUNKS - 1:
            break
    if at < samples:
        starts.append(at)
    starts.append(samples)
    return starts


def longest_chunk(samples):
    plan = chunk_plan(samples)
    return max(b - a for a, b in zip(plan, plan[1:]))


def halvings(longest):
    h = 0
    while longest > 2048:
        longest = (longest + 1) // 2
        h += 1
    return h, longest


def sample_radiances(desc, camera, params, use_bvh=1):
    """The oracle's radiance of every sample of every pixel -> float64 [H, W, spp, 3] (the terms of the f64 sums)."""
    from oracle import oracle_ctypes as orc
    lib = orc.lib()
    scene = lib.orc_scene_build(C.byref(desc), use_bvh, params.seed)
    w, h, spp = params.width, params.height, params.samples
    out = np.zeros((h, w, spp, 3))
    o = (C.c_double * 3)()
    f, d, cam, p = lib.orc_sample_radiance, C.byref(desc), C.byref(camera), C.byref(params)
    try:
        for y in range(h):
            for x in range(w):
                for s in range(spp):
                    f(d, scene, cam, p, x, y, s, o, None)
                    out[y, x, s] = o[:]
    finally:
        lib.orc_scene_free(scene)
    return out


def fixed_point_frame(T, e):
    """The kernel's sums in numpy: every sample rounded to the nearest multiple of 2^(e-52) (fma(T, 2^(52-e), 2^52):
    round to nearest even, as np.rint), summed, sqrt(sum / spp)."""
    q = 2.0 ** (52 - e)
    return np.sqrt((np.rint(T * q) / q).sum(axis=2) / T.shape[2])


def f64_frame(T):
    return np.sqrt(T.sum(axis=2) / T.shape[2])


def room(light_tex, wall_tex=None, textures=(), images=(), perlins=(), background=None, light_radius=1.2):
    """A closed box of six Lambertian walls (wall_tex, default a grey) around a camera that looks at a large emitting
    sphere (light_tex); `textures` go in front of the two."""
    tex = list(textures)
    if wall_tex is None:
        wall_tex = abi.solid((0.6, 0.6, 0.6))
    tex += [wall_tex, light_tex]
    walls, light = len(tex) - 2, len(tex) - 1
    mats = [abi.material(V.L, walls), abi.material(V.E, light)]
    k = 3.0
    prims = [abi.rect(abi.RT_PRIM_XY_RECT, -k, k, -k, k, -k, 0), abi.rect(abi.RT_PRIM_XY_RECT, -k, k, -k, k, k, 0),
             abi.rect(abi.RT_PRIM_XZ_RECT, -k, k, -k, k, -k, 0), abi.rect(abi.RT_PRIM_XZ_RECT, -k, k, -k, k, k, 0),
             abi.rect(abi.RT_PRIM_YZ_RECT, -k, k, -k, k, -k, 0), abi.rect(abi.RT_PRIM_YZ_RECT, -k, k, -k, k, k, 0),
             abi.sphere((0.0, 0.0, -1.5), light_radius, 1)]
    for i, p in enumerate(prims):
        p.obj_id = i + 1
    bg = background if background is not None else abi.solid_background((0.0, 0.0, 0.0))
    bundle = abi.SceneBundle(prims, mats, tex, bg, images=images, perlins=perlins)
    return bundle, dict(look_from=(0.0, 0.0, 2.5), look_at=(0.0, 0.0, -1.5), vfov=70.0, aperture=0.0, focus_distance=4.0)


def noise(color, perlin=0, depth=7, scale=40.0):
    return abi.RtTexture(abi.RT_TEX_NOISE, -1, -1, -1, perlin, depth, abi.D3(*color), scale)


def image_tex(image=0):
    return abi.RtTexture(abi.RT_TEX_IMAGE, -1, -1, image, -1, 0, abi.D3(0, 0, 0), 0.0)


def checkered(even, odd):
    return abi.RtTexture(abi.RT_TEX_CHECKERED, even, odd, -1, -1, 0, abi.D3(0, 0, 0), 0.0)


def white_image(w=4, h=4):
    return np.full((h, w, 4), 255, dtype=np.uint8)


def adversarial_scenes():
    """name -> (bundle, camera dict, max_depth, the least the brightest sample reaches, as a fraction of the bound)."""
    out = {}
    # a Noise on the light: colour x 0.5 (1 + sin(..)), whose factor reaches 1 at the crests
    b, cam = room(noise((8.0, 8.0, 8.0)), perlins=[V.perlin(False)])
    out["noise_light"] = (b, cam, 20, 0.99)
    b, cam = room(noise((8.0 * (1 - 5e-7),) * 3), perlins=[V.perlin(True)])
    out["noise_light_a_hair_below_8"] = (b, cam, 20, 0.99)
    # an image on the light: texels px * (1/255), 255 -> 1
    b, cam = room(image_tex(), images=[V.image()])
    out["image_light"] = (b, cam, 20, 0.99)
    b, cam = room(image_tex(), images=[white_image()])
    out["white_image_light"] = (b, cam, 20, 1.0)
    # Checkered sides on a light: a solid colour and a Noise, and a bright side beside a dim one
    b, cam = room(checkered(0, 1), textures=[abi.solid((16.0, 16.0, 16.0)), noise((4.0, 2.0, 1.0))], perlins=[V.perlin(False)])
    out["checkered_light_solid_noise"] = (b, cam, 20, 0.99)
    b, cam = room(checkered(0, 1), textures=[abi.solid((0.5, 0.5, 0.5)), image_tex()], images=[white_image()])
    out["checkered_light_solid_image"] = (b, cam, 20, 0.99)
    # an all-white image on every wall and a white light: every attenuation 1, twenty bounces deep, then the white of an
    # exhausted depth (no emitter in reach: a black sphere-light)
    b, cam = room(abi.solid((0.0, 0.0, 0.0)), wall_tex=image_tex(), images=[white_image()])
    out["white_image_walls_depth_20"] = (b, cam, 20, 1.0)
    b, cam = room(abi.solid((1.0, 1.0, 1.0)), wall_tex=image_tex(), images=[white_image()])
    out["white_image_walls_white_light"] = (b, cam, 20, 1.0)
    # max_depth exhaustion without any light at all
    for depth in (0, 1, 3):
        b, cam = room(abi.solid((0.0, 0.0, 0.0)), wall_tex=abi.solid((1.0, 1.0, 1.0)))
        out["depth_%d_exhausted" % depth] = (b, cam, depth, 1.0)
    # skies: the camera looks out of an open scene (a white sphere and a white ground) at a blend of top and bottom
    for name, top, bottom in (("sky_on_a_power_of_two", 4.0, 4.0), ("sky_a_hair_below", 4.0 * (1 - 1e-7), 4.0 * (1 - 9e-7)),
                              ("sky_just_outside_the_margin", 4.0 * (1 - 2e-6), 4.0 * (1 - 3e-6)),
                              ("sky_top_on_bottom_below", 8.0, 8.0 * (1 - 5e-7)), ("sky_of_ones", 1.0, 1.0)):
        tex = [abi.solid((1.0, 1.0, 1.0))]
        mats = [abi.material(V.L, 0)]
        prims = [abi.sphere((0.0, -1000.0, 0.0), 1000.0, 0, 1), abi.sphere((0.0, 1.0, 0.0), 1.0, 0, 2)]
        b = abi.SceneBundle(prims, mats, tex, abi.sky((top,) * 3, (bottom,) * 3))
        cam = dict(look_from=(0.0, 1.5, 6.0), look_at=(0.0, 1.0, 0.0), vfov=60.0, aperture=0.0, focus_distance=6.0)
        out[name] = (b, cam, 20, 0.99)
    return out


def shipped_scenes(host):
    """scenes/*.yml (and the generated `random`) through the host session -> name -> (desc, camera, max_depth, session)."""
    config = os.path.join(ROOT, "scenes", "config_c1.yml")
    paths = sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.yml")) if not os.path.basename(p).startswith("config"))
    assert len(paths) >= 7
    out = {}
    for scene in paths + ["random"]:
        s = host.Session(config, scene=scene)
        out[os.path.basename(scene)] = (s.desc, s.camera, s.params.max_depth, s)
    return out


def assert_bounded(rt, desc, camera, w, h, spp, max_depth, use_bvh=1, reach=0.0, name=""):
    bound = rt.radiance_bound(desc)
    assert bound >= 1.0, name
    params = abi.render_params(w, h, spp, max_depth=max_depth)
    T = sample_radiances(desc, camera, params, use_bvh)
    assert np.isfinite(T).all() and T.min() >= 0.0, name
    assert T.max() <= bound, (name, T.max(), bound)
    assert T.max() >= reach * bound, (name, T.max(), bound)
    for samples in (spp, 32768, 32769):
        e = rt.sum_exponent(bound, samples)
        assert 0 < e <= 31, (name, e)
        assert (T * 2.0 ** (52 - e)).max() < 2.0 ** 52, name
    return T


# ---- 1. the bound bounds every sample ------------------------------------------------------------------------------------

def test_shipped_scenes_stay_within_their_radiance_bound(rt, orc, host):
    for name, (desc, camera, depth, _session) in shipped_scenes(host).items():
        assert_bounded(rt, desc, camera, 12, 8, 6, depth, name=name)


@pytest.mark.parametrize("form", sorted(V.SPECS), ids=lambda f: "%d%d%d%d" % f)
def test_variant_forms_stay_within_their_radiance_bound(rt, orc, form):
    bundle, cam = V.build(form)
    w, h = 12, 8
    assert_bounded(rt, bundle.desc, S.camera_for(cam, w, h), w, h, 6, V.DEPTH, V.oracle_use_bvh(bundle), name=str(form))


@pytest.mark.parametrize("name", sorted(adversarial_scenes()))
def test_adversarial_scenes_stay_within_their_radiance_bound(rt, orc, name):
    """Every source a sample can take its value from, pushed to its bound: Noise and image lights, Checkered sides on a
    light, attenuations of exactly 1 twenty bounces deep, depth exhaustion, skies on and a hair below a power of two.  The
    brightest sample has to reach the bound (or nearly), so that the check has something to check."""
    bundle, cam, depth, reach = adversarial_scenes()[name]
    w, h = 12, 8
    assert_bounded(rt, bundle.desc, S.camera_for(cam, w, h), w, h, 8, depth, reach=reach, name=name)


def test_descriptions_without_a_bound_report_none(rt):
    def with_light(bundle, colour):
        textures = list(bundle.textures)
        textures[3] = abi.solid(colour)
        return abi.SceneBundle(list(bundle.primitives), list(bundle.materials), textures, bundle.desc.background)

    boxes, _, _ = S.cornell_box_boxes()
    unbounded, _ = V.unbounded_scene()
    hot_wall = list(boxes.textures)
    hot_wall[2] = abi.solid((0.63, 1.0 + 1e-12, 0.63))
    cases = {
        "lambertian_above_1": unbounded,
        "lambertian_a_hair_above_1": abi.SceneBundle(list(boxes.primitives), list(boxes.materials), hot_wall, boxes.desc.background),
        "negative_light": with_light(boxes, (15.0, -1e-300, 15.0)),
        "light_at_the_cap": with_light(boxes, (2.0 ** 30, 1.0, 1.0)),
        "light_above_the_cap": with_light(boxes, (2.0 ** 39, 2.0 ** 39, 2.0 ** 39)),
        "sky_at_the_cap": abi.SceneBundle(list(boxes.primitives), list(boxes.materials), list(boxes.textures),
                                          abi.sky((1.0, 1.0, 1.0), (2.0 ** 30, 0.5, 0.5))),
        "negative_sky": abi.SceneBundle(list(boxes.primitives), list(boxes.materials), list(boxes.textures),
                                        abi.sky((1.0, 1.0, 1.0), (0.5, -0.5, 0.5))),
        "nan_background": abi.SceneBundle(list(boxes.primitives), list(boxes.materials), list(boxes.textures),
                                          abi.solid_background((0.0, float("nan"), 0.0))),
    }
    for name, bundle in cases.items():
        assert rt.radiance_bound(bundle) == 0.0, name
    # and the sides that keep one
    assert rt.radiance_bound(with_light(boxes, (2.0 ** 30 * (1 - 1e-15), 1.0, 1.0))) == 2.0 ** 30 * (1 - 1e-15)
    assert rt.radiance_bound(with_light(boxes, (0.5, 0.5, 0.5))) == 1.0      # the white of an exhausted depth


# ---- 2. the scale rule ----------------------------------------------------------------------------------------------------

BOUNDS = sorted({1.0}     # (never below: the white of an exhausted depth; rtdev_sum_exponent refuses 0.5)
                | {2.0 ** k * f for k in range(1, 41) for f in (1.0, 1 - 5e-7, 1 - 2e-6)}
                | {2.0 ** 30 * (1 - 1e-15), 2.0 ** 30 * (1 + 2e-16), 2.0 ** 29 * (1 + 1e-9)})
SAMPLES = [1, 24, 1000, 32752, 32768,            # longest chunk <= 2048 (exactly 2048 from 32 752 on)
           32769, 32784, 40000,                  # just above: one halving
           65536, 65537, 131073, 1000000, 1 << 24]


def test_chunk_plan_replica_matches_the_library(rt):
    """The test's copy of chunk_plan against the library's rule: a bound of 1 has e = 1 plus one per halving of the
    longest chunk — and the plans stay within RT_MAX_CHUNKS."""
    assert longest_chunk(32768) == 2048 and longest_chunk(32752) == 2048 and longest_chunk(32769) > 2048
    for samples in SAMPLES + [2, 9, 63, 64, 65, 257, 2049, 4096, 65535, 99999, 262144]:
        plan = chunk_plan(samples)
        assert plan[0] == 0 and plan[-1] == samples and len(plan) - 1 <= MAX_CHUNKS
        assert rt.sum_exponent(1.0, samples) == 1 + halvings(longest_chunk(samples))[0], samples


@pytest.mark.parametrize("samples", SAMPLES)
def test_the_scale_rule_fits_the_sums_and_the_budget(rt, samples):
    longest = longest_chunk(samples)
    h, per_sum = halvings(longest)
    for bound in BOUNDS:
        mantissa, e0 = math.frexp(bound)
        if mantissa > 1 - 1e-6:
            e0 += 1
        try:
            e = rt.sum_exponent(bound, samples)
        except rt.RtError as err:  # refused: no exponent within the budget holds these chunks
            assert err.code == abi.RT_ERR_UNSUPPORTED
            assert "RT_ARITH_REFERENCE" in str(err)
            assert e0 + h > 31 and bound < 2.0 ** 30, (bound, samples)
            continue
        if e == 0:  # f64 sums: only a bound the budget cannot hold
            assert bound >= 2.0 ** 30, (bound, samples)
            continue
        assert e <= e0 + h, (bound, samples, e)           # not coarser than the chunk needs
        # 1. a sample at the bound — or a few ulps above it (sky blends, Noise crests, twenty bounces) — fits 52 bits
        top = bound * (1 + 64 * 2.0 ** -52)
        assert top * 2.0 ** (52 - e) < 2.0 ** 52, (bound, samples, e)
        # 2. the longest chunk of such integers fits the 64-bit sum (and its 2^52 exponent fields, taken off in start_item)
        assert longest * math.floor(top * 2.0 ** (52 - e) + 1) <= 2.0 ** 63, (bound, samples, e)
        assert longest * 2.0 ** (52 - (e - e0)) <= 2.0 ** 63, (bound, samples, e)
        # 3. the quantum stays inside the budget: a dark pixel's gamma-encoded value is off by at most sqrt(2^(e-53))
        assert math.sqrt(2.0 ** (e - 53)) <= BUDGET, (bound, samples, e)


def test_the_cap_on_both_sides(rt):
    below, at = 2.0 ** 30 * (1 - 1e-15), 2.0 ** 30
    assert rt.sum_exponent(below, 32768) == 31
    assert rt.sum_exponent(at, 32768) == 0 and rt.sum_exponent(2.0 ** 39, 64) == 0
    assert rt.sum_exponent(0.0, 64) == 0                       # a scene without a bound
    with pytest.raises(rt.RtError) as err:                     # one halving more would be e = 32
        rt.sum_exponent(below, 32769)
    assert err.value.code == abi.RT_ERR_UNSUPPORTED
    assert rt.sum_exponent(2.0 ** 30 * (1 - 2e-6), 32769) == 31  # e = 30 before the halving
    for bad in (-1.0, 0.5):
        with pytest.raises(rt.RtError) as err:
            rt.sum_exponent(bad, 64)
        assert err.value.code == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(rt.RtError):
        rt.sum_exponent(16.0, 0)


# ---- 3. the rounding model: dark walls under a bright light -------------------------------------------------------------

def dark_under_bright(emission):
    """cornell_box_boxes with a light of `emission` and walls (and boxes) of albedo 0.45 2^-12 / emission: a path that
    bounces once off a wall brings 1.1e-4 whatever the light — a dark pixel whose error is the sums' quantum."""
    bundle, cam, _ = S.cornell_box_boxes()
    a = 0.45 * 2.0 ** -12 / emission
    textures = [abi.solid((a, a, a))] * 3 + [abi.solid((emission,) * 3)]
    return abi.SceneBundle(list(bundle.primitives), list(bundle.materials), textures, abi.solid_background((0.0, 0.0, 0.0))), cam


EMISSIONS = sorted({2.0 ** k * f for k in range(4, 41) for f in (1.0, 1 - 5e-7, 1 - 2e-6)})


def test_rounding_model_of_dark_walls_under_a_bright_light(rt, orc):
    """The kernel's rounding applied to the oracle's samples, at every emission the host accepts for fixed-point sums:
    gamma-encoded, the frame stays within 1e-3 of the f64 sums.  (With the bound capped at 2^40, as it once was, E = 2^39
    took e = 40 and the frame was 2.6e-3 off, 13 % of its pixels beyond 1e-3.)"""
    w, h, spp = 24, 24, 32
    accepted = []
    for emission in EMISSIONS:
        bundle, cam = dark_under_bright(emission)
        bound = rt.radiance_bound(bundle)
        if bound == 0.0:
            continue
        assert bound == emission
        e = rt.sum_exponent(bound, spp)
        accepted.append(emission)
        T = sample_radiances(bundle.desc, S.camera_for(cam, w, h), abi.render_params(w, h, spp), use_bvh=0)
        assert T.max() <= bound
        ref = f64_frame(T)
        got = fixed_point_frame(T, e)
        assert np.abs(got - ref).max() < TOL, (emission, e, np.abs(got - ref).max())
        assert np.abs(got ** 2 - ref ** 2).max() <= 2.0 ** (e - 53) * (1 + 1e-9), (emission, e)
        assert ((T > 0) & (T < 1e-3)).mean() > 0.01        # the wall samples are there
    assert max(accepted) >= 2.0 ** 29 and len(accepted) >= 3 * 26 - 1
