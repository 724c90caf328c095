"""The denoiser without a device: the numpy model of DESIGN.md 4.6 (tests/denoise_model.py) on synthetic input and on
oracle renders, and the C ABI's shape — exported symbols, struct layouts against gcc, the defaults, and every refusal that
comes before a device is touched."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_model as M
import denoise_reference as R
import scenes_py as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
abi = S.abi
ENTRY_POINTS = ("rt_denoise_params_default", "rt_render_guides_device", "rt_denoise_device", "rt_denoise_frame",
                "rt_render_progressive_denoised")


# ---- the model on synthetic input -----------------------------------------------------------------------------------

SETTINGS = [dict(), dict(flags=0), dict(sigma_color=0.5), dict(sigma_normal=0.0, sigma_plane=0.0),
            dict(iterations=1), dict(iterations=10, sigma_color=2.0)]


@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "defaults")
def test_a_constant_radiance_stays_constant(kw):
    g, _ = M.synthetic_guides()
    flags = kw.get("flags", M.DEMODULATE)
    L = np.full(g["albedo"].shape, 0.3)
    want = np.sqrt(L)
    if flags & M.DEMODULATE:   # constant demodulated radiance: the frame carries the (clamped) albedo, the output the albedo
        L = L * np.maximum(g["albedo"], 1e-3)
        want = np.sqrt(0.3 * g["albedo"])
    rgb = np.sqrt(L)
    out = M.denoise(rgb, g, **kw)
    assert np.max(np.abs(out - want)) < 1e-12


def test_zero_iterations_is_an_exact_copy():
    g, rng = M.synthetic_guides()
    rgb = rng.uniform(0.0, 2.0, g["albedo"].shape)
    for flags in (0, M.DEMODULATE):
        out = M.denoise(rgb, g, iterations=0, flags=flags, sigma_color=1.0)
        assert np.array_equal(out, rgb) and out is not rgb


@pytest.mark.parametrize("kw", SETTINGS[:4], ids=["defaults", "no-demod", "colour", "no-stops"])
def test_every_output_is_a_convex_combination_of_its_objects_inputs(kw):
    g, rng = M.synthetic_guides()
    rgb = rng.uniform(0.0, 2.0, g["albedo"].shape)
    I = rgb * rgb
    if kw.get("flags", M.DEMODULATE) & M.DEMODULATE:
        I = I / np.maximum(g["albedo"], 1e-3)
    kw = dict(kw, iterations=1)   # one level: each output is a weighted mean of ITS taps' inputs
    flags = kw.get("flags", M.DEMODULATE)
    out_I = M.atrous(I, g, 0, kw.get("sigma_color", 0.0), kw.get("sigma_normal", 0.1), kw.get("sigma_plane", 1.0))
    for oid in (1, 2):
        m = g["obj_id"] == oid
        lo, hi = I[m].min(axis=0), I[m].max(axis=0)
        assert np.all(out_I[m] >= lo - 1e-12) and np.all(out_I[m] <= hi + 1e-12)
    # ... and after five levels too, per object, in demodulated space
    # (out^2 = I_5 albedo: the bounds are carried to the output, where an albedo below the clamp or 0 leaves I_5 unreadable)
    out = M.denoise(rgb, g, **dict(kw, iterations=5))
    L = out * out
    a = g["albedo"] if flags & M.DEMODULATE else np.ones_like(L)
    for oid in (1, 2):
        m = g["obj_id"] == oid
        assert np.all(L[m] >= I[m].min(axis=0) * a[m] * (1 - 1e-12) - 1e-12)
        assert np.all(L[m] <= I[m].max(axis=0) * a[m] * (1 + 1e-12) + 1e-12)


def test_an_object_takes_nothing_from_its_neighbours():
    g, rng = M.synthetic_guides()
    rgb = rng.uniform(0.0, 1.0, g["albedo"].shape)
    other = rgb.copy()
    other[g["obj_id"] == 2] *= 5.0    # change object 2 only
    a, b = M.denoise(rgb, g), M.denoise(other, g)
    assert np.array_equal(a[g["obj_id"] == 1], b[g["obj_id"] == 1])


def test_misses_pass_through():
    g, rng = M.synthetic_guides()
    rgb = rng.uniform(0.0, 3.0, g["albedo"].shape)
    for kw in SETTINGS:
        out = M.denoise(rgb, g, **kw)
        miss = g["obj_id"] < 0
        # (albedo 1 on a miss; sqrt(g * g) == g for every non-negative double that neither underflows nor overflows)
        assert np.array_equal(out[miss], rgb[miss])


# ---- the model against the independent reference (tests/denoise_reference.py) ---------------------------------------

REF_SHAPES = [(2, 2), (9, 2), (13, 9), (17, 11)]     # (width, height): odd, and wider than tall and taller than wide
# a pairwise list: iterations 0, 1, 2, 5 and 10; each stop on and off; demodulation on and off
REF_SETTINGS = [dict(iterations=0, sigma_color=1.0),
                dict(iterations=1),
                dict(iterations=1, flags=0, sigma_normal=0.0, sigma_color=4.0),
                dict(iterations=2, sigma_plane=0.0, sigma_color=4.0),
                dict(iterations=2, flags=0, sigma_normal=0.0, sigma_plane=0.0),
                dict(iterations=5, sigma_color=1.0),
                dict(iterations=5, flags=0, sigma_plane=0.0),
                dict(iterations=10, sigma_color=40.0),
                dict(iterations=10, flags=0, sigma_normal=0.0, sigma_color=0.5)]
REL = 1e-12


def reference_mismatch(got, ref):
    return M.mismatch(got, ref, REL)


def _shape_id(s):
    return "%dx%d" % s


def _setting_id(kw):
    return ",".join("%s=%s" % i for i in kw.items())


@pytest.mark.parametrize("shape", REF_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("kw", REF_SETTINGS, ids=_setting_id)
def test_the_model_matches_the_independent_reference(shape, kw):
    w, h = shape
    g, rng = M.synthetic_guides(h, w, seed=100 * w + h)
    rgb = M.synthetic_frame(g, rng)
    ref = np.asarray(R.denoise(rgb, g, **kw))
    assert ref.shape == rgb.shape and np.all(np.isfinite(ref))
    got = M.denoise(rgb, g, **kw)
    assert reference_mismatch(got, ref) == 0, np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))
    if kw["iterations"] == 0:
        assert np.array_equal(ref, rgb)


def test_the_synthetic_guides_reach_the_corners():
    g, rng = M.synthetic_guides(11, 17, seed=1711)
    rgb = M.synthetic_frame(g, rng)
    ids, alb, hit = g["obj_id"], g["albedo"], g["obj_id"] >= 0
    assert (alb[hit] == 0.0).any() and ((alb[hit] > 0.0) & (alb[hit] < 1e-3)).any()
    assert (rgb[hit] == 0.0).all(axis=-1).any() and rgb.max() > 300.0
    inner = ids[1:-1, 1:-1]
    assert (inner < 0).any(), "no miss inside the frame"
    island = (inner != ids[:-2, 1:-1]) & (inner != ids[2:, 1:-1]) & (inner != ids[1:-1, :-2]) & (inner != ids[1:-1, 2:])
    assert (island & (inner >= 0)).any(), "no single-pixel object"
    fp = g["footprint"]
    both = hit[:, 1:] & hit[:, :-1]
    assert np.max(np.maximum(fp[:, 1:], fp[:, :-1])[both] / np.minimum(fp[:, 1:], fp[:, :-1])[both]) > 5.0


@pytest.mark.parametrize("kw", [dict(iterations=1), dict(iterations=2), dict(iterations=3, sigma_color=40.0)],
                         ids=_setting_id)
def test_the_reference_tells_the_plane_stops_footprint_apart(kw):
    """Dividing the plane distance by the neighbour's footprint instead of the centre's is caught."""
    g, rng = M.synthetic_guides(11, 17, seed=1711)
    rgb = M.synthetic_frame(g, rng)
    ref = np.asarray(R.denoise(rgb, g, **kw))
    assert reference_mismatch(np.asarray(R.denoise(rgb, g, footprint_of="q", **kw)), ref) > 50


@pytest.mark.parametrize("kw", [dict(iterations=2, sigma_color=40.0), dict(iterations=3, sigma_color=4.0)],
                         ids=_setting_id)
def test_the_reference_tells_the_colour_stop_schedule_apart(kw):
    """A colour stop of sigma_c at every level instead of sigma_c 2^-i is caught."""
    g, rng = M.synthetic_guides(11, 17, seed=1711)
    rgb = M.synthetic_frame(g, rng)
    ref = np.asarray(R.denoise(rgb, g, **kw))
    assert reference_mismatch(np.asarray(R.denoise(rgb, g, color_halves=False, **kw)), ref) > 50


# ---- the model on oracle renders ------------------------------------------------------------------------------------

def test_the_model_halves_the_error_of_a_16_spp_cornell_box_boxes(orc):
    w = h = 128
    bundle, cam, _ = S.cornell_box_boxes()
    c = S.camera_for(cam, w, h)
    guides = M.oracle_guides(orc, bundle, c, w, h)
    assert np.mean(guides["obj_id"] >= 1) > 0.8    # (the rest looks past the open box into the black background)
    ref, _ = orc.render(bundle.desc, c, abi.render_params(w, h, 512, seed=7))
    noisy, _ = orc.render(bundle.desc, c, abi.render_params(w, h, 16, seed=1))
    raw = M.gamma_rmse(noisy, ref)
    den = M.gamma_rmse(M.denoise(noisy, guides), ref)
    assert raw / den >= 1.8, (raw, den)


# ---- the C ABI without a device -------------------------------------------------------------------------------------

def test_the_entry_points_are_exported_and_bound(rt):
    lib = C.CDLL(rt.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in rt.abi.PROTOTYPES and hasattr(lib, name), name


def test_the_struct_layouts_match_the_c_compiler():
    structs = ["RtDenoiseParams", "RtGuides"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', 'int main(void){']
    for s in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, name, s, name))
    lines.append('printf("RT_DENOISE_DEMODULATE %d\\n", (int)RT_DENOISE_DEMODULATE);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", INC, "-o", exe, src])
        want = dict(l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l)
    for s in structs:
        cls = getattr(abi, s)
        assert C.sizeof(cls) == int(want[s]), s
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == int(want["%s.%s" % (s, name)]), (s, name)
    assert int(want["RT_DENOISE_DEMODULATE"]) == abi.RT_DENOISE_DEMODULATE == M.DEMODULATE


def test_the_defaults(rt):
    dp = rt.denoise_params()
    assert (dp.iterations, dp.flags, dp.sigma_color) == (5, abi.RT_DENOISE_DEMODULATE, 0.0)
    assert (dp.sigma_normal, dp.sigma_plane) == (0.1, 1.0)
    assert list(dp._reserved) == [0, 0, 0, 0]
    rt.lib().rt_denoise_params_default(None)   # a NULL is ignored


def _bad_params():
    """(what, RtRenderParams, RtDenoiseParams) that every entry point refuses"""
    ok = abi.render_params(64, 36, 8)
    out = []
    for it in (-1, 11):
        out.append(("iterations", ok, _dp(iterations=it)))
    for name in ("sigma_color", "sigma_normal", "sigma_plane"):
        for v in (float("nan"), float("inf"), -float("inf")):
            out.append(("finite", ok, _dp(**{name: v})))
    bad = _dp()
    bad._reserved[2] = 1
    out.append(("_reserved", ok, bad))
    out.append(("strip", abi.render_params(64, 36, 8, strip_rows=8, strip_count=2, strip_index=0), _dp()))
    out.append(("scale", abi.render_params(64, 36, 8, scale=4), _dp()))
    return out


def _dp(**kw):
    dp = abi.RtDenoiseParams()
    dp.iterations, dp.flags, dp.sigma_normal, dp.sigma_plane = 5, 1, 0.1, 1.0
    for k, v in kw.items():
        setattr(dp, k, v)
    return dp


def _calls(rt, params, dp, rgb=None, out=None, guides=None):
    """Every entry point with a NULL scene (scene-independent refusals come first)."""
    lib = rt.lib()
    cam = abi.RtCamera()
    a = (C.c_double * 3)()
    b = (C.c_double * 3)()
    rgb = a if rgb is None else rgb
    out = b if out is None else out
    g = guides if guides is not None else abi.RtGuides(1, 2, 3, 4, 5)   # never dereferenced: the calls are refused first
    cb = abi.RtFrameCallback(lambda *_: None)
    none = C.cast(None, abi.RtCancelCallback)
    return {
        "rt_denoise_frame": lambda: lib.rt_denoise_frame(None, C.byref(cam), C.byref(params), C.byref(dp), rgb, out),
        "rt_denoise_device": lambda: lib.rt_denoise_device(None, C.byref(params), C.byref(dp), C.cast(rgb, C.c_void_p),
                                                           C.byref(g), C.cast(out, C.c_void_p), None),
        "rt_render_progressive_denoised": lambda: lib.rt_render_progressive_denoised(None, C.byref(cam), C.byref(params), 8,
                                                                                     C.byref(dp), cb, None, none, None),
    }


@pytest.mark.parametrize("case", range(len(_bad_params())))
def test_bad_filter_parameters_are_refused_before_a_device(rt, case):
    what, params, dp = _bad_params()[case]
    for name, call in _calls(rt, params, dp).items():
        assert call() == abi.RT_ERR_INVALID_ARGUMENT, (name, what)
        msg = rt.lib().rt_last_error_message().decode()
        assert what in msg and "scene is NULL" not in msg, (name, msg)
    if what in ("strip", "scale"):   # the guides take no filter parameters, but whole frames only
        assert rt.lib().rt_render_guides_device(None, C.byref(abi.RtCamera()), C.byref(params),
                                                C.byref(abi.RtGuides(1, 2, 3, 4, 5)), None) == abi.RT_ERR_INVALID_ARGUMENT
        assert what in rt.lib().rt_last_error_message().decode()


def test_null_pointers_are_refused(rt):
    lib = rt.lib()
    params, dp, cam = abi.render_params(64, 36, 8), _dp(), abi.RtCamera()
    buf = (C.c_double * 3)()
    assert lib.rt_denoise_frame(None, C.byref(cam), C.byref(params), None, buf, buf) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_denoise_frame(None, C.byref(cam), None, C.byref(dp), buf, buf) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_denoise_frame(None, C.byref(cam), C.byref(params), C.byref(dp), None, buf) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_denoise_frame(None, C.byref(cam), C.byref(params), C.byref(dp), buf, None) == abi.RT_ERR_INVALID_ARGUMENT
    other = (C.c_double * 3)()
    assert lib.rt_denoise_frame(None, C.byref(cam), C.byref(params), C.byref(dp), buf, other) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"scene is NULL" in lib.rt_last_error_message()
    for hole in range(5):
        ptrs = [1, 2, 3, 4, 5]
        ptrs[hole] = 0
        g = abi.RtGuides(*ptrs)
        assert lib.rt_render_guides_device(None, C.byref(cam), C.byref(params), C.byref(g), None) == abi.RT_ERR_INVALID_ARGUMENT
        assert b"guides_device" in lib.rt_last_error_message()
        assert lib.rt_denoise_device(None, C.byref(params), C.byref(dp), C.cast(buf, C.c_void_p), C.byref(g),
                                     C.cast(other, C.c_void_p), None) == abi.RT_ERR_INVALID_ARGUMENT
        assert b"guides_device" in lib.rt_last_error_message()
    assert lib.rt_render_guides_device(None, C.byref(cam), C.byref(params), None, None) == abi.RT_ERR_INVALID_ARGUMENT
    cb = abi.RtFrameCallback(lambda *_: None)
    none = C.cast(None, abi.RtCancelCallback)
    assert lib.rt_render_progressive_denoised(None, C.byref(cam), C.byref(params), 8, None, cb, None, none,
                                              None) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_render_progressive_denoised(None, C.byref(cam), C.byref(params), 8, C.byref(dp), cb, None, none,
                                              None) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"scene is NULL" in lib.rt_last_error_message()


def test_the_input_and_output_must_differ(rt):
    lib = rt.lib()
    params, dp, cam = abi.render_params(64, 36, 8), _dp(), abi.RtCamera()
    buf = (C.c_double * 3)()
    assert lib.rt_denoise_frame(None, C.byref(cam), C.byref(params), C.byref(dp), buf, buf) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"must differ" in lib.rt_last_error_message()
    g = abi.RtGuides(1, 2, 3, 4, 5)
    assert lib.rt_denoise_device(None, C.byref(params), C.byref(dp), C.cast(buf, C.c_void_p), C.byref(g),
                                 C.cast(buf, C.c_void_p), None) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"must differ" in lib.rt_last_error_message()
