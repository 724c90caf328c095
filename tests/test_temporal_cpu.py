"""Temporal accumulation without a device: the numpy model of DESIGN.md 4.11 (tests/temporal_model.py) against closed
forms, the C ABI's shape — exported symbols, struct layouts against gcc, the defaults, every refusal that comes before a
device is touched — and the margin condition the GPU tests rely on."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_model as M
import scenes_py as S
import temporal_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
abi = S.abi
ENTRY_POINTS = ("rt_temporal_params_default", "rt_temporal_accumulate_device", "rt_denoise_history_device",
                "rt_temporal_create", "rt_temporal_destroy", "rt_temporal_reset", "rt_render_temporal")
W, H = 64, 48
SCENES = {"cornell_box_boxes": S.cornell_box_boxes, "three_balls": S.three_balls}


@pytest.fixture(scope="module")
def orbit_guides(orc):
    """Per scene: (camera A, guides A, camera B = A orbited 2 degrees about look_at, guides B), with the oracle, 64x48."""
    out = {}
    for name, make in SCENES.items():
        bundle, cam = make()[:2]
        a, b = S.camera_for(cam, W, H), S.camera_for(T.orbit(cam, 2.0), W, H)
        out[name] = (a, M.oracle_guides(orc, bundle, a, W, H), b, M.oracle_guides(orc, bundle, b, W, H))
    return out


def _frame(rng, shape):
    return rng.uniform(0.2, 1.5, shape + (3,))


# ---- closed forms -----------------------------------------------------------------------------------------------------

def _plane_guides(cam, w, h, depth):
    """The guides of the plane z = -depth (object 1, albedo textured by position) under a pinhole camera."""
    o, ulc, hor, ver = T.camera_vectors(cam)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u, v = (xs + 0.5) / (w - 1), (ys + 0.5) / (h - 1)
    d = ulc + u[..., None] * hor - v[..., None] * ver - o
    t = (-depth - o[2]) / d[..., 2]
    x = o + t[..., None] * d
    n = np.zeros((h, w, 3))
    n[..., 2] = 1.0
    albedo = 0.3 + 0.2 * np.stack([np.sin(3 * x[..., 0]), np.cos(2 * x[..., 1]), np.sin(x[..., 0] + x[..., 1])], axis=-1) ** 2
    return {"normal": n, "position": x, "albedo": albedo, "footprint": t * np.linalg.norm(ver) / (h - 1),
            "obj_id": np.ones((h, w), dtype=np.int32)}


@pytest.mark.parametrize("k", [1, 3, -2])
def test_a_translation_by_whole_pixels_reprojects_onto_one_tap(orc, k):
    w, h, depth = 40, 30, 5.0
    cam_a = orc.camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 40.0, 0.0, 1.0, w, h)
    ga = _plane_guides(cam_a, w, h, depth)
    pitch = ga["position"][0, 1, 0] - ga["position"][0, 0, 0]     # one pixel footprint along x on the plane
    cam_b = orc.camera((k * pitch, 0.0, 0.0), (k * pitch, 0.0, -1.0), 40.0, 0.0, 1.0, w, h)
    gb = _plane_guides(cam_b, w, h, depth)
    rng = np.random.default_rng(5)
    prev = T.first_history(_frame(rng, (h, w)), ga, flags=0)
    prev["length"][:] = 3.0
    rgb = _frame(rng, (h, w))
    out, info = T.accumulate(rgb, gb, prev, T.camera_vectors(cam_a), flags=0, alpha=0.0)
    sx, sy = info["shift"]
    assert np.max(np.abs(sx - k)) < 1e-9 and np.max(np.abs(sy)) < 1e-9
    xs = np.arange(w)
    interior = (xs + k >= 1) & (xs + k < w - 1)
    assert not info["fresh"][:, interior].any()
    want = 0.75 * np.roll(prev["radiance"], -k, axis=1) + 0.25 * rgb * rgb      # N = 4: a = 1/4
    err = np.abs(out["radiance"] - want)[:, interior]
    assert err.max() < 1e-9
    assert np.all(np.abs(out["length"][:, interior] - 4.0) < 1e-9)
    outside = (xs + k < -1) | (xs + k > w)
    assert info["fresh"][:, outside].all() and np.array_equal(out["radiance"][:, outside], (rgb * rgb)[:, outside])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_identical_camera_returns_every_hit_pixels_own_history(orbit_guides, name):
    cam, g = orbit_guides[name][:2]
    rng = np.random.default_rng(11)
    rgb = _frame(rng, (H, W))
    prev = T.first_history(rgb, g)
    out, info = T.accumulate(rgb, g, prev, T.camera_vectors(cam), alpha=0.0)      # the same frame again: C_p = C_h
    hit = g["obj_id"] >= 0
    sx, sy = info["shift"]
    assert np.max(np.abs(sx[hit])) < 1e-12 * W and np.max(np.abs(sy[hit])) < 1e-12 * H
    assert not info["fresh"][hit].any() and info["fresh"][~hit].all()
    assert np.max(np.abs(out["radiance"][hit] - prev["radiance"][hit]) / prev["radiance"][hit]) < 1e-12
    assert np.all(out["length"][hit] == 2.0) and np.all(out["length"][~hit] == 1.0)


def test_alpha_zero_over_k_frames_is_the_arithmetic_mean(orbit_guides):
    cam, g = orbit_guides["cornell_box_boxes"][:2]
    rng = np.random.default_rng(12)
    frames = [_frame(rng, (H, W)) for _ in range(6)]
    hist = None
    for f in frames:
        hist, _ = T.accumulate(f, g, hist, T.camera_vectors(cam) if hist is not None else None, alpha=0.0,
                               alpha_moments=0.0, max_history=1e9)
    hit = g["obj_id"] >= 0
    C = [T.demodulate(f, g) for f in frames]
    mean = sum(C) / 6.0
    assert np.max(np.abs(hist["radiance"][hit] - mean[hit]) / mean[hit]) < 1e-12
    l = [T.luminance(c) for c in C]
    m1, m2 = (sum(l) / 6.0)[hit], (sum(v * v for v in l) / 6.0)[hit]
    assert np.max(np.abs(hist["moments"][hit][:, 0] - m1) / m1) < 1e-12
    assert np.max(np.abs(hist["moments"][hit][:, 1] - m2) / m2) < 1e-12
    assert np.all(np.abs(hist["length"][hit] - 6.0) < 1e-12)
    # ... and max_history caps the length, after which the blend factor stays at 1 / (max_history + 1)
    capped = None
    for f in frames:
        capped, _ = T.accumulate(f, g, capped, T.camera_vectors(cam) if capped is not None else None, alpha=0.0, max_history=2.0)
    assert np.all(np.abs(capped["length"][hit] - 2.0) < 1e-12)


SETTINGS = [dict(), dict(flags=0), dict(sigma_color=0.5), dict(iterations=1), dict(iterations=10, sigma_color=2.0)]


@pytest.mark.parametrize("sl", [0.0, -1.0])
@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "defaults")
def test_without_the_luminance_stop_the_filter_is_denoise_models(kw, sl):
    g, rng = M.synthetic_guides()
    rgb = M.synthetic_frame(g, rng)
    hist = T.first_history(rgb, g, flags=kw.get("flags", M.DEMODULATE))
    got = T.denoise_history(hist, g, sigma_luminance=sl, **kw)
    assert np.array_equal(got, M.denoise(rgb, g, **kw))


def test_a_constant_variance_is_scaled_by_the_squared_weights():
    """var' = var * sum w^2 / (sum w)^2, against a hand sum at one pixel of a tilted plane."""
    h, w = 16, 20
    rng = np.random.default_rng(21)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    n = np.tile(np.array([0.0, 0.6, 0.8]), (h, w, 1)) + rng.normal(0.0, 0.02, (h, w, 3))
    x = np.stack([xs * 0.1, ys * 0.1, rng.normal(0.0, 0.01, (h, w))], axis=-1)
    g = {"normal": n, "position": x, "albedo": np.ones((h, w, 3)), "footprint": np.full((h, w), 0.1),
         "obj_id": np.ones((h, w), dtype=np.int32)}
    I = rng.uniform(0.5, 1.5, (h, w, 3))
    v0 = 0.04
    var = np.full((h, w), v0)
    sn, sx, sl = 0.1, 1.0, 2.0
    out, var_out = T.atrous_var(I, var, g, 1, sigma_normal=sn, sigma_plane=sx, sigma_luminance=sl)
    py, px, step = 7, 9, 2
    lum = lambda c: 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]
    s1 = s2 = 0.0
    acc = np.zeros(3)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            q = (py + dy * step, px + dx * step)
            wt = M.H5[dx + 2] * M.H5[dy + 2]
            wt *= math.exp(-float(np.sum((n[py, px] - n[q]) ** 2)) / (sn * sn))
            d = float(np.dot(n[py, px], x[q] - x[py, px])) / (sx * step * 0.1)
            wt *= math.exp(-d * d)
            wt *= math.exp(-abs(lum(I[py, px]) - lum(I[q])) / (sl * math.sqrt(v0) + 1e-10))
            s1 += wt
            s2 += wt * wt
            acc += wt * I[q]
    assert abs(var_out[py, px] - v0 * s2 / (s1 * s1)) < 1e-14
    assert np.max(np.abs(out[py, px] - acc / s1)) < 1e-14
    assert v0 / 25.0 <= var_out[py, px] < v0   # an average of up to 25 taps


def test_the_variance_takes_the_moments_where_the_history_is_long_enough():
    g, rng = M.synthetic_guides()
    hist = T.first_history(M.synthetic_frame(g, rng), g)
    hist["length"] = rng.choice([1.0, 2.0, 3.5, 4.0, 7.0, 40.0], hist["length"].shape)
    hist["moments"][..., 1] += rng.uniform(0.0, 0.5, hist["length"].shape)
    var = T.variance(hist, g)
    hit, long = g["obj_id"] >= 0, hist["length"] >= 4.0
    m = hist["moments"]
    assert np.all(var[~hit] == 0.0)
    want = np.maximum(0.0, m[..., 1] - m[..., 0] ** 2) / hist["length"]
    assert np.array_equal(var[hit & long], want[hit & long]) and (hit & long).any() and (hit & ~long).any()
    island = hit & ~long & (g["obj_id"] == 7)     # a single-pixel object sees itself alone: no spatial variance
    assert island.any() and np.all(var[island] < 1e-12 * np.maximum(1.0, m[..., 0][island] ** 2))
    assert np.all(var >= 0.0) and np.all(np.isfinite(var))


# ---- the margin condition ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SCENES))
def test_next_to_no_pixel_sits_on_a_threshold(orbit_guides, name):
    cam_a, ga, cam_b, gb = orbit_guides[name]
    rng = np.random.default_rng(31)
    prev = T.first_history(_frame(rng, (H, W)), ga)
    prev["length"] = rng.choice([1.0, 2.0, 3.5, 7.0, 40.0], (H, W))
    out, info = T.accumulate(_frame(rng, (H, W)), gb, prev, T.camera_vectors(cam_a), **T.DEFAULTS)
    hit = gb["obj_id"] >= 0
    assert np.mean(info["margin"] < 1e-9) <= 0.005
    continued = hit & ~info["fresh"]
    assert continued.sum() >= 0.9 * hit.sum()
    if name == "three_balls":      # disocclusions behind the balls
        assert (hit & info["fresh"]).any() and continued.any()
    # every hit point lies in front of the previous camera
    _, _, s, det = T.reproject(gb["position"], T.camera_vectors(cam_a), W, H)
    assert np.all(s[hit] > 0.0) and np.all(det[hit] != 0.0)


# ---- the C ABI --------------------------------------------------------------------------------------------------------

def test_the_entry_points_are_exported_and_bound(rt):
    lib = C.CDLL(rt.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in rt.abi.PROTOTYPES and hasattr(lib, name), name


def test_the_struct_layouts_match_the_c_compiler():
    structs = ["RtTemporalParams", "RtHistory"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', 'int main(void){']
    for s in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, name, s, name))
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
    assert [n for n, _ in abi.RtHistory._fields_] == list(T.PLANES)


def test_the_defaults(rt):
    tp = rt.temporal_params()
    assert (tp.alpha, tp.alpha_moments, tp.max_history) == (0.2, 0.2, 32.0)
    got = {k: getattr(tp, k) for k in T.DEFAULTS}
    assert got == T.DEFAULTS
    assert list(tp._reserved) == [0, 0, 0, 0]
    rt.lib().rt_temporal_params_default(None)   # a NULL is ignored
    assert rt.temporal_params(alpha=0.0, max_history=2.0).max_history == 2.0


def _tp(**kw):
    tp = abi.RtTemporalParams(0.2, 0.2, 32.0, 0.25, 2.0, 4.0)
    for k, v in kw.items():
        setattr(tp, k, v)
    return tp


def _dp(**kw):
    dp = abi.RtDenoiseParams()
    dp.iterations, dp.flags, dp.sigma_normal, dp.sigma_plane = 5, 1, 0.1, 1.0
    for k, v in kw.items():
        setattr(dp, k, v)
    return dp


def _bad():
    """(what the message must name, RtRenderParams, RtDenoiseParams, RtTemporalParams) that every entry point refuses"""
    ok = abi.render_params(64, 36, 8)
    out = []
    for name in ("alpha", "alpha_moments", "max_history", "normal_tolerance", "plane_tolerance", "sigma_luminance"):
        for v in (float("nan"), float("inf"), -float("inf")):
            out.append(("finite", ok, _dp(), _tp(**{name: v})))
    for name in ("alpha", "alpha_moments"):
        for v in (-0.01, 1.01):
            out.append(("alpha", ok, _dp(), _tp(**{name: v})))
    for v in (0.0, 0.99, -3.0):
        out.append(("max_history", ok, _dp(), _tp(max_history=v)))
    bad = _tp()
    bad._reserved[1] = 7
    out.append(("temporal->_reserved", ok, _dp(), bad))
    # ... and what check_denoise refuses about the frame and the filter
    out.append(("iterations", ok, _dp(iterations=11), _tp()))
    out.append(("finite", ok, _dp(sigma_plane=float("nan")), _tp()))
    dbad = _dp()
    dbad._reserved[0] = 1
    out.append(("denoise->_reserved", ok, dbad, _tp()))
    out.append(("strip", abi.render_params(64, 36, 8, strip_rows=8, strip_count=2, strip_index=0), _dp(), _tp()))
    out.append(("scale", abi.render_params(64, 36, 8, scale=4), _dp(), _tp()))
    return out


def _calls(rt, params, dp, tp):
    """Every code-returning entry point that takes parameters, with a NULL scene (scene-independent refusals come first)."""
    lib = rt.lib()
    cam = abi.RtCamera()
    buf = (C.c_double * 3)()
    g = abi.RtGuides(1, 2, 3, 4, 5)             # never dereferenced: the calls are refused first
    h1, h2 = abi.RtHistory(1, 2, 3, 4, 5, 6), abi.RtHistory(11, 12, 13, 14, 15, 16)
    return {
        "rt_temporal_accumulate_device": lambda: lib.rt_temporal_accumulate_device(
            None, C.byref(params), C.byref(tp), C.byref(dp), C.cast(buf, C.c_void_p), C.byref(g), C.byref(cam), C.byref(h1),
            C.byref(h2), None),
        "rt_denoise_history_device": lambda: lib.rt_denoise_history_device(
            None, C.byref(params), C.byref(dp), C.byref(tp), C.byref(h1), C.byref(g), C.cast(buf, C.c_void_p), None),
        "rt_render_temporal": lambda: lib.rt_render_temporal(None, None, C.byref(cam), C.byref(params), C.byref(tp),
                                                             C.byref(dp), buf, None),
    }


@pytest.mark.parametrize("case", range(len(_bad())))
def test_bad_parameters_are_refused_before_a_device(rt, case):
    what, params, dp, tp = _bad()[case]
    for name, call in _calls(rt, params, dp, tp).items():
        assert call() == abi.RT_ERR_INVALID_ARGUMENT, (name, what)
        msg = rt.lib().rt_last_error_message().decode()
        assert what in msg and "scene is NULL" not in msg and "temporal_state" not in msg, (name, msg)


def test_null_pointers_and_aliases_are_refused(rt):
    lib = rt.lib()
    params, dp, tp, cam = abi.render_params(64, 36, 8), _dp(), _tp(), abi.RtCamera()
    buf = (C.c_double * 3)()
    ptr = C.cast(buf, C.c_void_p)
    g = abi.RtGuides(1, 2, 3, 4, 5)
    h1, h2 = abi.RtHistory(1, 2, 3, 4, 5, 6), abi.RtHistory(11, 12, 13, 14, 15, 16)
    E = abi.RT_ERR_INVALID_ARGUMENT
    msg = lambda: lib.rt_last_error_message().decode()
    P, D, Tp, G, Cm, H1, H2 = (C.byref(v) for v in (params, dp, tp, g, cam, h1, h2))

    acc = lib.rt_temporal_accumulate_device
    assert acc(None, None, Tp, D, ptr, G, Cm, H1, H2, None) == E
    assert acc(None, P, None, D, ptr, G, Cm, H1, H2, None) == E and "temporal is NULL" in msg()
    assert acc(None, P, Tp, None, ptr, G, Cm, H1, H2, None) == E
    assert acc(None, P, Tp, D, None, G, Cm, H1, H2, None) == E and "rgb_device" in msg()
    assert acc(None, P, Tp, D, ptr, None, Cm, H1, H2, None) == E and "guides_device" in msg()
    assert acc(None, P, Tp, D, ptr, G, Cm, H1, None, None) == E and "out_history" in msg()
    assert acc(None, P, Tp, D, ptr, G, None, H1, H2, None) == E and "both NULL" in msg()
    assert acc(None, P, Tp, D, ptr, G, Cm, None, H2, None) == E and "both NULL" in msg()
    assert acc(None, P, Tp, D, ptr, G, Cm, H1, H1, None) == E and "must differ" in msg()
    for hole in range(6):
        ptrs = [1, 2, 3, 4, 5, 6]
        ptrs[hole] = 0
        holed = abi.RtHistory(*ptrs)
        assert acc(None, P, Tp, D, ptr, G, Cm, H1, C.byref(holed), None) == E and "out_history" in msg()
        assert acc(None, P, Tp, D, ptr, G, Cm, C.byref(holed), H2, None) == E and "prev_history" in msg()
        shared = [11, 12, 13, 14, 15, 16]
        shared[hole] = ptrs[hole] = hole + 1
        assert acc(None, P, Tp, D, ptr, G, Cm, H1, C.byref(abi.RtHistory(*shared)), None) == E and "must differ" in msg()
        assert lib.rt_denoise_history_device(None, P, D, Tp, C.byref(holed), G, ptr, None) == E and "history" in msg()
    for hole in range(5):
        ptrs = [1, 2, 3, 4, 5]
        ptrs[hole] = 0
        assert acc(None, P, Tp, D, ptr, C.byref(abi.RtGuides(*ptrs)), Cm, H1, H2, None) == E and "guides_device" in msg()
    assert acc(None, P, Tp, D, ptr, G, None, None, H2, None) == E and "scene is NULL" in msg()   # a first frame is legal
    assert acc(None, P, Tp, D, ptr, G, Cm, H1, H2, None) == E and "scene is NULL" in msg()

    den = lib.rt_denoise_history_device
    assert den(None, None, D, Tp, H1, G, ptr, None) == E
    assert den(None, P, None, Tp, H1, G, ptr, None) == E
    assert den(None, P, D, None, H1, G, ptr, None) == E and "temporal is NULL" in msg()
    assert den(None, P, D, Tp, None, G, ptr, None) == E and "history" in msg()
    assert den(None, P, D, Tp, H1, None, ptr, None) == E and "guides_device" in msg()
    assert den(None, P, D, Tp, H1, G, None, None) == E and "out_device" in msg()
    assert den(None, P, D, Tp, H1, G, C.c_void_p(1), None) == E and "must differ" in msg()
    assert den(None, P, D, Tp, H1, G, ptr, None) == E and "scene is NULL" in msg()

    ren = lib.rt_render_temporal
    assert ren(None, None, None, P, Tp, D, buf, None) == E
    assert ren(None, None, Cm, None, Tp, D, buf, None) == E
    assert ren(None, None, Cm, P, None, D, buf, None) == E
    assert ren(None, None, Cm, P, Tp, None, buf, None) == E
    assert ren(None, None, Cm, P, Tp, D, None, None) == E and "out_rgb_host" in msg()
    assert ren(None, None, Cm, P, Tp, D, buf, None) == E and "temporal_state is NULL" in msg()
    zero = abi.render_params(64, 36, 0)
    assert ren(None, None, Cm, C.byref(zero), Tp, D, buf, None) == E and "samples" in msg()

    assert lib.rt_temporal_reset(None) == E and "temporal_state is NULL" in msg()
    lib.rt_temporal_destroy(None)               # a NULL is ignored
    assert lib.rt_temporal_create(0, 64, 36, None) == E
    handle = C.c_void_p()
    for w, h in ((1, 36), (64, 1), (0, 0), (-4, 36)):
        assert lib.rt_temporal_create(0, w, h, C.byref(handle)) == E and "at least 2" in msg() and not handle.value
