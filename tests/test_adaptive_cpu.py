"""rt_render_adaptive without a device: the numpy model of its tile error and stop rule on synthetic data, the C ABI's
shape (exported symbols, the struct layout against gcc, the defaults), every refusal it makes before it looks at the
scene, and the CLI's refusals of --adaptive before any device is opened."""
import ctypes as C
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CLI = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
abi = importlib.import_module("racer-tracer_amd.abi")


def _chunk_sums(samples, bounds):
    """samples [n, ...] -> (S, Q) after every chunk of `bounds` (chunk ends, the last one n)"""
    S_all, Q_all, S, Q, prev = [], [], 0.0, 0.0, 0
    for b in bounds:
        Sj = samples[prev:b].sum(axis=0)
        S = S + Sj
        Q = Q + Sj * Sj / (b - prev)
        S_all.append(S)
        Q_all.append(Q)
        prev = b
    return S_all, Q_all


BOUNDS = [24, 48, 72, 84, 92, 96]   # the chunk boundaries of 96 spp (include/rt_abi.h)


# ---- the model ---------------------------------------------------------------------------------------------------------

def test_constant_samples_have_no_error():
    samples = np.full((96, 5, 3), 0.625)
    S, Q = _chunk_sums(samples, BOUNDS)
    for c, b in enumerate(BOUNDS[1:], start=1):
        assert np.array_equal(M.pixel_error(S[c], Q[c], b, c + 1), np.zeros((5, 3)))


def test_a_black_pixel_has_no_error_and_no_nan():
    S, Q = np.zeros((4, 3)), np.zeros((4, 3))
    e = M.pixel_error(S, Q, 96, 6)
    assert np.array_equal(e, np.zeros((4, 3)))


def test_the_two_forms_of_e_agree():
    rng = np.random.default_rng(5)
    samples = rng.exponential(0.3, size=(96, 200, 3)) * (rng.random((96, 200, 3)) < 0.4)
    S, Q = _chunk_sums(samples, BOUNDS)
    for c, b in enumerate(BOUNDS[1:], start=1):
        a, d = M.pixel_error(S[c], Q[c], b, c + 1), M.pixel_error_difference_form(S[c], Q[c], b, c + 1)
        assert np.allclose(a, d, rtol=1e-9, atol=1e-15)
        assert (a >= 0).all() and np.isfinite(a).all()


def test_the_batch_means_variance_is_roughly_unbiased():
    """V estimates the per-sample variance: its mean over many pixels of known variance is within a few per cent."""
    rng = np.random.default_rng(11)
    sd, mean = 0.2, 0.5
    samples = mean + sd * rng.standard_normal((96, 20000))
    S, Q = _chunk_sums(samples, BOUNDS)
    k, s = len(BOUNDS), BOUNDS[-1]
    var = (Q[-1] - S[-1] * (S[-1] / s)) / (k - 1)
    assert abs(var.mean() / sd ** 2 - 1.0) < 0.03
    # ... and sigma is the standard error of the mean that e moves the gamma-encoded value by
    sigma = np.sqrt(np.maximum(var, 0) / s)
    assert abs(np.sqrt(np.mean(sigma ** 2)) / (sd / np.sqrt(s)) - 1.0) < 0.03


def test_the_tile_maximum_covers_in_image_pixels_only():
    e = np.zeros((10, 13, 3))
    e[9, 12, 2] = 0.5
    e[3, 4, 0] = 0.25
    t = M.tile_max(e)
    assert t.shape == (2, 2)
    assert t[1, 1] == 0.5 and t[0, 0] == 0.25 and t[0, 1] == 0 and t[1, 0] == 0


def test_the_model_reads_cumulative_frames():
    """S = f^2 s at every boundary, chunk sums the differences: the model's sums equal the direct ones."""
    rng = np.random.default_rng(3)
    samples = rng.random((96, 6, 7, 3)) ** 3
    S, Q = _chunk_sums(samples, BOUNDS)
    frames = [np.sqrt(Sc / b) for Sc, b in zip(S, BOUNDS)]
    S2, Q2 = M.sums_at_boundaries(frames, BOUNDS)
    for a, b in zip(S, S2):
        assert np.allclose(a, b, rtol=1e-13)
    for a, b in zip(Q, Q2):
        assert np.allclose(a, b, rtol=1e-9)


def test_the_stop_rule():
    """A tile stops at the first pass boundary with >= 4 chunks, >= min_samples and an error <= threshold; none stops with
    threshold <= 0; an error of -1 stands for fewer than 2 chunks."""
    rng = np.random.default_rng(7)
    h, w = 12, 16                                       # two tile columns, two rows (the second one half outside)
    samples = np.full((96, h, w, 3), 0.25)
    samples[:, :, 8:] += 0.3 * rng.standard_normal((96, h, 8, 3))   # the right column is noisy
    samples = np.abs(samples)
    S, _ = _chunk_sums(samples, BOUNDS)
    frames = [np.sqrt(Sc / b) for Sc, b in zip(S, BOUNDS)]
    done, err, per_pass = M.simulate(frames, BOUNDS, BOUNDS, 1e-3, 0)
    assert (done[:, 0] == 84).all() and (done[:, 1] == 96).all()     # 84: the fourth boundary
    assert (err[:, 0] <= 1e-3).all() and (err[:, 1] > 1e-3).all()
    assert (per_pass[24] == -1).all() and (per_pass[48] >= 0).all()
    done, _, _ = M.simulate(frames, BOUNDS, BOUNDS, 1e-3, 90)
    assert (done[:, 0] == 92).all()
    for thr in (0.0, -1.0):
        done, _, _ = M.simulate(frames, BOUNDS, BOUNDS, thr, 0)
        assert (done == 96).all()
    done, _, _ = M.simulate(frames, BOUNDS, [48, 84, 96], 1e9, 0)    # coarser passes: decisions at their ends only
    assert (done == 84).all()
    assert M.expand(done, h, w).shape == (h, w)


# ---- the C ABI without a device --------------------------------------------------------------------------------------

def test_the_entry_points_are_exported_and_bound(rt):
    lib = C.CDLL(rt.LIB_PATH)
    for name in ("rt_adaptive_params_default", "rt_render_adaptive"):
        assert name in rt.abi.PROTOTYPES and hasattr(lib, name), name


def test_the_struct_layout_matches_the_c_compiler():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', 'int main(void){',
             'printf("RtAdaptiveParams %zu\\n", sizeof(RtAdaptiveParams));']
    for name, _ in abi.RtAdaptiveParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(RtAdaptiveParams, %s));' % (name, name))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", INC, "-o", exe, src])
        want = dict(l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l)
    assert C.sizeof(abi.RtAdaptiveParams) == int(want["RtAdaptiveParams"]) == 32
    for name, _ in abi.RtAdaptiveParams._fields_:
        assert getattr(abi.RtAdaptiveParams, name).offset == int(want[name]), name


def test_the_defaults(rt):
    ap = rt.adaptive_params()
    assert np.isfinite(ap.threshold) and ap.threshold > 0 and ap.pass_samples > 0 and ap.min_samples >= 0
    assert (ap.threshold, ap.pass_samples, ap.min_samples) == (0.01, 64, 0)
    assert list(ap._reserved) == [0, 0, 0, 0]
    assert rt.adaptive_params(threshold=0.5, pass_samples=8).threshold == 0.5
    rt.lib().rt_adaptive_params_default(None)   # a NULL is ignored


def _call(rt, params=None, ap=None, out=True, default_ap=True):
    lib = rt.lib()
    cam = abi.RtCamera()
    params = params if params is not None else abi.render_params(64, 36, 96)
    if ap is None and default_ap:
        ap = rt.adaptive_params()
    rgb = (C.c_double * (64 * 36 * 3))() if out else None
    return lib.rt_render_adaptive(None, C.byref(cam), C.byref(params), C.byref(ap) if ap is not None else None,
                                  C.cast(rgb, C.POINTER(C.c_double)) if out else None, None, None,
                                  C.cast(None, abi.RtFrameCallback), None, C.cast(None, abi.RtCancelCallback), None)


def _ap(rt, **kw):
    ap = rt.adaptive_params()
    for k, v in kw.items():
        if k == "reserved":
            ap._reserved[v] = 1
        else:
            setattr(ap, k, v)
    return ap


@pytest.mark.parametrize("what,kw", [
    ("threshold", dict(threshold=float("nan"))), ("threshold", dict(threshold=float("inf"))),
    ("threshold", dict(threshold=-float("inf"))), ("pass_samples", dict(pass_samples=0)),
    ("pass_samples", dict(pass_samples=-4)), ("min_samples", dict(min_samples=-1)),
    ("_reserved", dict(reserved=0)), ("_reserved", dict(reserved=3))])
def test_bad_adaptive_parameters_are_refused_before_the_scene(rt, what, kw):
    assert _call(rt, ap=_ap(rt, **kw)) == abi.RT_ERR_INVALID_ARGUMENT
    msg = rt.lib().rt_last_error_message().decode()
    assert what in msg and "scene is NULL" not in msg, msg


def test_null_pointers_strips_and_scale_are_refused_before_the_scene(rt):
    assert _call(rt, ap=None, default_ap=False) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"adaptive is NULL" in rt.lib().rt_last_error_message()
    assert _call(rt, out=False) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"out_rgb is NULL" in rt.lib().rt_last_error_message()
    assert _call(rt, params=abi.render_params(64, 36, 96, strip_rows=8, strip_count=2, strip_index=0)) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"strip" in rt.lib().rt_last_error_message()
    assert _call(rt, params=abi.render_params(64, 36, 96, scale=2)) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"scale" in rt.lib().rt_last_error_message()
    # everything in order: the scene is what is missing
    assert _call(rt) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"scene is NULL" in rt.lib().rt_last_error_message()
    for thr in (0.0, -2.0):     # threshold <= 0 is allowed (no tile stops)
        assert _call(rt, ap=_ap(rt, threshold=thr)) == abi.RT_ERR_INVALID_ARGUMENT
        assert b"scene is NULL" in rt.lib().rt_last_error_message()


# ---- the CLI ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args,what", [
    (["--adaptive"], "missing value"), (["--adaptive", "abc"], "positive threshold"),
    (["--adaptive", "0"], "positive threshold"), (["--adaptive", "-0.5"], "positive threshold"),
    (["--adaptive", "nan"], "positive threshold"), (["--adaptive=0.01x"], "positive threshold"),
    (["--adaptive", "0.01", "--devices", "2"], "one device"), (["--devices", "2", "--adaptive", "0.01"], "one device")])
def test_cli_refuses_bad_adaptive_arguments_before_a_device(args, what):
    if not os.path.exists(CLI):
        pytest.fail("the CLI is not built (%s)" % CLI)
    run = subprocess.run([CLI, "-c", os.path.join(ROOT, "scenes", "config_c3.yml")] + args, capture_output=True, text=True,
                         timeout=60)
    assert run.returncode == abi.RT_ERR_ARGUMENT_PARSING, (run.returncode, run.stderr)
    assert what in run.stderr and "Rendering image" not in run.stderr, run.stderr
