"""The variance-guided filter of a still frame without a device: tests/variance_filter_model.py against
closed forms and against the models it is built from, and the C ABI of rt_batch_variance_device,
rt_denoise_variance_device and rt_render_adaptive_filtered — layouts, defaults and every refusal, none of which may touch a
device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_model as M
import temporal_model as T
import variance_filter_model as VF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
COUNTS = (24, 12, 8, 4)      # the chunks of a 48-spp frame: unequal n_j


def _flat_guides(h, w, albedo=(0.5, 0.25, 1.0), ids=1):
    """One object on one plane, seen head-on."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    n = np.zeros((h, w, 3))
    n[..., 2] = 1.0
    return {"normal": n, "position": np.stack([xs * 0.1, ys * 0.1, np.zeros((h, w))], axis=-1),
            "albedo": np.broadcast_to(np.array(albedo, dtype=float), (h, w, 3)).copy(),
            "footprint": np.full((h, w), 0.1), "obj_id": np.full((h, w), ids, dtype=np.int32)}


def _planes(h, w, s, k):
    return np.full((h, w), s, dtype=np.int32), np.full((h, w), k, dtype=np.int32)


# ---- the model against closed forms ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("demod", [1, 0], ids=["demod", "plain"])
def test_equal_chunk_means_of_a_constant_pixel_give_exactly_no_variance(demod):
    h, w = 4, 5
    g = _flat_guides(h, w)
    colour = np.broadcast_to(np.array([0.75, 0.5, 1.5]), (h, w, 3))      # dyadic: every product below is exact
    S, Q = VF.chunk_sums([colour] * len(COUNTS), COUNTS)
    samples, chunks = _planes(h, w, sum(COUNTS), len(COUNTS))
    Cr, var = VF.batch_variance(S, Q, samples, chunks, g, flags=demod, min_chunks=4)
    assert np.array_equal(var, np.zeros((h, w)))
    assert np.array_equal(Cr, colour / g["albedo"] if demod else colour)


def test_two_valued_chunks_with_unequal_counts_match_the_hand_sum():
    """Chunk means x1 over n1 samples and x2 over n2: Q - S m = n1 n2 (x1 - x2)^2 / s, so with k = 2
    sigma = sqrt(n1 n2) |x1 - x2| / s per channel, and var = (sum_c w_c sigma_c / a_c)^2."""
    h, w = 3, 4
    g = _flat_guides(h, w, albedo=(0.5, 1e-5, 1.0))      # the green albedo sits below the clamp: a = 1e-3
    n1, n2 = 24, 8
    x1, x2 = np.array([0.9, 0.2, 0.05]), np.array([0.3, 0.7, 0.0])
    S, Q = VF.chunk_sums([np.broadcast_to(x1, (h, w, 3)), np.broadcast_to(x2, (h, w, 3))], (n1, n2))
    samples, chunks = _planes(h, w, n1 + n2, 2)
    Cr, var = VF.batch_variance(S, Q, samples, chunks, g, min_chunks=2)
    a = np.array([0.5, 1e-3, 1.0])
    sig = np.sqrt(n1 * n2) * np.abs(x1 - x2) / (n1 + n2)
    want = float(np.dot(T.LUMA, sig / a)) ** 2
    assert np.all(np.abs(var - want) <= 1e-12 * want)
    assert np.all(np.abs(Cr - (x1 * n1 + x2 * n2) / (n1 + n2) / a) <= 1e-15 * np.abs(Cr))
    assert np.all(np.abs(VF.sigma(S, Q, samples, chunks) - sig) <= 1e-12 * np.maximum(sig, 1e-3))
    _, plain = VF.batch_variance(S, Q, samples, chunks, g, flags=0, min_chunks=2)
    assert np.all(np.abs(plain - float(np.dot(T.LUMA, sig)) ** 2) <= 1e-12 * plain)


@pytest.fixture(scope="module")
def synthetic():
    """denoise_model.synthetic_guides (24x32: misses, islands, albedo below the clamp) under batch sums whose chunk means
    scatter by about 30 %, and per-tile chunk counts on both sides of min_chunks = 4."""
    g, rng = M.synthetic_guides()
    h, w = g["obj_id"].shape
    base = M.synthetic_frame(g, rng) ** 2
    means = [base * rng.uniform(0.7, 1.3, base.shape) for _ in COUNTS]
    S_all, Q_all = [], []
    for k in range(1, len(COUNTS) + 1):
        S, Q = VF.chunk_sums(means[:k], COUNTS[:k])
        S_all.append(S)
        Q_all.append(Q)
    tiles = rng.integers(1, len(COUNTS) + 1, ((h + 7) // 8, (w + 7) // 8))
    chunks = np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)[:h, :w].astype(np.int32)
    samples = np.cumsum(COUNTS)[chunks - 1].astype(np.int32)
    pick = (chunks - 1)[..., None]
    S = np.choose(pick, S_all)
    Q = np.choose(pick, Q_all)
    assert (chunks >= 4).any() and (chunks < 4).any() and (g["obj_id"] < 0).any()
    return g, S, Q, samples, chunks


def test_a_guide_miss_has_no_variance(synthetic):
    g, S, Q, samples, chunks = synthetic
    miss = g["obj_id"] < 0
    for min_chunks in (2, 4, 9):
        Cr, var = VF.batch_variance(S, Q, samples, chunks, g, min_chunks=min_chunks)
        assert np.array_equal(var[miss], np.zeros(miss.sum()))
        assert np.array_equal(Cr[miss], (S / samples[..., None])[miss]), "a miss has albedo 1"
        assert np.all(np.isfinite(var)) and (var >= 0).all() and (var[~miss] > 0).any()


def test_a_tile_one_chunk_short_takes_the_spatial_estimate(synthetic):
    g, S, Q, _, _ = synthetic
    h, w = g["obj_id"].shape
    min_chunks = 4
    samples, chunks = _planes(h, w, sum(COUNTS[:3]), min_chunks - 1)
    Cr, var = VF.batch_variance(S, Q, samples, chunks, g, min_chunks=min_chunks)
    l = T.luminance(Cr)
    once = {"radiance": Cr, "moments": np.stack([l, l * l], axis=-1), "length": np.ones((h, w)), "normal": g["normal"],
            "position": g["position"], "obj_id": g["obj_id"]}
    assert np.array_equal(var, T.variance(once, g))
    # ... and one chunk more takes the batch estimate, which is another number
    _, batch = VF.batch_variance(S, Q, samples, chunks + 1, g, min_chunks=min_chunks)
    hit = g["obj_id"] >= 0
    assert not np.array_equal(batch[hit], var[hit])


def test_mixed_tiles_take_each_branch_where_it_applies(synthetic):
    g, S, Q, samples, chunks = synthetic
    _, var = VF.batch_variance(S, Q, samples, chunks, g, min_chunks=4)
    _, all_batch = VF.batch_variance(S, Q, samples, np.maximum(chunks, 4), g, min_chunks=4)
    _, all_spatial = VF.batch_variance(S, Q, samples, np.ones_like(chunks), g, min_chunks=4)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(var[chunks >= 4], all_batch[chunks >= 4])
    assert np.array_equal(var[chunks < 4], all_spatial[chunks < 4])


@pytest.mark.parametrize("sl", [0.0, -1.0])
@pytest.mark.parametrize("K", [0, 1, 5])
def test_without_the_luminance_stop_the_levels_are_the_denoisers(synthetic, K, sl):
    g, S, Q, samples, chunks = synthetic
    Cr, var = VF.batch_variance(S, Q, samples, chunks, g)
    got = VF.denoise_variance(Cr, var, g, iterations=K, sigma_luminance=sl)
    I = Cr
    for i in range(K):
        I = M.atrous(I, g, i, 0.0, 0.1, 1.0)
    assert np.array_equal(got, np.sqrt(np.maximum(I * g["albedo"], 0.0)))
    if K > 0:      # the whole of denoise_model.denoise on the gamma-encoded mean, up to the rounding of its own demodulation
        want = M.denoise(np.sqrt(S / samples[..., None]), g, iterations=K)
        assert np.all(np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want)))
        assert not np.array_equal(got, VF.denoise_variance(Cr, var, g, iterations=K, sigma_luminance=4.0))


def test_chunks_of_reads_the_chunk_plan():
    assert VF.chunks_of(np.array([[24, 48], [44, 36]]), [24, 36, 44, 48]).tolist() == [[1, 4], [3, 2]]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

STRUCTS = ("RtVarianceFilterParams", "RtBatchPlanes", "RtBatchOutputs")


def test_struct_layouts_match_the_c_compiler(abi):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', 'int main(void){']
    for s in STRUCTS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, name, s, name))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", INC, "-o", exe, src])
        want = dict(l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l)
    for s in STRUCTS:
        cls = getattr(abi, s)
        assert C.sizeof(cls) == int(want[s]), s
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == int(want["%s.%s" % (s, name)]), (s, name)


def test_the_defaults(rt, abi):
    fp = rt.variance_filter_params()
    assert (fp.sigma_luminance, fp.min_chunks, list(fp._reserved)) == (4.0, 4, [0] * 5)
    assert (fp.sigma_luminance, fp.min_chunks) == (VF.DEFAULTS["sigma_luminance"], VF.DEFAULTS["min_chunks"])
    rt.lib().rt_variance_filter_params_default(None)      # a NULL is ignored
    assert rt.variance_filter_params(min_chunks=2).min_chunks == 2


def _bad_filters(rt):
    reserved = rt.variance_filter_params()
    reserved._reserved[4] = 1
    return [(rt.variance_filter_params(sigma_luminance=float("nan")), b"sigma_luminance"),
            (rt.variance_filter_params(sigma_luminance=float("inf")), b"sigma_luminance"),
            (rt.variance_filter_params(min_chunks=1), b"min_chunks"), (reserved, b"_reserved")]


def test_every_refusal_comes_before_a_device_is_touched(rt, abi):
    """Every call below is refused with RT_ERR_INVALID_ARGUMENT and a message of its own; none of them reaches the scene
    (NULL here) or a device (this runs where there is none)."""
    lib = rt.lib()
    p, dp, fp = abi.render_params(16, 16, 48), rt.denoise_params(), rt.variance_filter_params()
    cam, ap, ls = abi.RtCamera(), rt.adaptive_params(), rt.light_sampling_params()
    one = C.c_void_p(8)      # any non-NULL address: nothing is read through it
    planes = abi.RtBatchPlanes(8, 8, 8, 8)
    guides = abi.RtGuides(8, 8, 8, 8, 8)
    out = (C.c_double * (16 * 16 * 3))()
    no_cb, never = C.cast(None, abi.RtFrameCallback), C.cast(None, abi.RtCancelCallback)

    def batch(p=p, dp=dp, fp=fp, planes=planes, guides=guides, rad=one, var=one):
        return lib.rt_batch_variance_device(None, C.byref(p) if p else None, C.byref(dp) if dp else None,
                                            C.byref(fp) if fp else None, C.byref(planes) if planes else None,
                                            C.byref(guides) if guides else None, rad, var, None)

    def levels(p=p, dp=dp, fp=fp, rad=one, var=one, guides=guides, dst=C.c_void_p(16)):
        return lib.rt_denoise_variance_device(None, C.byref(p) if p else None, C.byref(dp) if dp else None,
                                              C.byref(fp) if fp else None, rad, var, C.byref(guides) if guides else None, dst, None)

    def composed(p=p, ls=None, ap=ap, dp=dp, fp=fp, dst=out):
        return lib.rt_render_adaptive_filtered(None, C.byref(cam), C.byref(p) if p else None, C.byref(ls) if ls else None,
                                               C.byref(ap) if ap else None, C.byref(dp) if dp else None,
                                               C.byref(fp) if fp else None, dst, None, no_cb, None, never, None)

    def refused(rc, needle):
        assert rc == abi.RT_ERR_INVALID_ARGUMENT
        assert needle in lib.rt_last_error_message(), (needle, lib.rt_last_error_message())

    for call in (batch, levels, composed):
        for bad, needle in _bad_filters(rt):
            refused(call(fp=bad), needle)
        refused(call(fp=None), b"NULL")
        refused(call(dp=None), b"NULL")
        refused(call(p=None), b"NULL")
        refused(call(dp=rt.denoise_params(iterations=11)), b"iterations")
        refused(call(dp=rt.denoise_params(sigma_normal=float("nan"))), b"finite")
        refused(call(p=abi.render_params(16, 16, 48, strip_rows=8, strip_count=2)), b"strip")
        refused(call(p=abi.render_params(16, 16, 48, scale=2)), b"scale")
        refused(call(), b"scene is NULL")      # ... and with everything else in order, the scene is looked at last
    for k in range(4):
        half = abi.RtBatchPlanes(*[0 if i == k else 8 for i in range(4)])
        refused(batch(planes=half), b"batch_planes")
    refused(batch(planes=None), b"batch_planes")
    refused(batch(guides=None), b"guides_device")
    refused(batch(guides=abi.RtGuides(8, 8, 0, 8, 8)), b"guides_device")
    refused(batch(rad=None), b"NULL")
    refused(batch(var=None), b"NULL")
    refused(levels(rad=None), b"NULL")
    refused(levels(var=None), b"NULL")
    refused(levels(guides=None), b"guides_device")
    refused(levels(dst=None), b"out_device")
    refused(levels(dst=one), b"differ")
    refused(composed(dst=None), b"out_rgb")
    refused(composed(ap=None), b"adaptive is NULL")
    refused(composed(ap=rt.adaptive_params(pass_samples=0)), b"pass_samples")
    refused(composed(ap=rt.adaptive_params(threshold=float("nan"))), b"threshold")
    refused(composed(ls=rt.light_sampling_params(max_lights=65)), b"max_lights")
    refused(composed(ls=ls), b"NULL")
