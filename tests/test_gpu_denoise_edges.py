"""The denoiser on the device at its edges (csrc/rt_denoise.hip): the filter on caller-made guides
(denoise_model.synthetic_guides) at odd and partial-tile shapes and a frame large enough for the demodulation's
grid-stride loop to make a second trip, against the numpy model (itself held to tests/denoise_reference.py); properties
that need no model; the guides of every trace-kernel form against the oracle; the stream contract of rt_abi.h and the
reuse of the scene's scratch across sizes; the progressive form with non-default settings."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as M
import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
abi = S.abi
REL = 1e-11

# (width, height): none of them a multiple of the kernels' 16x16 tile on both sides but 96x80
SHAPES = [(2, 2), (2, 9), (9, 2), (17, 3), (37, 23), (131, 5), (96, 80)]
# 705 x 499 = 351 795 pixels: 3 W H > 4096 x 256 lanes, so demodulation and remodulation make a second grid-stride trip
BIG = (705, 499)
# a pairwise list: iterations 0, 1, 5 and 10; each of the three stops off at least once; demodulation on and off
SETTINGS = [dict(iterations=0, sigma_color=0.5),
            dict(iterations=1, flags=0, sigma_normal=0.0),
            dict(iterations=5, sigma_plane=0.0, sigma_color=1.0),
            dict(iterations=10, sigma_color=40.0),
            dict(iterations=5, flags=0),
            dict(iterations=10, flags=0, sigma_normal=0.0, sigma_plane=0.0, sigma_color=4.0)]
BIG_SETTINGS = [SETTINGS[0], SETTINGS[1], SETTINGS[2], SETTINGS[3]]


def _sid(kw):
    return ",".join("%s=%s" % i for i in kw.items())


def _frame(shape, seed=None):
    w, h = shape
    g, rng = M.synthetic_guides(h, w, seed=100 * w + h if seed is None else seed)
    return g, M.synthetic_frame(g, rng)


def _upload(guides, rgb, dev):
    import torch
    planes = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in guides.items()}
    return planes, torch.from_numpy(np.ascontiguousarray(rgb)).to(dev)


def _filter(rt, scene, shape, rgb, guides, dp):
    """rt_denoise_device on torch copies of rgb and guides (NaN in the output beforehand) -> numpy."""
    import torch
    dev = torch.device("cuda", scene.device)
    planes, src = _upload(guides, rgb, dev)
    out = torch.full_like(src, float("nan"))
    torch.cuda.synchronize(dev)
    scene.denoise_device(abi.render_params(shape[0], shape[1], 1), src.data_ptr(), rt.guides_struct(planes), out.data_ptr(), dp)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def host_scene(rt, gpu):
    """A scene only for its device and its scratch: rt_denoise_device reads nothing else of it."""
    scene = rt.Scene(S.three_balls()[0])
    yield scene
    scene.close()


def _check_against_model(rt, scene, shape, kw):
    g, rgb = _frame(shape)
    dp = rt.denoise_params(**kw)
    got = _filter(rt, scene, shape, rgb, g, dp)
    assert np.all(np.isfinite(got))
    want = M.denoise(rgb, g, **M.params_kwargs(dp))
    bad = M.mismatch(got, want, REL)
    assert bad == 0, "%d channels beyond %g of the model" % (bad, REL)
    miss = g["obj_id"] < 0
    assert miss.any() and np.array_equal(got[miss], rgb[miss]), "misses pass through"
    if kw["iterations"] == 0:
        assert np.array_equal(got, rgb)
    assert np.array_equal(_filter(rt, scene, shape, rgb, g, dp), got), "two calls differ"


@pytest.mark.parametrize("kw", SETTINGS, ids=_sid)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_filter_on_caller_guides_matches_the_model(rt, host_scene, shape, kw):
    _check_against_model(rt, host_scene, shape, kw)


@pytest.mark.parametrize("kw", BIG_SETTINGS, ids=_sid)
def test_the_filter_on_a_frame_past_one_grid_stride_matches_the_model(rt, host_scene, kw):
    _check_against_model(rt, host_scene, BIG, kw)


# ---- properties without the model ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [SETTINGS[3], SETTINGS[5], dict(iterations=5)], ids=_sid)
@pytest.mark.parametrize("shape", [(37, 23), (131, 5)], ids=lambda s: "%dx%d" % s)
def test_a_constant_demodulated_radiance_stays_constant(rt, host_scene, shape, kw):
    g, _ = _frame(shape)
    dp = rt.denoise_params(**kw)
    c = 0.37
    if dp.flags & abi.RT_DENOISE_DEMODULATE:   # the frame carries the clamped albedo, the output the albedo itself
        rgb, want = np.sqrt(c * np.maximum(g["albedo"], 1e-3)), np.sqrt(c * g["albedo"])
    else:
        rgb = want = np.full(g["albedo"].shape, np.sqrt(c))
    got = _filter(rt, host_scene, shape, rgb, g, dp)
    assert M.mismatch(got, want, 1e-12) == 0


@pytest.mark.parametrize("kw", [dict(iterations=5), SETTINGS[3], SETTINGS[5]], ids=_sid)
def test_scaling_one_object_leaves_the_others_bit_identical(rt, host_scene, kw):
    shape = (37, 23)
    g, rgb = _frame(shape)
    other = rgb.copy()
    other[g["obj_id"] == 2] *= 3.0
    dp = rt.denoise_params(**kw)
    a, b = _filter(rt, host_scene, shape, rgb, g, dp), _filter(rt, host_scene, shape, other, g, dp)
    keep = g["obj_id"] != 2
    assert np.array_equal(a[keep], b[keep])
    assert not np.array_equal(a[~keep], b[~keep])


@pytest.mark.parametrize("flags", [0, abi.RT_DENOISE_DEMODULATE])
def test_one_level_stays_inside_its_objects_input_range(rt, host_scene, flags):
    shape = (37, 23)
    g, rgb = _frame(shape)
    dp = rt.denoise_params(iterations=1, flags=flags, sigma_color=4.0)
    got = _filter(rt, host_scene, shape, rgb, g, dp)
    I = rgb * rgb
    a = np.ones_like(I)
    if flags:
        I, a = I / np.maximum(g["albedo"], 1e-3), g["albedo"]
    L = got * got    # = I_1 albedo (or I_1)
    for oid in np.unique(g["obj_id"][g["obj_id"] >= 0]):
        m = g["obj_id"] == oid
        lo, hi = I[m].min(axis=0), I[m].max(axis=0)
        assert np.all(L[m] >= lo * a[m] * (1 - 1e-12)) and np.all(L[m] <= hi * a[m] * (1 + 1e-12)), oid


# ---- guides on every trace-kernel form ----------------------------------------------------------------------------------

def _form_id(f):
    return "%s%s%s%s" % ("RSA"[f[0]], "t" if f[1] else "", "s" if f[2] else "", "-bvh" if f[3] else "")


def check_guides(got, want, what):
    """The planes of the device against the oracle's: obj_id on all but at most 1e-3 of the pixels, each mismatch on a
    silhouette; normal, position, albedo and footprint to 1e-9 where the ids agree; the miss values exact."""
    gid, wid = got["obj_id"], want["obj_id"]
    bad = np.argwhere(gid != wid)
    assert len(bad) <= 1e-3 * gid.size, "%s: obj_id differs on %d of %d pixels" % (what, len(bad), gid.size)
    h, w = gid.shape
    for y, x in bad:
        near = [wid[v, u] for v, u in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)) if 0 <= v < h and 0 <= u < w]
        assert gid[y, x] < 0 or wid[y, x] < 0 or gid[y, x] in near, "%s: obj_id %d/%d at (%d, %d) off a silhouette" % (
            what, gid[y, x], wid[y, x], y, x)
    same = gid == wid
    for plane in ("normal", "position", "albedo"):
        assert np.all(np.abs(got[plane][same] - want[plane][same]) < 1e-9), (what, plane)
    hit = same & (wid >= 0)
    assert np.all(np.abs(got["footprint"][hit] - want["footprint"][hit]) < 1e-9), what
    miss = same & (wid < 0)
    assert np.all(np.isinf(got["footprint"][miss])) and np.all(got["albedo"][miss] == 1.0), what
    assert np.all(got["normal"][miss] == 0.0) and np.all(got["position"][miss] == 0.0), what


@pytest.mark.parametrize("shape", [(61, 37), (2, 9)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("arith", [abi.RT_ARITH_FAST, abi.RT_ARITH_REFERENCE], ids=["fast", "reference"])
@pytest.mark.parametrize("form", list(V.SPECS), ids=_form_id)
def test_guides_of_every_form_match_the_oracle(rt, orc, gpu, form, arith, shape):
    bundle, cam = V.build(form)
    w, h = shape
    camera = S.camera_for(cam, w, h)
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR, arithmetic=arith)
    try:
        got = scene.render_guides(camera, abi.render_params(w, h, 1))
    finally:
        scene.close()
    want = M.oracle_guides(orc, bundle, camera, w, h)
    assert (want["obj_id"] >= 0).any() and (want["obj_id"] < 0).any()
    check_guides(got, want, _form_id(form))


def test_guides_after_a_frame_from_another_camera_match_the_oracle(rt, orc, gpu):
    """An LDS tree re-ordered for camera A (order_bvh_for_camera) still gives camera B's guides."""
    bundle, cam = V.build((V.ANY, 1, 1, 1))
    w, h = 61, 37
    cam_b = dict(cam, look_from=(4.5, 2.5, -3.5))
    a, b = S.camera_for(cam, w, h), S.camera_for(cam_b, w, h)
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH)
    try:
        assert scene.variant()["bvh_nodes_in_lds"] == 1
        scene.render_frame(a, abi.render_params(w, h, 4, max_depth=V.DEPTH))
        got = scene.render_guides(b, abi.render_params(w, h, 1))
    finally:
        scene.close()
    want = M.oracle_guides(orc, bundle, b, w, h)
    assert not np.array_equal(want["obj_id"], M.oracle_guides(orc, bundle, a, w, h)["obj_id"])
    check_guides(got, want, "camera B after A")


# ---- the stream contract and the scratch --------------------------------------------------------------------------------

def test_guides_and_filter_run_in_the_callers_stream_order(rt, gpu):
    """rt_abi.h: guides and filter are enqueued on hip_stream without synchronising.  Every buffer holds NaN; the caller's
    stream sleeps, then copies the frame in, then calls both: work on any other stream would read the NaN."""
    import torch
    bundle, cam = S.cornell_box_boxes()[:2]
    w, h = 96, 80
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, 16)
    dp = rt.denoise_params(iterations=5, sigma_color=1.0)
    scene = rt.Scene(bundle)
    try:
        rgb = scene.render_frame(camera, params)
        want_guides = scene.render_guides(camera, params)
        want = scene.denoise(camera, params, rgb, dp)
        dev = torch.device("cuda", scene.device)
        staged = torch.from_numpy(rgb).to(dev)
        nan = float("nan")
        src, out = torch.full_like(staged, nan), torch.full_like(staged, nan)
        planes = {k: torch.full((h, w, 3), nan, dtype=torch.float64, device=dev) for k in ("normal", "position", "albedo")}
        planes["footprint"] = torch.full((h, w), nan, dtype=torch.float64, device=dev)
        planes["obj_id"] = torch.full((h, w), -5, dtype=torch.int32, device=dev)
        g = rt.guides_struct(planes)
        torch.cuda.synchronize(dev)
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(300_000_000)
            src.copy_(staged, non_blocking=True)
            rc = scene._lib.rt_render_guides_device(scene._h, C.byref(camera), C.byref(params), C.byref(g),
                                                    C.c_void_p(stream.cuda_stream))
            scene.denoise_device(params, src.data_ptr(), g, out.data_ptr(), dp, stream=stream.cuda_stream)
        assert rc == abi.RT_OK
        stream.synchronize()
        got = out.cpu().numpy()
        got_guides = {k: v.cpu().numpy() for k, v in planes.items()}
    finally:
        scene.close()
    for k, v in want_guides.items():
        assert np.array_equal(got_guides[k], v), k
    assert np.array_equal(got, want)


def test_scratch_is_reused_across_sizes(rt, gpu):
    """One scene filters 705x499, then 37x23, then 705x499 again: each as on a fresh scene, bit for bit."""
    dp = rt.denoise_params(iterations=5, sigma_color=1.0)
    runs = [BIG, (37, 23), BIG]
    inputs = [_frame(s, seed=i) for i, s in enumerate(runs)]
    bundle = S.three_balls()[0]
    scene = rt.Scene(bundle)
    try:
        got = [_filter(rt, scene, s, rgb, g, dp) for s, (g, rgb) in zip(runs, inputs)]
    finally:
        scene.close()
    for s, (g, rgb), out in zip(runs, inputs, got):
        fresh = rt.Scene(bundle)
        try:
            assert np.array_equal(_filter(rt, fresh, s, rgb, g, dp), out), s
        finally:
            fresh.close()


# ---- progressive with non-default settings --------------------------------------------------------------------------

@pytest.mark.parametrize("form", [(V.SPHERES, 1, 1, 0), (V.ANY, 1, 0, 1)], ids=_form_id)
def test_progressive_denoised_with_non_default_settings_ends_on_the_one_shot_frame(rt, gpu, form):
    bundle, cam = V.build(form)
    camera, params = S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH)
    dp = rt.denoise_params(iterations=10, flags=0, sigma_color=0.75, sigma_normal=0.0)
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR)
    try:
        want = scene.denoise(camera, params, scene.render_frame(camera, params), dp)
        assert not np.array_equal(want, scene.denoise(camera, params, scene.render_frame(camera, params)))
        frames = scene.render_progressive(camera, params, 30, denoise=dp)
        assert [d for d, _ in frames] == rt.progressive_passes(params.samples, 30)
        assert np.array_equal(frames[-1][1], want)
    finally:
        scene.close()

