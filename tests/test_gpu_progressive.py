"""rt_render_progressive on the device: passes of whole sample chunks folded into running per-pixel sums, one whole frame
per pass, the last equal bit for bit to rt_render_frame's (include/rt_abi.h; csrc/rt_progressive.hip)."""
import ctypes as C

import numpy as np
import pytest

import scenes_py as S
import variant_scenes as V
from test_gpu_fixed_point import into_the_light

pytestmark = pytest.mark.gpu
abi = S.abi
TOL = 1e-3          # the north star's per-channel tolerance (tests/test_gpu_parity.py)
TIGHT = 1e-9        # what f64 against f64 with the same draws achieves on the bulk


def _fresh_frame(rt, bundle, camera, params, **options):
    scene = rt.Scene(bundle, **options)
    try:
        return scene.render_frame(camera, params), scene.last_stats()
    finally:
        scene.close()


def _assert_last_is_one_shot(rt, bundle, camera, params, pass_list, **options):
    want, _ = _fresh_frame(rt, bundle, camera, params, **options)
    scene = rt.Scene(bundle, **options)
    try:
        for pass_samples in pass_list:
            frames = scene.render_progressive(camera, params, pass_samples)
            assert [d for d, _ in frames] == rt.progressive_passes(params.samples, pass_samples)
            assert np.array_equal(frames[-1][1], want), "pass_samples %d" % pass_samples
    finally:
        scene.close()


# ---- 1. the last frame is the one-shot frame ------------------------------------------------------------------------

@pytest.mark.parametrize("form", list(V.SPECS), ids=lambda f: "%s%s%s%s" % ("RSA"[f[0]], "t" if f[1] else "", "s" if f[2] else "",
                                                                              "-bvh" if f[3] else ""))
def test_last_frame_is_the_one_shot_frame_for_every_variant(rt, gpu, form):
    bundle, cam = V.build(form)
    closest_hit = abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR
    _assert_last_is_one_shot(rt, bundle, S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH),
                             (1, 30), closest_hit=closest_hit)


@pytest.mark.parametrize("form", [(V.ANY, 1, 1, 0), (V.ANY, 0, 1, 1)], ids=["Ats", "As-bvh"])
def test_last_frame_is_the_one_shot_frame_with_the_reference_arithmetic(rt, gpu, form):
    bundle, cam = V.build(form)
    closest_hit = abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR
    _assert_last_is_one_shot(rt, bundle, S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH),
                             (1, 30), closest_hit=closest_hit, arithmetic=abi.RT_ARITH_REFERENCE)


def test_last_frame_is_the_one_shot_frame_with_f64_sums(rt, gpu):
    bundle, cam = V.unbounded_scene()
    scene = rt.Scene(bundle)
    try:
        assert scene.variant()["exact"] == 1          # no radiance bound: f64 sums on the any-primitive path
    finally:
        scene.close()
    _assert_last_is_one_shot(rt, bundle, S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH), (1, 30))


def test_last_frame_is_the_one_shot_frame_with_the_tree_in_global_memory(rt, gpu):
    bundle, cam = V.large_bvh_scene()
    scene = rt.Scene(bundle)
    try:
        assert scene.variant()["bvh_nodes_in_lds"] == 0
    finally:
        scene.close()
    _assert_last_is_one_shot(rt, bundle, S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH), (1, 30))


def test_last_frame_is_the_one_shot_frame_of_cornell_box(rt, gpu):
    bundle, cam, _ = S.cornell_box()
    w, h = 320, 180
    _assert_last_is_one_shot(rt, bundle, S.camera_for(cam, w, h), abi.render_params(w, h, 1024), (256,))


# ---- 2. pass boundaries -----------------------------------------------------------------------------------------------

def test_pass_boundaries_and_totals(rt, gpu):
    bundle, cam, _ = S.three_balls()
    w, h = 64, 36
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, 96)
    want, _ = _fresh_frame(rt, bundle, camera, params)
    scene = rt.Scene(bundle)
    totals = []
    try:
        for pass_samples, done in ((1, [24, 48, 72, 84, 92, 96]), (30, [48, 84, 96]), (96, [96]), (97, [96]), (5000, [96])):
            cb_done = []

            def on_pass(_user, _rgb, samples_done, total):
                cb_done.append(samples_done)
                totals.append(total)

            cb = abi.RtFrameCallback(on_pass)
            rc = scene._lib.rt_render_progressive(scene._h, C.byref(camera), C.byref(params), pass_samples, cb, None,
                                                  C.cast(None, abi.RtCancelCallback), None)
            assert rc == abi.RT_OK
            assert cb_done == done
            if len(done) == 1:
                frames = scene.render_progressive(camera, params, pass_samples)
                assert len(frames) == 1 and frames[0][0] == 96 and np.array_equal(frames[0][1], want)
    finally:
        scene.close()
    assert set(totals) == {96}


# ---- 3. intermediate frames are s-spp frames ---------------------------------------------------------------------------

@pytest.mark.parametrize("scene_fn,use_bvh", [(S.cornell_box, 1), (S.three_balls, 1), (S.cornell_box_boxes, 0)])
def test_intermediate_frames_match_the_oracle_at_their_sample_count(rt, orc, gpu, scene_fn, use_bvh):
    bundle, cam, tm = scene_fn()
    w, h, n = 64, 36, 48                              # chunk boundaries 24, 36, 44, 48
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, n, seed=3)
    scene = rt.Scene(bundle)
    try:
        frames = scene.render_progressive(camera, params, 1)
    finally:
        scene.close()
    assert [d for d, _ in frames] == [24, 36, 44, 48]
    kind = {"None": orc.ORC_TM_NONE, "Aces": orc.ORC_TM_ACES}[tm]
    for done, got in frames:
        ref, _ = orc.render(bundle.desc, camera, abi.render_params(w, h, done, seed=3), use_bvh=use_bvh)
        assert np.isfinite(got).all()
        diff = np.abs(orc.tone_map(kind, ref) - orc.tone_map(kind, got))
        assert diff.max() < TOL, "%d spp: max |delta| = %g" % (done, diff.max())
        frac = float((diff.max(axis=-1) > TIGHT).mean())
        assert frac < 1e-3, "%d spp: fraction of pixels beyond %g: %g" % (done, TIGHT, frac)
    # the frames converge: each one differs from the last
    assert all(not np.array_equal(a, frames[-1][1]) for _, a in frames[:-1])


# ---- 4. stats describe the whole call ----------------------------------------------------------------------------------

def test_stats_describe_the_whole_call(rt, gpu):
    bundle, cam, _ = S.cornell_box()
    w, h, n = 160, 90, 256
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, n)
    _, one_shot = _fresh_frame(rt, bundle, camera, params)
    scene = rt.Scene(bundle)
    try:
        for pass_samples in (1, 64, n):
            frames = scene.render_progressive(camera, params, pass_samples)
            st = scene.last_stats()
            assert st.samples == w * h * n
            assert st.segments == one_shot.segments
            assert st.kernel_launches == len(frames)
            assert st.kernel_ms > 0.0 and st.resolve_ms > 0.0
    finally:
        scene.close()


# ---- 5. cancel ----------------------------------------------------------------------------------------------------------

def test_cancel_raised_on_entry(rt, gpu):
    bundle, cam, _ = S.cornell_box()
    w, h = 64, 36
    scene = rt.Scene(bundle)
    try:
        calls = []
        with pytest.raises(rt.RtError) as err:
            scene.render_progressive(S.camera_for(cam, w, h), abi.render_params(w, h, 96), 1, cancel=lambda: True,
                                     on_frame=lambda *a: calls.append(a))
        assert err.value.code == abi.RT_ERR_CANCEL_EVENT
        assert calls == []
    finally:
        scene.close()


def test_cancel_raised_in_the_first_callback_and_the_scene_afterwards(rt, gpu):
    bundle, cam, _ = S.cornell_box()
    w, h, n = 320, 180, 2048
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, n)
    small = abi.render_params(w, h, 96)
    want_frame, _ = _fresh_frame(rt, bundle, camera, small)
    fresh = rt.Scene(bundle)
    try:
        want_tiles = fresh.render_tiles(camera, small)
        want_passes = fresh.render_progressive(camera, small, 30)
    finally:
        fresh.close()
    scene = rt.Scene(bundle)
    try:
        raised = []
        frames = scene.render_progressive(camera, params, 64, cancel=lambda: bool(raised),
                                          on_frame=lambda done, _: raised.append(done))
        first = rt.progressive_passes(n, 64)[0]               # 128: the chunks of 2048 spp are 128 samples long
        assert [d for d, _ in frames] == [first] and raised == [first]
        assert scene.last_stats().samples < w * h * n          # the launch in flight was cut short
        # nothing stale: cancel word, item counters, slots
        assert np.array_equal(scene.render_frame(camera, small), want_frame)
        for got, want in zip(scene.render_tiles(camera, small), want_tiles):
            assert got[:4] == want[:4] and np.array_equal(got[4], want[4])
        for cancel in (None, lambda: False):
            again = scene.render_progressive(camera, small, 30, cancel=cancel)
            assert [d for d, _ in again] == [d for d, _ in want_passes]
            assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(again, want_passes))
        assert np.array_equal(again[-1][1], want_frame)
        st = scene.last_stats()
        assert st.samples == w * h * 96 and st.kernel_launches == len(again)
    finally:
        scene.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_scene_usable(rt, gpu):
    bundle, cam, _ = S.three_balls()
    w, h = 64, 36
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, 96)
    want, _ = _fresh_frame(rt, bundle, camera, params)
    scene = rt.Scene(bundle)
    try:
        def refused(code, p, pass_samples=1):
            with pytest.raises(rt.RtError) as err:
                scene.render_progressive(camera, p, pass_samples)
            assert err.value.code == code
            assert np.array_equal(scene.render_progressive(camera, params, 30)[-1][1], want)

        refused(abi.RT_ERR_INVALID_ARGUMENT, abi.render_params(w, h, 96, strip_rows=8, strip_count=2, strip_index=0))
        refused(abi.RT_ERR_INVALID_ARGUMENT, abi.render_params(w, h, 96, scale=2))
        refused(abi.RT_ERR_INVALID_ARGUMENT, params, pass_samples=0)
        refused(abi.RT_ERR_INVALID_ARGUMENT, params, pass_samples=-3)
        rc = scene._lib.rt_render_progressive(scene._h, C.byref(camera), C.byref(params), 1, C.cast(None, abi.RtFrameCallback),
                                              None, C.cast(None, abi.RtCancelCallback), None)
        assert rc == abi.RT_ERR_INVALID_ARGUMENT
        assert np.array_equal(scene.render_progressive(camera, params, 1)[-1][1], want)
    finally:
        scene.close()
    v1 = rt.Scene(bundle, kernel=abi.RT_KERNEL_V1)
    try:
        with pytest.raises(rt.RtError) as err:
            v1.render_progressive(camera, params, 1)
        assert err.value.code == abi.RT_ERR_UNSUPPORTED
        assert np.isfinite(v1.render_frame(camera, params)).all()
    finally:
        v1.close()


def test_a_render_refused_at_its_total_is_refused_here_too(rt, gpu):
    """Fixed-point sums take the exponent of the TOTAL sample count: what rt_render_frame refuses at N is refused before
    anything is enqueued, however small the passes."""
    w, h = 16, 16
    bundle, cam = into_the_light(2.0 ** 30 * (1 - 1e-15))
    camera = S.camera_for(cam, w, h)
    scene = rt.Scene(bundle)
    try:
        calls = []
        with pytest.raises(rt.RtError) as err:
            scene.render_progressive(camera, abi.render_params(w, h, 32769), 1, on_frame=lambda *a: calls.append(a))
        assert err.value.code == abi.RT_ERR_UNSUPPORTED and calls == []
        small = abi.render_params(w, h, 96)
        assert np.array_equal(scene.render_progressive(camera, small, 1)[-1][1], scene.render_frame(camera, small))
    finally:
        scene.close()
