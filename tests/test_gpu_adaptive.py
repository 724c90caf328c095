"""rt_render_adaptive on the device: rt_render_progressive's passes with converged 8x8 tiles left out after they stop
(include/rt_abi.h; csrc/rt_progressive.hip, k_fold_adaptive_f64).  Every pixel is held bit for bit to the progressive frame
at its own sample count, and the stop points and tile errors to the numpy model of tests/adaptive_model.py."""
import numpy as np
import pytest

import adaptive_model as M
import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
abi = S.abi


def _one_shot(rt, bundle, camera, params, **options):
    scene = rt.Scene(bundle, **options)
    try:
        return scene.render_frame(camera, params), scene.last_stats()
    finally:
        scene.close()


def _assert_threshold_off_is_one_shot(rt, bundle, camera, params, **options):
    want, st_want = _one_shot(rt, bundle, camera, params, **options)
    scene = rt.Scene(bundle, **options)
    try:
        for thr, pass_samples in ((0.0, 30), (-1.0, 1)):
            frame, samples, err, frames = scene.render_adaptive(camera, params, threshold=thr, pass_samples=pass_samples)
            st = scene.last_stats()
            assert np.array_equal(frame, want), (thr, pass_samples)
            assert (samples == params.samples).all()
            assert [d for d, _ in frames] == rt.progressive_passes(params.samples, pass_samples)
            assert np.array_equal(frames[-1][1], frame)
            assert st.samples == st_want.samples == samples.sum() and st.segments == st_want.segments
            assert st.kernel_launches == len(frames)
            assert err.shape == ((params.height + 7) // 8, (params.width + 7) // 8) and (err >= 0).all()
    finally:
        scene.close()


# ---- 1. threshold <= 0 is rt_render_frame -----------------------------------------------------------------------------

@pytest.mark.parametrize("form", list(V.SPECS), ids=lambda f: "%s%s%s%s" % ("RSA"[f[0]], "t" if f[1] else "", "s" if f[2] else "",
                                                                              "-bvh" if f[3] else ""))
def test_threshold_off_is_the_one_shot_frame_for_every_variant(rt, gpu, form):
    bundle, cam = V.build(form)
    closest_hit = abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR
    _assert_threshold_off_is_one_shot(rt, bundle, S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH),
                                      closest_hit=closest_hit)


def test_threshold_off_with_the_reference_arithmetic(rt, gpu):
    bundle, cam = V.build((V.ANY, 1, 1, 0))
    _assert_threshold_off_is_one_shot(rt, bundle, S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH),
                                      closest_hit=abi.RT_HIT_LINEAR, arithmetic=abi.RT_ARITH_REFERENCE)


def test_threshold_off_with_f64_sums_and_the_tree_in_global_memory(rt, gpu):
    for make, key, want in ((V.unbounded_scene, "exact", 1), (V.large_bvh_scene, "bvh_nodes_in_lds", 0)):
        bundle, cam = make()
        scene = rt.Scene(bundle)
        try:
            assert scene.variant()[key] == want
        finally:
            scene.close()
        _assert_threshold_off_is_one_shot(rt, bundle, S.camera_for(cam, V.W, V.H),
                                          abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH))


# ---- 2. a huge threshold stops every tile at the first eligible boundary ---------------------------------------------

def test_a_huge_threshold_stops_every_tile_at_the_first_eligible_boundary(rt, gpu):
    bundle, cam, _ = S.three_balls()
    w, h, n = 64, 40, 256
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, n, seed=5)
    scene = rt.Scene(bundle)
    try:
        prog = dict(scene.render_progressive(camera, params, 1))
        bounds = sorted(prog)
        for pass_samples, min_samples in ((1, 0), (1, 100), (64, 0)):
            passes = rt.progressive_passes(n, pass_samples)
            first = next(b for b in passes if bounds.index(b) + 1 >= 4 and b >= min_samples)
            frame, samples, err, frames = scene.render_adaptive(camera, params, threshold=1e9, pass_samples=pass_samples,
                                                                min_samples=min_samples)
            st = scene.last_stats()
            assert (samples == first).all(), (pass_samples, min_samples, first, np.unique(samples))
            assert np.array_equal(frame, prog[first])
            assert [d for d, _ in frames] == passes[:passes.index(first) + 1]
            assert st.kernel_launches == len(frames) < len(passes)
            assert st.samples == samples.sum() == w * h * first
            assert (err >= 0).all()
    finally:
        scene.close()


# ---- 3. an intermediate threshold: every pixel is the progressive frame at its own count ------------------------------

CASES = [(S.three_balls, 64, 48, 1), (S.three_balls, 37, 29, 64), (S.three_balls, 2, 2, 1),
         (S.cornell_box_boxes, 64, 48, 64), (S.cornell_box_boxes, 37, 29, 1)]


@pytest.mark.parametrize("scene_fn,w,h,pass_samples", CASES,
                         ids=["%s-%dx%d-p%d" % (c[0].__name__, c[1], c[2], c[3]) for c in CASES])
def test_intermediate_threshold_matches_progressive_and_the_model(rt, gpu, scene_fn, w, h, pass_samples):
    bundle, cam, _ = scene_fn()
    n = 256
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, n, seed=9)
    scene = rt.Scene(bundle)
    try:
        prog_list = scene.render_progressive(camera, params, 1)
        prog = dict(prog_list)
        bounds = [d for d, _ in prog_list]
        passes = rt.progressive_passes(n, pass_samples)
        # the threshold: the 30th percentile of the tiles' errors over all chunks (fixed by the seed)
        S_all, Q_all = M.sums_at_boundaries([f for _, f in prog_list], bounds)
        final = M.tile_errors(S_all[-1], Q_all[-1], n, len(bounds))
        thr = float(np.quantile(final, 0.3)) if final.size > 1 else float(final.max()) * 1.5 + 1e-6
        want_tiles, want_err, per_pass = M.simulate([f for _, f in prog_list], bounds, passes, thr, 0)
        frame, samples, err, frames = scene.render_adaptive(camera, params, threshold=thr, pass_samples=pass_samples)
        st = scene.last_stats()
    finally:
        scene.close()
    # every pixel equals the progressive frame at its own count
    for b in np.unique(samples):
        mask = samples == b
        assert np.array_equal(frame[mask], prog[int(b)][mask]), b
    # counts: tile-constant, pass boundaries, eligible (>= 4 chunks) unless N
    tiles = samples[::8, ::8]
    assert np.array_equal(M.expand(tiles, h, w), samples)
    assert set(np.unique(samples)) <= set(passes)
    assert all(bounds.index(int(b)) + 1 >= 4 for b in np.unique(samples))
    # the stop points and the device's tile errors agree with the model, away from the threshold
    near = np.zeros(tiles.shape, dtype=bool)
    for e in per_pass.values():
        near |= np.abs(e - thr) <= 1e-6 * max(thr, 1e-300)
    assert near.mean() < 0.1
    ok = ~near
    assert np.array_equal(tiles[ok], want_tiles[ok])
    assert np.allclose(err[ok], want_err[ok], rtol=1e-6, atol=1e-12)
    if tiles.size > 1:                                   # at this seed: some tile stops early, another runs to N
        assert tiles.min() < n and tiles.max() == n
    assert st.samples == samples.sum()
    assert st.kernel_launches == len(frames)
    # every callback's frame: running tiles at the pass boundary, stopped ones at their own
    assert [d for d, _ in frames] == passes[:len(frames)]
    for done, got in frames:
        at = np.minimum(samples, done)
        for b in np.unique(at):
            mask = at == b
            assert np.array_equal(got[mask], prog[int(b)][mask]), (done, b)
    assert np.array_equal(frames[-1][1], frame)


# ---- 4. cancel and refusals -------------------------------------------------------------------------------------------

def test_cancel_on_entry_and_v1(rt, gpu):
    bundle, cam, _ = S.cornell_box()
    w, h = 64, 36
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, 96)
    scene = rt.Scene(bundle)
    try:
        calls = []
        with pytest.raises(rt.RtError) as err:
            scene.render_adaptive(camera, params, cancel=lambda: True, on_frame=lambda *a: calls.append(a))
        assert err.value.code == abi.RT_ERR_CANCEL_EVENT and calls == []
    finally:
        scene.close()
    v1 = rt.Scene(bundle, kernel=abi.RT_KERNEL_V1)
    try:
        with pytest.raises(rt.RtError) as err:
            v1.render_adaptive(camera, params)
        assert err.value.code == abi.RT_ERR_UNSUPPORTED
    finally:
        v1.close()


@pytest.mark.parametrize("cancel_at", [1, 5])
def test_cancel_from_a_callback_keeps_the_last_delivered_state(rt, gpu, cancel_at):
    bundle, cam, _ = S.three_balls()
    w, h, n = 160, 96, 1024
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, n, seed=2)
    small = abi.render_params(w, h, 96)
    want_small, _ = _one_shot(rt, bundle, camera, small)
    scene = rt.Scene(bundle)
    try:
        full, full_samples, full_err, full_frames = scene.render_adaptive(camera, params, threshold=0.02, pass_samples=64)
        seen = []
        frame, samples, err, frames = scene.render_adaptive(camera, params, threshold=0.02, pass_samples=64,
                                                            cancel=lambda: len(seen) >= cancel_at,
                                                            on_frame=lambda d, _: seen.append(d))
        assert len(frames) == cancel_at
        done = frames[-1][0]
        assert np.array_equal(frame, frames[-1][1])
        assert np.array_equal(frame, full_frames[cancel_at - 1][1])
        assert np.array_equal(samples, np.minimum(full_samples, done))
        stopped = full_samples[::8, ::8] <= done
        assert np.array_equal(err[stopped], full_err[stopped])
        # nothing stale afterwards
        assert np.array_equal(scene.render_frame(camera, small), want_small)
        again = scene.render_adaptive(camera, small, threshold=0.0, pass_samples=30)
        assert np.array_equal(again[0], want_small) and (again[1] == 96).all()
    finally:
        scene.close()
