"""rt_render_progressive_nee and rt_render_adaptive_nee on the device (include/rt_abi.h).  The oracle of
every frame is rt_render_frame_nee — itself held to tests/nee_model.py by tests/test_gpu_nee.py — at the sample count the
frame (or the pixel) stands at: the passes carry each pixel's f64 sum from launch to launch in sample order, so the
comparison is np.array_equal throughout."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_model as M
import nee_model as NM
import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(abi, w, h, spp, depth=10, seed=1):
    p = abi.render_params(w, h, spp, max_depth=depth)
    p.seed = seed
    return p


def _scene(name, abi):
    if name.startswith("mixed"):
        return NM.mixed_scene(abi)
    bundle, cam, _ = getattr(S, name)()
    return bundle, cam


def _one_shot(scene, abi, c, w, h, spp, depth=10, seed=1, **kw):
    return scene.render_frame_nee(c, _params(abi, w, h, spp, depth, seed), **kw)


# ---- 1. every pass is the s-spp NEE frame ----------------------------------------------------------------------------

CASES_1 = [("cornell_box", 40, 24, 96, {}), ("cornell_box", 40, 24, 256, {}), ("mixed", 40, 24, 96, {}), ("mixed_bvh", 40, 24, 256, {}),
           ("mixed", 40, 24, 96, dict(max_lights=1)), ("cornell_box", 40, 24, 96, dict(heuristic=NM.BALANCE)),
           ("mixed", 40, 24, 96, dict(heuristic=NM.BALANCE)), ("cornell_box", 37, 29, 96, {}), ("cornell_box", 2, 2, 96, {}),
           ("mixed_exact", 40, 24, 96, {}), ("cornell_box_v1", 40, 24, 96, {})]


@pytest.mark.parametrize("name,w,h,n,kw", CASES_1, ids=["%s-%dx%d-%d-%s" % (c[0], c[1], c[2], c[3], "-".join(c[4]) or "default")
                                                        for c in CASES_1])
def test_every_pass_is_the_nee_frame_of_its_sample_count(rt, abi, gpu, name, w, h, n, kw):
    bundle, cam = _scene(name.replace("_v1", ""), abi)
    c = S.camera_for(cam, w, h)
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if name == "mixed_bvh" else abi.RT_HIT_LINEAR,
                     arithmetic=abi.RT_ARITH_REFERENCE if name == "mixed_exact" else abi.RT_ARITH_FAST,
                     kernel=abi.RT_KERNEL_V1 if name.endswith("_v1") else abi.RT_KERNEL_POOL)  # (v1 scenes are NOT refused)
    try:
        final = _one_shot(scene, abi, c, w, h, n, seed=7, **kw)
        st1 = scene.last_stats()
        for pass_samples in (1, 30, n):
            frames = scene.render_progressive_nee(c, _params(abi, w, h, n, seed=7), pass_samples, **kw)
            st = scene.last_stats()
            assert [d for d, _ in frames] == rt.progressive_passes(n, pass_samples)
            for done, frame in frames:
                assert np.array_equal(frame, _one_shot(scene, abi, c, w, h, done, seed=7, **kw)), (pass_samples, done)
            assert np.array_equal(frames[-1][1], final)
            assert st.segments == st1.segments and st.samples == w * h * n == st1.samples
            assert st.kernel_launches == len(frames) and st.kernel_ms > 0
    finally:
        scene.close()


def test_nothing_listed_is_the_plain_estimator_in_passes(rt, orc, abi, gpu):
    bundle, cam, _ = S.cornell_box()
    c = S.camera_for(cam, 16, 16)
    p = _params(abi, 16, 16, 8, 6, seed=3)
    scene = rt.Scene(bundle)
    try:
        frames = scene.render_progressive_nee(c, p, 4, max_lights=0)
    finally:
        scene.close()
    want, _ = orc.render(bundle.desc, c, p)
    d = np.abs(frames[-1][1] - want).max(axis=2)  # the parity tolerance of tests/test_gpu_parity.py
    assert float(d.max()) < 1e-3 and float(np.mean(d > 1e-9)) < 0.002


# ---- 2. every variant ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("form", sorted(V.SPECS), ids=lambda f: "p%d-t%d-s%d-b%d" % f)
def test_every_variant_ends_on_the_one_shot_frame(rt, abi, gpu, form, flavour):
    # (every form's scene lists a light, so the light-sampling branch runs in every instantiation of the pass kernel; with
    # `light2` it lists several, of every rect axis and of spheres as the class allows.  The one-shot frame itself is held
    # to the model in tests/test_gpu_nee.py)
    for light2 in (False, True):
        bundle, cam = V.build(form, light2=light2)
        c = S.camera_for(cam, V.W, V.H)
        p = abi.render_params(V.W, V.H, 48, max_depth=V.DEPTH)
        scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR,
                         arithmetic=abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST)
        try:
            v = scene.variant()
            assert (v["prims_class"], v["textured"], v["specular"], v["use_bvh"]) == form
            assert scene.lights() and (len(scene.lights()) > 1) == light2
            want = scene.render_frame_nee(c, p)
            frames = scene.render_progressive_nee(c, p, 10)
            assert len(frames) > 1 and np.array_equal(frames[-1][1], want)
        finally:
            scene.close()


# ---- 3. / 4. adaptive off, and a huge threshold ----------------------------------------------------------------------

@pytest.mark.parametrize("threshold", [0.0, -1.0])
def test_adaptive_off_is_the_one_shot_frame(rt, abi, gpu, threshold):
    bundle, cam, _ = S.cornell_box()
    w, h, n = 40, 24, 96
    c = S.camera_for(cam, w, h)
    scene = rt.Scene(bundle)
    try:
        frame, samples, err, frames = scene.render_adaptive_nee(c, _params(abi, w, h, n, seed=5), threshold=threshold, pass_samples=30)
        st = scene.last_stats()
        assert np.array_equal(frame, _one_shot(scene, abi, c, w, h, n, seed=5))
    finally:
        scene.close()
    assert np.all(samples == n) and st.samples == w * h * n
    assert [d for d, _ in frames] == rt.progressive_passes(n, 30)


def test_a_huge_threshold_stops_every_tile_at_the_first_eligible_boundary(rt, abi, gpu):
    bundle, cam, _ = S.cornell_box()
    w, h, n = 40, 24, 256
    c = S.camera_for(cam, w, h)
    bounds = rt.progressive_passes(n, 1)
    scene = rt.Scene(bundle)
    try:
        for pass_samples, min_samples in ((1, 0), (64, 0), (1, 100)):
            passes = rt.progressive_passes(n, pass_samples)
            first = next(b for b in passes if bounds.index(b) + 1 >= 4 and b >= min_samples)
            frame, samples, err, frames = scene.render_adaptive_nee(c, _params(abi, w, h, n, seed=5), threshold=1e9,
                                                                    pass_samples=pass_samples, min_samples=min_samples)
            assert np.all(samples == first), (pass_samples, min_samples, np.unique(samples), first)
            assert frames[-1][0] == first and scene.last_stats().samples == w * h * first
            assert np.array_equal(frame, _one_shot(scene, abi, c, w, h, first, seed=5))
            assert np.all(err >= 0.0)
    finally:
        scene.close()


# ---- 5. an intermediate threshold against the model ------------------------------------------------------------------

CASES_5 = [(64, 48, 1), (64, 48, 64), (37, 29, 1), (37, 29, 64)]


@pytest.mark.parametrize("w,h,pass_samples", CASES_5, ids=["%dx%d-p%d" % c for c in CASES_5])
def test_intermediate_threshold_matches_progressive_and_the_model(rt, abi, gpu, w, h, pass_samples):
    """Tolerances (set by the issue, from the model's own error): the model rebuilds S = f^2 b from a rounded frame, a
    relative error of a few ulp, which a constant pixel turns into a spurious sigma of about sqrt(8 eps) m and an e of about
    2e-8 sqrt(m): rtol 1e-6, atol 1e-7 (radiance <= 15), a tile being near when a model error at any of its passes lies
    within 1e-6 thr + 1e-7 of thr; near tiles < 10 %."""
    bundle, cam, _ = S.cornell_box()
    n = 256
    c, params = S.camera_for(cam, w, h), _params(abi, w, h, n, seed=9)
    scene = rt.Scene(bundle)
    try:
        prog_list = scene.render_progressive_nee(c, params, 1)
        prog = dict(prog_list)
        bounds = [d for d, _ in prog_list]
        passes = rt.progressive_passes(n, pass_samples)
        S_all, Q_all = M.sums_at_boundaries([f for _, f in prog_list], bounds)
        final = M.tile_errors(S_all[-1], Q_all[-1], n, len(bounds))
        thr = float(np.quantile(final, 0.5))  # the median of the tiles' final errors (fixed by the seed)
        assert thr > 0.0
        want_tiles, want_err, per_pass = M.simulate([f for _, f in prog_list], bounds, passes, thr, 0)
        frame, samples, err, frames = scene.render_adaptive_nee(c, params, threshold=thr, pass_samples=pass_samples)
        st = scene.last_stats()
    finally:
        scene.close()
    for b in np.unique(samples):  # every pixel equals the progressive NEE frame at its own count
        mask = samples == b
        assert np.array_equal(frame[mask], prog[int(b)][mask]), b
    tiles = samples[::8, ::8]
    assert np.array_equal(M.expand(tiles, h, w), samples)
    assert set(np.unique(samples)) <= set(passes)
    assert all(bounds.index(int(b)) + 1 >= 4 for b in np.unique(samples))
    near = np.zeros(tiles.shape, dtype=bool)
    for e in per_pass.values():
        near |= np.abs(e - thr) <= 1e-6 * thr + 1e-7
    print("%dx%d p%d: thr %.6g, near tiles %.3f, traced %.3f" % (w, h, pass_samples, thr, near.mean(), samples.mean() / n))
    assert near.mean() < 0.1
    ok = ~near
    assert np.array_equal(tiles[ok], want_tiles[ok])
    assert np.allclose(err[ok], want_err[ok], rtol=1e-6, atol=1e-7)
    assert tiles.min() < n and tiles.max() == n  # at this seed: some tile stops early, another runs to N
    assert st.samples == samples.sum() and st.kernel_launches == len(frames)
    # 6a. every callback's frame: running tiles at the pass boundary, stopped ones at their own
    assert [d for d, _ in frames] == passes[:len(frames)]
    for done, got in frames:
        at = np.minimum(samples, done)
        for b in np.unique(at):
            mask = at == b
            assert np.array_equal(got[mask], prog[int(b)][mask]), (done, b)
    assert np.array_equal(frames[-1][1], frame)


# ---- 6. cancel -------------------------------------------------------------------------------------------------------

def test_cancel_on_entry(rt, abi, gpu):
    bundle, cam, _ = S.cornell_box()
    c, p = S.camera_for(cam, 40, 24), _params(abi, 40, 24, 96)
    scene = rt.Scene(bundle)
    try:
        calls = []
        for render in (lambda: scene.render_progressive_nee(c, p, 8, cancel=lambda: True, on_frame=lambda *a: calls.append(a)),
                       lambda: scene.render_adaptive_nee(c, p, cancel=lambda: True, on_frame=lambda *a: calls.append(a))):
            with pytest.raises(rt.RtError) as err:
                render()
            assert err.value.code == abi.RT_ERR_CANCEL_EVENT and calls == []
    finally:
        scene.close()


@pytest.mark.parametrize("cancel_at", [1, 5])
def test_cancel_from_a_callback_keeps_the_last_delivered_state(rt, abi, gpu, cancel_at):
    bundle, cam, _ = S.cornell_box()
    w, h, n = 64, 48, 256
    c, p = S.camera_for(cam, w, h), _params(abi, w, h, n, seed=9)
    scene = rt.Scene(bundle)
    try:
        nee_before = scene.render_frame_nee(c, p)
        plain_before = scene.render_frame(c, p)
        # a threshold some tiles meet: the median of the tiles' errors after the whole frame
        _, _, err_n, _ = scene.render_adaptive_nee(c, p, threshold=0.0, pass_samples=1)
        thr = float(np.median(err_n[err_n > 0]))
        full = scene.render_adaptive_nee(c, p, threshold=thr, pass_samples=1)
        assert len(full[3]) > cancel_at
        seen = []
        frame, samples, err, frames = scene.render_adaptive_nee(c, p, threshold=thr, pass_samples=1, cancel=lambda: len(seen) >= cancel_at,
                                                                on_frame=lambda d, f: seen.append(d))
        assert len(frames) == cancel_at
        done = frames[-1][0]
        assert np.array_equal(frame, frames[-1][1]) and np.array_equal(frame, full[3][cancel_at - 1][1])
        assert np.array_equal(samples, np.minimum(full[1], done))
        # progressive form: the callbacks stop, the call returns RT_OK
        seen2 = []
        got = scene.render_progressive_nee(c, p, 1, cancel=lambda: len(seen2) >= cancel_at, on_frame=lambda d, f: seen2.append(d))
        assert len(got) == cancel_at
        # nothing stale afterwards
        assert np.array_equal(scene.render_frame_nee(c, p), nee_before)
        assert np.array_equal(scene.render_frame(c, p), plain_before)
        again = scene.render_adaptive_nee(c, p, threshold=thr, pass_samples=1)
        assert np.array_equal(again[0], full[0]) and np.array_equal(again[1], full[1])
    finally:
        scene.close()


# ---- 7. it is worth having -------------------------------------------------------------------------------------------

def test_noisy_tiles_stop_and_the_frame_stays_within_the_threshold_of_the_uniform_one(rt, abi, gpu):
    """Self-calibrating: thr = the median positive tile error after 256 samples, so at N = 1024 with passes of 64 (256 is then
    the first eligible boundary) about half the noisy tiles may stop at once.  Derived, not measured: a stopped tile's
    one-standard-error move of the gamma value is <= thr, hence rmse_adaptive <= rmse_uniform_N + thr."""
    bundle, cam, _ = S.cornell_box()
    w = h = 128
    c = S.camera_for(cam, w, h)
    scene = rt.Scene(bundle)
    try:
        _, _, err256, _ = scene.render_adaptive_nee(c, _params(abi, w, h, 256, seed=5), threshold=0.0)
        thr = float(np.median(err256[err256 > 0]))
        n = 1024
        assert 256 in rt.progressive_passes(n, 64)
        frame, samples, err, frames = scene.render_adaptive_nee(c, _params(abi, w, h, n, seed=5), threshold=thr, pass_samples=64)
        uniform = scene.render_frame_nee(c, _params(abi, w, h, n, seed=5))
        ref = scene.render_frame(c, _params(abi, w, h, 16384, seed=77))
    finally:
        scene.close()
    tiles = samples[::8, ::8]
    rmse = lambda f: float(np.sqrt(np.mean((f - ref) ** 2)))  # noqa: E731
    share = float(samples.sum()) / (w * h * n)
    print("cornell_box 128x128 N=1024: thr %.5f, traced %.1f %%, gamma RMSE adaptive %.5f, uniform %.5f"
          % (thr, 100 * share, rmse(frame), rmse(uniform)))
    assert np.any((tiles < n) & (err > 0.0))  # a NOISY tile stopped
    assert np.any(tiles == n)
    assert samples.sum() < w * h * n
    assert rmse(frame) <= rmse(uniform) + thr


# ---- 8. CLI ----------------------------------------------------------------------------------------------------------

def test_cli_nee_adaptive_writes_the_adaptive_nee_frame(rt, host, gpu):
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "cornell_box.yml")
    out = tempfile.mkdtemp(prefix="rt_cli_nee_adaptive_")
    r = subprocess.run([exe, "-c", config, "-s", scene_yml, "--image-action", "png", "--seed", "1", "--nee-adaptive", "0.01"],
                       capture_output=True, text=True, cwd=out, timeout=600)
    assert r.returncode == 0, r.stderr
    assert re.search(r"Adaptive sampling \(threshold 0\.01\) traced [0-9.]+ % of the \d+ samples per pixel", r.stderr), r.stderr
    m = re.search(r"Saved image to: (.+)", r.stderr)
    assert m, r.stderr
    path = m.group(1).strip()
    path = path if os.path.isabs(path) else os.path.join(out, path)
    session = host.Session(config, scene=scene_yml, image_action="png", seed=1)
    scene = rt.Scene(session)
    try:
        frame = scene.render_adaptive_nee(session.camera, session.params, threshold=0.01)[0]
        want = host.pack_rgba8(session.tone_map(frame))
    finally:
        scene.close()
        session.close()
    assert np.array_equal(host.decode_image(path), want)
    for bad in (["--nee-adaptive", "0.01", "--adaptive", "0.01"], ["--nee-adaptive", "0.01", "--devices", "2"], ["--nee-adaptive", "0"]):
        r = subprocess.run([exe, "-c", config, "-s", scene_yml] + bad, capture_output=True, text=True, cwd=out, timeout=60)
        assert r.returncode != 0 and "--nee-adaptive" in r.stderr, (bad, r.stderr)
