"""rt_scene_set_lights on the MI355X: the extended-light kernels equal to tests/nee_lights_model.py in every form and both
flavours, one estimator through every NEE entry point, strictly opt-in, worth its shadow rays on a wrapped light, and
reachable from the CLI."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import nee_lights_model as LM
import nee_lights_scenes as LS
import nee_model as NM
import nee_variant_frames as F
import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY_FORMS = [f for f in V.SPECS if f[0] == V.ANY]
PLAIN_FORMS = [f for f in V.SPECS if f[0] != V.ANY]
_form_id = lambda f: "%s%s%s%s" % ("RSA"[f[0]], "t" * f[1], "s" * f[2], "-bvh" * f[3])  # noqa: E731

# (pick, heuristic, max_lights, max_depth) of a form's renders; the last one: the cap, and only the first vertex samples
RENDERS = ((LM.UNIFORM, NM.POWER, NM.MAX_LIGHTS, V.DEPTH), (LM.UNIFORM, NM.BALANCE, NM.MAX_LIGHTS, V.DEPTH),
           (LM.POWER_PICK, NM.POWER, NM.MAX_LIGHTS, V.DEPTH), (LM.POWER_PICK, NM.BALANCE, NM.MAX_LIGHTS, V.DEPTH),
           (LM.POWER_PICK, NM.POWER, 1, 2))

_MODEL_FRAMES = {}   # (form, kinds, pick, heuristic, max_lights, depth) -> (frame, segments): one model render per session


def _case(form):
    bundle, cam = LS.variant_case(form) if form[0] == V.ANY else V.build(form, light2=True)
    return bundle, S.camera_for(cam, F.W, F.H)


def _model_frame(orc, form, kinds, pick, heuristic, max_lights, depth):
    key = (form, kinds, pick, heuristic, max_lights, depth)
    if key not in _MODEL_FRAMES:
        bundle, camera = _case(form)
        model = LM.Model(orc, bundle.desc, kinds, pick)
        try:
            _MODEL_FRAMES[key] = model.render(camera, F.params(S.abi, depth), max_lights=max_lights, heuristic=heuristic)
        finally:
            model.close()
        _MODEL_FRAMES[key][0].setflags(write=False)
    return _MODEL_FRAMES[key]


def _parity(got, want):
    """The parity tolerance of tests/test_gpu_nee.py: max < 1e-3, fewer than 0.2 % of the pixels beyond 1e-9."""
    d = np.abs(got - want).max(axis=2)
    assert float(d.max()) < 1e-3, float(d.max())
    assert float(np.mean(d > 1e-9)) < 0.002, float(np.mean(d > 1e-9))


def _scene(rt, abi, bundle, form, flavour="fast"):
    return rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR,
                    arithmetic=abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST)


# ---- 1. against the model --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("form", ANY_FORMS, ids=_form_id)
def test_every_extended_form_matches_the_model(rt, orc, abi, gpu, form, flavour):
    """The form's light2 scene plus a box light, a wrapped rect, a wrapped sphere and (where the form has one) a moving
    light still selects its form; with RT_LIGHTS_ALL the library lists the model's lights and k_nee_lights_f64 renders
    the model's frame under both picks and both heuristics, and with the list capped at one light at max_depth 2."""
    bundle, camera = _case(form)
    scene = _scene(rt, abi, bundle, form, flavour)
    got = []
    try:
        variant = scene.variant()
        before = scene.lights()
        for pick, heuristic, max_lights, depth in RENDERS:
            scene.set_lights(abi.RT_LIGHTS_ALL, pick)
            lights, weights = scene.lights(), scene.light_weights()
            frame = scene.render_frame_nee(camera, F.params(abi, depth), max_lights=max_lights, heuristic=heuristic)
            got.append((frame, int(scene.last_stats().segments), lights, weights))
    finally:
        scene.close()
    want = dict(prims_class=V.ANY, textured=form[1], specular=form[2], use_bvh=form[3], exact=int(flavour == "exact"))
    assert {k: variant[k] for k in want} == want
    assert before == NM.light_list(bundle.desc) and len(before) == F.N_LIGHTS[V.ANY]
    for (pick, heuristic, max_lights, depth), (frame, segments, lights, weights) in zip(RENDERS, got):
        assert lights == LM.light_list(bundle.desc, LM.ALL) and len(lights) == F.N_LIGHTS[V.ANY] + LS.n_extended(form)
        assert weights == LM.pick_table(bundle.desc, lights, len(lights), pick)[0]
        ref, ref_segments = _model_frame(orc, form, LM.ALL, pick, heuristic, max_lights, depth)
        d = np.abs(frame - ref)
        print("%s %s pick %d heuristic %d max_lights %d depth %d: max |delta| = %.3g, share beyond 1e-9 = %.3g, segments %d (model %d)"
              % (form, flavour, pick, heuristic, max_lights, depth, d.max(), float((d.max(axis=2) > 1e-9).mean()), segments, ref_segments))
    for r, (frame, segments, _, _) in zip(RENDERS, got):
        ref, ref_segments = _model_frame(orc, form, LM.ALL, *r)
        assert np.isfinite(frame).all()
        _parity(frame, ref)
        assert frame.std() > 0.05   # a picture, not a flat background
        assert abs(segments - ref_segments) <= 4, (segments, ref_segments)


@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("form", PLAIN_FORMS, ids=_form_id)
def test_a_pick_by_power_on_the_rects_and_spheres_forms(rt, orc, abi, gpu, form, flavour):
    """A rects-only or spheres-only scene that asks for RT_PICK_POWER keeps its class and its list and is rendered by the
    PRIMS_ANY form of the extended kernels: the model's frame."""
    bundle, camera = _case(form)
    scene = _scene(rt, abi, bundle, form, flavour)
    try:
        assert scene.variant()["prims_class"] == form[0]
        scene.set_lights(abi.RT_LIGHTS_PLAIN, abi.RT_PICK_POWER)
        lights, weights = scene.lights(), scene.light_weights()
        frame = scene.render_frame_nee(camera, F.params(abi, V.DEPTH))
        segments = int(scene.last_stats().segments)
    finally:
        scene.close()
    assert lights == NM.light_list(bundle.desc) and weights == LM.pick_table(bundle.desc, lights, len(lights), LM.POWER_PICK)[0]
    ref, ref_segments = _model_frame(orc, form, LM.PLAIN, LM.POWER_PICK, NM.POWER, NM.MAX_LIGHTS, V.DEPTH)
    d = np.abs(frame - ref)
    print("%s %s: max |delta| = %.3g, share beyond 1e-9 = %.3g, segments %d (model %d)"
          % (form, flavour, d.max(), float((d.max(axis=2) > 1e-9).mean()), segments, ref_segments))
    _parity(frame, ref)
    assert abs(segments - ref_segments) <= 4, (segments, ref_segments)


# ---- 2. one estimator, every road ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [(V.ANY, 0, 1, 0), (V.ANY, 1, 0, 1)], ids=_form_id)
def test_every_entry_point_renders_the_one_shot_frame(rt, abi, gpu, form):
    """After rt_scene_set_lights(ALL, POWER): the passes of rt_render_progressive_nee, rt_render_adaptive_nee, the tiles of
    rt_render_nee, rt_render_frame_nee_strips_device at strip height 3 and the three several-scene calls (two scenes on one
    card) equal rt_render_frame_nee at their sample counts, bit for bit."""
    import torch
    bundle, _ = _case(form)
    _, cam = LS.variant_case(form)
    w, h, n = 40, 27, 96
    c = S.camera_for(cam, w, h)
    p = abi.render_params(w, h, n, max_depth=8)
    p.seed = 13
    p.tiles_w, p.tiles_h = 4, 3
    scenes = [_scene(rt, abi, bundle, form) for _ in range(2)]
    try:
        for s in scenes:
            s.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_POWER)
        scene = scenes[0]
        want = scene.render_frame_nee(c, p)
        assert want.std() > 0.05

        def at(samples):
            q = abi.render_params(w, h, samples, max_depth=8)
            q.seed = 13
            return scene.render_frame_nee(c, q)
        frames = scene.render_progressive_nee(c, p, 24)
        assert len(frames) >= 2 and frames[-1][0] == n
        for done, frame in frames:
            assert np.array_equal(frame, at(done)), done
        frame, samples, _, _ = scene.render_adaptive_nee(c, p, threshold=1e-9, pass_samples=24)
        for count in np.unique(samples):   # every pixel is the one-shot frame's at its own sample count
            mask = samples == count
            assert np.array_equal(frame[mask], at(int(count))[mask]), count
        assert int(samples.max()) == n
        tiles, order = scene.render_tiles_nee(c, p)
        assert len(order) == 12 and np.array_equal(tiles, want)
        dev = torch.device("cuda", 0)
        out = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        for index in range(2):
            q = abi.render_params(w, h, n, max_depth=8, strip_rows=3, strip_count=2, strip_index=index)
            q.seed = 13
            scene.render_frame_nee_strips_device(c, q, out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(rt.render_frame_nee_multi(scenes, c, p, strip_rows=3), want)
        out.zero_()
        rt.render_frame_nee_multi_device(scenes, c, p, out.data_ptr(), strip_rows=5)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        tiles, order = rt.render_tiles_nee_multi(scenes, c, p, strip_rows=8)
        assert len(order) == 12 and np.array_equal(tiles, want)
        # scenes that do not carry the same list params are refused
        scenes[1].set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_UNIFORM)
        for call in (lambda: rt.render_frame_nee_multi(scenes, c, p), lambda: rt.render_frame_nee_multi_device(scenes, c, p, out.data_ptr()),
                     lambda: rt.render_tiles_nee_multi(scenes, c, p)):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT and "light list" in str(e.value)
    finally:
        for s in scenes:
            s.close()


def test_a_cancel_leaves_nothing_stale(rt, abi, gpu):
    """The wrapper twin with its light listed, 640x360 in a 10x10 tile grid: the hook rises inside the first tile's callback;
    every tile that arrived is the one-shot frame's, and the scene then renders as a fresh one."""
    bundle, cam = LS.cornell_twin()
    w, h, n = 640, 360, 128
    scene, fresh = rt.Scene(bundle), rt.Scene(bundle)
    try:
        for s in (scene, fresh):
            s.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_POWER)
        c = S.camera_for(cam, w, h)
        p = abi.render_params(w, h, n, max_depth=10)
        want = fresh.render_frame_nee(c, p)
        raised = []
        frame, order = scene.render_tiles_nee(c, p, cancel=lambda: bool(raised), on_tile=lambda *t: raised.append(t))
        assert 1 <= len(order) <= 100
        for r, col, tw, th in order:
            assert np.array_equal(frame[r:r + th, col:col + tw], want[r:r + th, col:col + tw])
        small = abi.render_params(160, 90, 24, max_depth=10, seed=9)
        cs = S.camera_for(cam, 160, 90)
        for render in (lambda s: s.render_tiles_nee(cs, small)[0], lambda s: s.render_frame_nee(cs, small),
                       lambda s: s.render_progressive_nee(cs, small, 8)[-1][1]):
            assert np.array_equal(render(scene), render(fresh))
    finally:
        scene.close()
        fresh.close()


# ---- 3. opt-in -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hit", ["linear", "bvh"])
def test_until_it_is_called_and_after_the_defaults_a_scene_is_a_fresh_one(rt, abi, gpu, hit):
    bundle, cam = LS.all_kinds_scene()
    mixed, mixed_cam = NM.mixed_scene(abi)
    for b, cm, plain_list, all_list in ((bundle, cam, [], [2, 3, 4, 5]), (mixed, mixed_cam, [2, 3, 8], [2, 3, 4, 8])):
        c = S.camera_for(cm, 32, 20)
        p = abi.render_params(32, 20, 8, max_depth=8, seed=3)
        kw = dict(closest_hit=abi.RT_HIT_BVH if hit == "bvh" else abi.RT_HIT_LINEAR)
        fresh, scene = rt.Scene(b, **kw), rt.Scene(b, **kw)
        try:
            want = (fresh.lights(), fresh.light_weights(), fresh.render_frame_nee(c, p), fresh.render_frame(c, p))
            assert want[0] == plain_list == NM.light_list(b.desc)
            assert want[1] == [1.0 / max(1, len(plain_list))] * len(plain_list)
            state = lambda s: (s.lights(), s.light_weights(), s.render_frame_nee(c, p), s.render_frame(c, p))  # noqa: E731

            def same(a):
                return a[0] == want[0] and a[1] == want[1] and np.array_equal(a[2], want[2]) and np.array_equal(a[3], want[3])
            assert same(state(scene))
            scene.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_POWER)
            assert scene.lights() == all_list == LM.light_list(b.desc, LM.ALL)
            weights = scene.light_weights()
            assert weights == LM.pick_table(b.desc, all_list, len(all_list), LM.POWER_PICK)[0] and abs(sum(weights) - 1.0) < 1e-12
            extended = scene.render_frame_nee(c, p)
            assert not np.array_equal(extended, want[2])
            assert np.array_equal(scene.render_frame(c, p), want[3])   # the plain frame never moves
            scene.set_lights()                                         # the defaults: today's list, exactly
            assert same(state(scene))
            scene.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_POWER)     # ... and any number of times
            assert np.array_equal(scene.render_frame_nee(c, p), extended)
        finally:
            fresh.close()
            scene.close()


# ---- 4. it pays ----------------------------------------------------------------------------------------------------------------

def test_a_listed_wrapped_light_is_worth_the_original(rt, abi, gpu):
    """128x128 at 64 spp against a 4096-spp plain frame at another seed, as tests/test_gpu_nee.py measures cornell_box: the
    wrapper twin with RT_LIGHTS_ALL has at most 1.25 x the RMSE of the unwrapped original with today's list (the two take
    the same samples up to rounding; 1.25 leaves room for the RMSE estimate over 16 384 pixels), and the twin with the
    default list — its light unlisted — is noisier than with ALL."""
    original, cam, _ = S.cornell_box()
    twin, _ = LS.cornell_twin()
    c = S.camera_for(cam, 128, 128)

    def params(spp, seed):
        p = abi.render_params(128, 128, spp, max_depth=10)
        p.seed = seed
        return p
    a, b = rt.Scene(original), rt.Scene(twin)
    try:
        ref = a.render_frame(c, params(4096, 77))
        nee_original = a.render_frame_nee(c, params(64, 5))
        assert b.lights() == []
        nee_twin_default = b.render_frame_nee(c, params(64, 5))
        b.set_lights(abi.RT_LIGHTS_ALL)
        assert b.lights() == [5]
        nee_twin_all = b.render_frame_nee(c, params(64, 5))
    finally:
        a.close()
        b.close()
    rmse = lambda f: float(np.sqrt(np.mean((f - ref) ** 2)))  # noqa: E731
    print("128x128x64 gamma RMSE: original, today's list %.5f; twin, ALL %.5f; twin, default list %.5f"
          % (rmse(nee_original), rmse(nee_twin_all), rmse(nee_twin_default)))
    assert rmse(nee_twin_all) <= 1.25 * rmse(nee_original)
    assert rmse(nee_twin_default) > rmse(nee_twin_all)


# ---- 5. the CLI ------------------------------------------------------------------------------------------------------------------

def test_cli_writes_the_frame_of_the_same_call_through_the_abi(rt, host, abi, gpu):
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "lights", "cornell_box_lamp.yml")
    out = tempfile.mkdtemp(prefix="rt_cli_nee_lights_")
    r = subprocess.run([exe, "-c", config, "-s", scene_yml, "--image-action", "png", "--seed", "1", "--nee", "--nee-lights", "all",
                        "--nee-pick", "power"], capture_output=True, text=True, cwd=out, timeout=600)
    assert r.returncode == 0, r.stderr
    m = re.search(r"Saved image to: (.+)", r.stderr)
    assert m, r.stderr
    path = m.group(1).strip()
    path = path if os.path.isabs(path) else os.path.join(out, path)
    session = host.Session(config, scene=scene_yml, image_action="png", seed=1)
    scene = rt.Scene(session)
    try:
        p, cam = session.params, session.camera
        assert scene.lights() == []
        default = scene.render_frame_nee(cam, p)
        scene.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_POWER)
        assert len(scene.lights()) == 1 and scene.light_weights() == [1.0]
        frame = scene.render_frame_nee(cam, p)
        want = host.pack_rgba8(session.tone_map(frame))
    finally:
        scene.close()
        session.close()
    assert not np.array_equal(frame, default)
    assert np.array_equal(host.decode_image(path), want)
    for bad in (["--nee-lights", "all"], ["--nee-pick", "power", "--adaptive", "0.01"]):
        r = subprocess.run([exe, "-c", config, "-s", scene_yml] + bad, capture_output=True, text=True, cwd=out, timeout=60)
        assert r.returncode == abi.RT_ERR_ARGUMENT_PARSING and "--nee" in r.stderr
