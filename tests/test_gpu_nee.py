"""rt_render_frame_nee on the MI355X: equal to tests/nee_model.py, the plain frame wherever nothing is listed, unbiased
where the model cannot go, less noisy than the plain estimator on cornell_box, deterministic, and the same through every
entry point and the CLI."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import nee_model as NM
import nee_variant_frames as F
import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(abi, w, h, spp, depth=10, seed=1):
    p = abi.render_params(w, h, spp, max_depth=depth)
    p.seed = seed
    return p


def _parity(got, want):
    """The parity tolerance of tests/test_gpu_parity.py: max < 1e-3, fewer than 0.2 % of the pixels beyond 1e-9."""
    d = np.abs(got - want).max(axis=2)
    assert float(d.max()) < 1e-3, float(d.max())
    assert float(np.mean(d > 1e-9)) < 0.002, float(np.mean(d > 1e-9))


def _scene(name, abi):
    if name == "mixed":
        return NM.mixed_scene(abi)
    bundle, cam, _ = getattr(S, name)()
    return bundle, cam


@pytest.mark.parametrize("name", ["cornell_box", "mixed"])
def test_equal_to_the_model(rt, orc, abi, gpu, name):
    bundle, cam = _scene(name, abi)
    c = S.camera_for(cam, 16, 16)
    scene = rt.Scene(bundle)
    model = NM.Model(orc, bundle.desc)
    try:
        for depth, heuristic in ((1, NM.POWER), (3, NM.POWER), (3, NM.BALANCE), (10, NM.POWER), (10, NM.BALANCE)):
            p = _params(abi, 16, 16, 8, depth, seed=7)
            got = scene.render_frame_nee(c, p, heuristic=heuristic)
            segments = scene.last_stats().segments
            want, want_segments = model.render(c, p, heuristic=heuristic)
            _parity(got, want)
            # the same paths: the plain estimator's segment count (shadow rays are not counted)
            _, plain_segments = orc.render(bundle.desc, c, p)
            assert want_segments == plain_segments
            assert abs(int(segments) - plain_segments) <= 4, (depth, segments, plain_segments)
    finally:
        scene.close()


def _wrapped_light_cornell(abi):
    bundle, cam, _ = S.cornell_box()
    prims = list(bundle.primitives)[:6]
    prims[5].flags = abi.RT_PRIM_HAS_TRANSLATE  # a zero Translate: the same light, unlisted
    prims[5].translate = abi.D3(0.0, 0.0, 0.0)
    return abi.SceneBundle(prims, list(bundle.materials)[:4], list(bundle.textures)[:4], bundle.desc.background), cam


@pytest.mark.parametrize("case", ["max_lights_0", "three_balls", "wrapped_light"])
def test_plain_when_nothing_is_listed(rt, orc, abi, gpu, case):
    if case == "wrapped_light":
        bundle, cam = _wrapped_light_cornell(abi)
    else:
        bundle, cam = _scene("three_balls" if case == "three_balls" else "cornell_box", abi)
    c = S.camera_for(cam, 32, 32)
    p = _params(abi, 32, 32, 16, 10, seed=3)
    scene = rt.Scene(bundle)
    try:
        if case != "max_lights_0":
            assert scene.lights() == []
        got = scene.render_frame_nee(c, p, max_lights=0 if case == "max_lights_0" else None)
    finally:
        scene.close()
    want, _ = orc.render(bundle.desc, c, p)
    _parity(got, want)


@pytest.mark.parametrize("case", ["cornell_box_boxes", "emissive", "mixed_bvh"])
def test_unbiased_where_the_model_cannot_go(rt, abi, host, gpu, case):
    """Boxes and wrappers, Perlin and the lens, a BVH: NEE's linear-radiance block means against the plain frame's, with
    standard errors from 8 independent seeds each."""
    session = None
    w, h = 32, 32
    if case == "emissive":  # the scene's own camera, at 32x32 (the aspect changes; the estimators see the same rays)
        session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", "emissive.yml"))
        desc, c = session, session.camera
    else:
        desc, cam = _scene("cornell_box_boxes" if case == "cornell_box_boxes" else "mixed", abi)
        c = S.camera_for(cam, w, h)
    scene = rt.Scene(desc, closest_hit=abi.RT_HIT_BVH if case == "mixed_bvh" else abi.RT_HIT_AUTO)
    try:
        if case == "mixed_bvh":
            assert scene.variant()["use_bvh"] == 1
        nee, plain = [], []
        for k in range(8):
            nee.append(scene.render_frame_nee(c, _params(abi, w, h, 512, 10, seed=100 + k)))
            plain.append(scene.render_frame(c, _params(abi, w, h, 2048, 10, seed=900 + k)))
    finally:
        scene.close()
        if session is not None:
            session.close()
    z = NM.block_z(nee, plain, block=8)
    assert np.all(np.abs(z) <= 5.0), np.abs(z).max()
    assert float(np.mean(z * z)) <= 2.0, float(np.mean(z * z))


def test_less_noise_on_cornell_box(rt, abi, gpu):
    bundle, cam, _ = S.cornell_box()
    c = S.camera_for(cam, 128, 128)
    scene = rt.Scene(bundle)
    try:
        ref = scene.render_frame(c, _params(abi, 128, 128, 16384, 10, seed=77))
        plain = scene.render_frame(c, _params(abi, 128, 128, 64, 10, seed=5))
        nee = scene.render_frame_nee(c, _params(abi, 128, 128, 64, 10, seed=5))
    finally:
        scene.close()
    rmse = lambda f: float(np.sqrt(np.mean((f - ref) ** 2)))  # noqa: E731
    ratio = rmse(nee) / rmse(plain)
    print("cornell_box 128x128x64: gamma RMSE plain %.5f, NEE %.5f, ratio %.3f" % (rmse(plain), rmse(nee), ratio))
    assert ratio <= 0.6, ratio


def test_deterministic_and_independent_of_tiles_and_arithmetic(rt, abi, gpu):
    bundle, cam = NM.mixed_scene(abi)
    c = S.camera_for(cam, 40, 24)
    p = _params(abi, 40, 24, 32, 10, seed=9)
    scene = rt.Scene(bundle)
    exact = rt.Scene(bundle, arithmetic=abi.RT_ARITH_REFERENCE)
    try:
        a = scene.render_frame_nee(c, p)
        assert np.array_equal(a, scene.render_frame_nee(c, p))
        p2 = _params(abi, 40, 24, 32, 10, seed=9)
        p2.tiles_w, p2.tiles_h = 3, 7
        assert np.array_equal(a, scene.render_frame_nee(c, p2))
        assert exact.variant()["exact"] == 1
        _parity(exact.render_frame_nee(c, p), a)
    finally:
        scene.close()
        exact.close()


def test_light_list_and_device_entry_point(rt, abi, gpu):
    import torch
    bundle, cam = NM.mixed_scene(abi)
    for hit in (abi.RT_HIT_LINEAR, abi.RT_HIT_BVH):
        scene = rt.Scene(bundle, closest_hit=hit)
        try:
            assert scene.lights() == NM.light_list(bundle.desc) == [2, 3, 8]
            c = S.camera_for(cam, 24, 16)
            p = _params(abi, 24, 16, 8, 6, seed=4)
            host_frame = scene.render_frame_nee(c, p, max_lights=2)
            dev = torch.device("cuda", 0)
            out = torch.zeros((16, 24, 3), dtype=torch.float64, device=dev)
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                scene.render_frame_nee_device(c, p, out.data_ptr(), stream=stream.cuda_stream, max_lights=2)
            stream.synchronize()
            assert np.array_equal(out.cpu().numpy(), host_frame)
            st = scene.last_stats()
            assert st.samples == 24 * 16 * 8 and st.kernel_ms > 0
        finally:
            scene.close()


def test_cli_nee_writes_the_nee_frame(rt, host, gpu):
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "cornell_box.yml")
    out = tempfile.mkdtemp(prefix="rt_cli_nee_")
    r = subprocess.run([exe, "-c", config, "-s", scene_yml, "--image-action", "png", "--seed", "1", "--nee"],
                       capture_output=True, text=True, cwd=out, timeout=600)
    assert r.returncode == 0, r.stderr
    m = re.search(r"Saved image to: (.+)", r.stderr)
    assert m, r.stderr
    path = m.group(1).strip()
    path = path if os.path.isabs(path) else os.path.join(out, path)
    session = host.Session(config, scene=scene_yml, image_action="png", seed=1)
    scene = rt.Scene(session)
    try:
        p, cam = session.params, session.camera
        want = host.pack_rgba8(session.tone_map(scene.render_frame_nee(cam, p)))
    finally:
        scene.close()
        session.close()
    assert np.array_equal(host.decode_image(path), want)
    for bad in (["--nee", "--adaptive", "0.01"], ["--nee", "--devices", "2"]):
        r = subprocess.run([exe, "-c", config, "-s", scene_yml] + bad, capture_output=True, text=True, cwd=out, timeout=60)
        assert r.returncode != 0 and "--nee" in r.stderr


# ---- k_nee_f64's own dispatch ----------------------------------------------------------------------------------------------
# k_nee_pass_f64 and k_nee_stream_f64 are compared with k_nee_f64, and all three pick their instantiation through one
# dispatcher (rt_variant_dispatch.h): a wrong pick would agree with itself.  So every form of the variant matrix, in both
# flavours, renders the plain estimator through rtdev_launch_nee (max_lights = 0) against the oracle, under the conditions
# tests/test_gpu_variants.py applies to these scenes.

_ORACLE_FRAMES = {}   # form -> (frame, segments): one oracle render serves both flavours


def _oracle_frame(orc, form, bundle, camera, params):
    if form not in _ORACLE_FRAMES:
        _ORACLE_FRAMES[form] = orc.render(bundle.desc, camera, params, use_bvh=V.oracle_use_bvh(bundle))
    return _ORACLE_FRAMES[form]


@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("form", list(V.SPECS), ids=lambda f: "%s%s%s%s" % ("RSA"[f[0]], "t" * f[1], "s" * f[2], "-bvh" * f[3]))
def test_every_variant_of_the_nee_kernel_matches_the_oracle(rt, orc, abi, gpu, form, flavour):
    """Each form's scene selects its form, and the plain estimator through k_nee_f64 (no light listed) is the oracle's frame:
    every linear value within 1e-3, fewer than 1e-3 of them beyond 1e-9 (the oracle against itself: none), a picture and
    not a flat background, and the oracle's path segments to within 4.  (This is the test that found the reference
    arithmetic's <PRIMS_RECTS, plain, SPECULAR> kernels continuing from a wrong origin behind a Fresnel reflection:
    rt_nee_common.h, LABNOTES 10.)"""
    prims_class, textured, specular, bvh = form
    bundle, cam = V.build(form)
    camera = S.camera_for(cam, V.W, V.H)
    params = abi.render_params(V.W, V.H, V.SPP, max_depth=V.DEPTH)
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if bvh else abi.RT_HIT_LINEAR,
                     arithmetic=abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST)
    try:
        variant = scene.variant()
        got = scene.render_frame_nee(camera, params, max_lights=0)
        segments = int(scene.last_stats().segments)
    finally:
        scene.close()
    want = dict(prims_class=prims_class, textured=textured, specular=specular, use_bvh=bvh, exact=int(flavour == "exact"))
    assert {k: variant[k] for k in want} == want
    ref, ref_segments = _oracle_frame(orc, form, bundle, camera, params)
    d = np.abs(got - ref)
    share = float((d > 1e-9).mean())
    print("%s %s: max |delta| = %.3g, share beyond 1e-9 = %.3g, std = %.3g, segments %d (oracle %d)"
          % (form, flavour, d.max(), share, got.std(), segments, ref_segments))
    assert np.isfinite(got).all()
    assert d.max() < 1e-3, "max |delta| = %g" % d.max()
    assert share < 1e-3, "share of values beyond 1e-9: %g" % share   # (a cap: the oracle against itself has share 0)
    assert got.std() > 0.05   # a picture, not a flat background
    assert abs(segments - ref_segments) <= 4, (segments, ref_segments)


# ---- ... and with lights listed ------------------------------------------------------------------------------------------
# Listing a light makes other branches of the same function live: the pick among several lights, the pdf and the sample of
# every rect axis and of a sphere, the shadow ray, both MIS heuristics.  tests/nee_model.py is verified on these scenes by
# tests/test_nee_cpu.py (lights off it is the oracle, its mean is the plain mean, and the frames below move with the lights).

@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("form", list(V.SPECS), ids=lambda f: "%s%s%s%s" % ("RSA"[f[0]], "t" * f[1], "s" * f[2], "-bvh" * f[3]))
def test_every_variant_of_the_nee_kernel_matches_the_model(rt, orc, abi, gpu, form, flavour):
    """Each form's scene with `light2` (XZ, YZ and XY rect lights, two sphere lights, as the class allows) still selects
    its form, lists the model's lights, and k_nee_f64 renders the model's frame under the power heuristic, under the
    balance heuristic, and with the list capped at one light at max_depth 2 (only the first vertex samples a light): the
    parity tolerance each time, a picture, and the model's path segments to within 4 (shadow rays are not counted)."""
    prims_class, textured, specular, bvh = form
    bundle, camera = F.case(abi, form)
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if bvh else abi.RT_HIT_LINEAR,
                     arithmetic=abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST)
    got = []
    try:
        variant = scene.variant()
        lights = scene.lights()
        for heuristic, max_lights, depth in F.RENDERS:
            frame = scene.render_frame_nee(camera, F.params(abi, depth), max_lights=max_lights, heuristic=heuristic)
            got.append((frame, int(scene.last_stats().segments)))
    finally:
        scene.close()
    want = dict(prims_class=prims_class, textured=textured, specular=specular, use_bvh=bvh, exact=int(flavour == "exact"))
    assert {k: variant[k] for k in want} == want
    assert lights == NM.light_list(bundle.desc) and len(lights) == F.N_LIGHTS[prims_class]
    refs = [F.model_frame(orc, abi, form, *r) for r in F.RENDERS]
    for (heuristic, max_lights, depth), (frame, segments), (ref, ref_segments) in zip(F.RENDERS, got, refs):
        d = np.abs(frame - ref)
        print("%s %s %s max_lights %d depth %d: max |delta| = %.3g, share beyond 1e-9 = %.3g, std = %.3g, segments %d (model %d)"
              % (form, flavour, "balance" if heuristic == NM.BALANCE else "power", max_lights, depth, d.max(),
                 float((d.max(axis=2) > 1e-9).mean()), frame.std(), segments, ref_segments))
    for (frame, segments), (ref, ref_segments) in zip(got, refs):
        assert np.isfinite(frame).all()
        _parity(frame, ref)
        assert frame.std() > 0.05   # a picture, not a flat background
        assert abs(segments - ref_segments) <= 4, (segments, ref_segments)
