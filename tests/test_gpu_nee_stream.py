"""rt_render_nee on the device (include/rt_abi.h): the tile stream of the next-event estimator.  The oracle
of every pixel is rt_render_frame_nee — itself held to tests/nee_model.py by tests/test_gpu_nee.py — and the oracle of the
tile sequence is rt_render_ex: sums are per pixel, in f64, in sample order, so the comparison is np.array_equal throughout.
No test asserts a time."""
import hashlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import nee_model as NM
import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(abi, w, h, spp, tiles=(10, 10), depth=10, seed=1):
    p = abi.render_params(w, h, spp, max_depth=depth, tiles_w=tiles[0], tiles_h=tiles[1])
    p.seed = seed
    return p


def _scene(rt, abi, name):
    """-> (Scene, camera description).  name: cornell_box | mixed | mixed_bvh | mixed_exact | cornell_box_v1"""
    if name.startswith("mixed"):
        bundle, cam = NM.mixed_scene(abi)
    else:
        bundle, cam, _ = S.cornell_box()
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if name == "mixed_bvh" else abi.RT_HIT_LINEAR,
                     arithmetic=abi.RT_ARITH_REFERENCE if name == "mixed_exact" else abi.RT_ARITH_FAST,
                     kernel=abi.RT_KERNEL_V1 if name.endswith("_v1") else abi.RT_KERNEL_POOL)
    return scene, cam


def _check_stream(scene, c, p, **kw):
    """One streamed frame against the one-shot frame and rt_render_ex's tile sequence; -> the frame."""
    want = scene.render_frame_nee(c, p, **kw)
    st1 = scene.last_stats()
    frame, order = scene.render_tiles_nee(c, p, **kw)
    st = scene.last_stats()
    assert len(order) == p.tiles_w * p.tiles_h
    assert order == [t[:4] for t in scene.render_tiles(c, p, cancel=lambda: False)]
    assert np.array_equal(frame, want)
    assert st.segments == st1.segments and st.samples == p.width * p.height * p.samples == st1.samples
    assert st.kernel_launches == 1 and st.kernel_ms > 0
    return frame


# ---- 1. bit-identity: scenes, estimator settings, arithmetic, kernels ---------------------------------------------------

CASES_1 = [("cornell_box", {}), ("mixed", {}), ("mixed_bvh", {}), ("mixed_exact", {}), ("cornell_box_v1", {}),
           ("mixed", dict(max_lights=0)), ("mixed", dict(max_lights=1)), ("cornell_box", dict(heuristic=NM.BALANCE)),
           ("mixed", dict(heuristic=NM.BALANCE)), ("mixed", dict(heuristic=NM.POWER))]


@pytest.mark.parametrize("name,kw", CASES_1, ids=["%s-%s" % (c[0], "-".join("%s%s" % kv for kv in sorted(c[1].items())) or "default") for c in CASES_1])
def test_the_stream_is_the_one_shot_frame(rt, abi, gpu, name, kw):
    scene, cam = _scene(rt, abi, name)
    try:
        _check_stream(scene, S.camera_for(cam, 64, 48), _params(abi, 64, 48, 40, tiles=(3, 2), seed=7), **kw)
    finally:
        scene.close()


@pytest.mark.parametrize("name", ["cornell_box_v1", "mixed_bvh", "mixed_exact"])
def test_the_stream_as_a_scenes_first_call(rt, abi, gpu, name):
    """rt_render_nee as the first call on a scene: no other entry point has sized a buffer, so the stream runs on
    enqueue_nee_stream's own allocations.  The one-shot frame comes from a second scene."""
    scene, cam = _scene(rt, abi, name)
    fresh, _ = _scene(rt, abi, name)
    try:
        c, p = S.camera_for(cam, 64, 48), _params(abi, 64, 48, 40, tiles=(3, 2), seed=7)
        frame, order = scene.render_tiles_nee(c, p)
        st = scene.last_stats()
        want = fresh.render_frame_nee(c, p)
        assert len(order) == 6 and np.array_equal(frame, want)
        assert st.segments == fresh.last_stats().segments and st.kernel_launches == 1
        _check_stream(scene, c, p)
    finally:
        scene.close()
        fresh.close()


# ---- 2. sizes and grids --------------------------------------------------------------------------------------------------

CASES_2 = [(64, 48, (3, 2)), (37, 29, (10, 10)), (2, 2, (10, 10)), (400, 16, (40, 1)), (64, 48, (1, 1)), (64, 48, (10, 60))]


@pytest.mark.parametrize("w,h,tiles", CASES_2, ids=["%dx%d-%dx%d" % (c[0], c[1], c[2][0], c[2][1]) for c in CASES_2])
def test_sizes_and_grids(rt, abi, gpu, w, h, tiles):
    # 2x2 with 10x10 tiles: empty tiles and the fallback path; 40 columns: more than RT_MAX_REGIONS, columns share regions
    scene, cam = _scene(rt, abi, "cornell_box")
    try:
        _check_stream(scene, S.camera_for(cam, w, h), _params(abi, w, h, 24, tiles=tiles, seed=3))
    finally:
        scene.close()


# ---- 3. sample counts around the chunk length ------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_sample_counts_around_the_chunk_length(rt, abi, gpu, flavour):
    arith = abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST
    chunk = rt.nee_stream_chunk(arith)
    bundle, cam = NM.mixed_scene(abi)
    c = S.camera_for(cam, 37, 29)
    scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_LINEAR, arithmetic=arith)
    try:
        counts = sorted({1, max(1, chunk - 1), chunk, chunk + 1, 2 * chunk + max(1, chunk // 2) + (1 if chunk == 1 else 0), 3 * chunk})
        assert any(n < chunk for n in counts) or chunk == 1
        assert any(n > chunk and n % chunk for n in counts) or chunk == 1
        for n in counts:
            _check_stream(scene, c, _params(abi, 37, 29, n, tiles=(4, 3), seed=11))
    finally:
        scene.close()


# ---- 4. every variant --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("form", sorted(V.SPECS), ids=lambda f: "p%d-t%d-s%d-b%d" % f)
def test_every_variant_streams_the_one_shot_frame(rt, abi, gpu, form, flavour):
    # (the plain scene lists one light; with `light2` several, of every rect axis and of spheres as the class allows)
    for light2 in (False, True):
        bundle, cam = V.build(form, light2=light2)
        c = S.camera_for(cam, V.W, V.H)
        p = abi.render_params(V.W, V.H, 40, max_depth=V.DEPTH, tiles_w=3, tiles_h=2)
        scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR,
                         arithmetic=abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST)
        try:
            v = scene.variant()
            assert (v["prims_class"], v["textured"], v["specular"], v["use_bvh"]) == form
            assert scene.lights() and (len(scene.lights()) > 1) == light2
            _check_stream(scene, c, p)
        finally:
            scene.close()


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits(rt, abi, gpu):
    scene, cam = _scene(rt, abi, "mixed")
    try:
        c, p = S.camera_for(cam, 200, 120), _params(abi, 200, 120, 48, seed=5)
        a = _check_stream(scene, c, p)
        b, order = scene.render_tiles_nee(c, p, cancel=lambda: False)  # (an armed hook: the waves read the cancel word)
        assert np.array_equal(a, b) and len(order) == 100
    finally:
        scene.close()


# ---- 6. cancel -----------------------------------------------------------------------------------------------------------------

def test_cancel_on_entry(rt, abi, gpu):
    scene, cam = _scene(rt, abi, "cornell_box")
    try:
        c, p = S.camera_for(cam, 64, 48), _params(abi, 64, 48, 8)
        seen = []
        with pytest.raises(rt.RtError) as e:
            scene.render_tiles_nee(c, p, cancel=lambda: True, on_tile=lambda *t: seen.append(t))
        assert e.value.code == abi.RT_ERR_CANCEL_EVENT and not seen
        _check_stream(scene, c, p)  # the scene is as good as new
    finally:
        scene.close()


def test_cancel_from_the_first_tile(rt, abi, gpu):
    """1920x1080 on cornell_box: 32 400 item tiles for ~4 000 resident waves, so the grid needs several rounds and the
    columns do not finish together.  The hook rises inside the first tile's callback: RT_OK, strictly fewer than all tiles,
    every tile that arrived is the one-shot frame's, and the scene renders as a fresh one afterwards through
    rt_render_nee, rt_render_frame_nee and rt_render_ex."""
    w, h, n = 1920, 1080, 128
    scene, cam = _scene(rt, abi, "cornell_box")
    fresh, _ = _scene(rt, abi, "cornell_box")
    try:
        c, p = S.camera_for(cam, w, h), _params(abi, w, h, n)
        want = fresh.render_frame_nee(c, p)
        raised = []
        frame, order = scene.render_tiles_nee(c, p, cancel=lambda: bool(raised), on_tile=lambda *t: raised.append(t))
        started = int(scene.last_stats().samples)
        print("cancelled after %d of 100 tiles; %.1f %% of the primary rays were started" % (len(order), 100.0 * started / (w * h * n)))
        assert 1 <= len(order) < 100
        assert order == [(108 * hs, 192 * ws, 192, 108) for ws in range(10) for hs in range(10)][:len(order)]
        for r, col, tw, th in order:
            assert np.array_equal(frame[r:r + th, col:col + tw], want[r:r + th, col:col + tw])
        small = _params(abi, 320, 180, 24, seed=9)
        cs = S.camera_for(cam, 320, 180)
        for render in (lambda s: s.render_tiles_nee(cs, small)[0], lambda s: s.render_frame_nee(cs, small),
                       lambda s: np.concatenate([t[4].ravel() for t in s.render_tiles(cs, small, cancel=lambda: False)])):
            assert np.array_equal(render(scene), render(fresh))
    finally:
        scene.close()
        fresh.close()


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------------

def test_cli_nee_stream_writes_the_bytes_of_nee(rt, gpu):
    exe = os.path.join(ROOT, "racer-tracer_amd", "bin", "racer-tracer-amd")
    config, scene_yml = os.path.join(ROOT, "scenes", "config_c1.yml"), os.path.join(ROOT, "scenes", "cornell_box.yml")
    digests = {}
    for flag in ("--nee", "--nee-stream"):
        out = tempfile.mkdtemp(prefix="rt_cli_nee_stream_")
        r = subprocess.run([exe, "-c", config, "-s", scene_yml, "--image-action", "png", "--seed", "1", flag],
                           capture_output=True, text=True, cwd=out, timeout=600)
        assert r.returncode == 0, r.stderr
        m = re.search(r"Saved image to: (.+)", r.stderr)
        assert m, r.stderr
        path = m.group(1).strip()
        path = path if os.path.isabs(path) else os.path.join(out, path)
        digests[flag] = hashlib.sha256(open(path, "rb").read()).hexdigest()
    assert digests["--nee"] == digests["--nee-stream"]
    out = tempfile.mkdtemp(prefix="rt_cli_nee_stream_")
    for bad in (["--nee-stream", "--nee"], ["--nee-stream", "--devices", "2"], ["--nee-stream", "--adaptive", "0.01"]):
        r = subprocess.run([exe, "-c", config, "-s", scene_yml] + bad, capture_output=True, text=True, cwd=out, timeout=60)
        assert r.returncode != 0 and "--nee-stream" in r.stderr
