"""The rects-only plain variant of the pooled kernel traces every path's PRIMARY segment in the camera batches
(racer-tracer_amd/csrc/rt_trace_pool_kernel.hip: PRIMARY SEGMENTS IN THE BATCHES): a path that ends there — a miss, a
light, a depth limit of 0 or 1 — never takes a lane, the others wait in a ring with their first hit, and the path loop
starts a lane on its second segment.  Every sample keeps its value; what these tests hold is that no entry is lost,
doubled or given another entry's hit at the places where that bookkeeping can go wrong: tiles cut by the image edge,
pools smaller than a batch, batches that end every entry or none, the ring wrapping over several chunks, an aperture
(per-entry origins), strips that cut tiles, tile lists and the tile stream.

Everything goes through the C ABI against the CPU oracle with the parity tests' own helpers and tolerances."""
import numpy as np
import pytest

import scenes_py as S
from test_gpu_parity import _assert_parity, _both

pytestmark = pytest.mark.gpu


def _with_camera(**cam_overrides):
    def scene_fn():
        bundle, cam, tm = S.cornell_box()
        return bundle, dict(cam, **cam_overrides), tm
    return scene_fn


# C3's own camera: outside the box, half the frame's rays miss, the rest see walls and the light
MIX = _with_camera()
# looking away from the box: every entry ends in its batch, the path loop is never entered
BACKGROUND = _with_camera(look_at=(278.0, 278.0, -1600.0))
# 54 units under the light (213..343 x 227..332 at y = 554), looking up: every primary hit is the light
LIGHT = _with_camera(look_from=(278.0, 500.0, 279.5), look_at=(278.0, 554.0, 280.0))
# inside the box, facing the back wall: every primary hit is a Lambertian wall, no entry ends in a batch (max_depth > 1)
INSIDE = _with_camera(look_from=(278.0, 278.0, 100.0), look_at=(278.0, 278.0, 555.0))
CAMERAS = {"mix": MIX, "background": BACKGROUND, "light": LIGHT, "inside": INSIDE}


def _variant_is_rects_plain(rt):
    bundle, _, _ = S.cornell_box()
    scene = rt.Scene(bundle)
    try:
        return scene.variant()
    finally:
        scene.close()


def _check(rt, orc, scene_fn, w, h, spp, **kw):
    ref, got, ref_segs, stats = _both(rt, orc, scene_fn, w, h, spp, **kw)
    _assert_parity(ref, got)
    assert stats.samples == w * h * spp
    assert abs(int(stats.segments) - ref_segs) <= max(4, ref_segs // 100000)   # (test_gpu_parity's allowance for flips)
    return got, stats


def test_the_scene_runs_the_rects_only_plain_variant(rt, gpu):
    v = _variant_is_rects_plain(rt)
    print(v)
    assert v["kernel"] == S.abi.RT_KERNEL_POOL and v["prims_class"] == 0 and not v["textured"] and not v["specular"] and not v["use_bvh"]
    # the ring fits the LDS the camera batches' buffers took: seven blocks per CU as before, with and without an aperture
    assert v["static_lds"] + v["dyn_lds"] <= 23040 and v["blocks_per_cu"] == 7
    assert v["blocks_per_cu_lens"] >= 5   # (five before: the lens samples' 8 KB per block decide)


# one full tile; tiles cut by the right and the bottom edge; a pool smaller than one batch (2x2: the smallest frame
# rt_render_frame accepts — a 1x1 frame is refused, its pixel coordinates divide by width - 1); C3's mix on several tiles.
# spp 1 and 2: one or two terms per sum, so the frame is the per-sample values themselves; 9: a single chunk; 24 and 70:
# taper and several chunks, the ring wrapping many times
@pytest.mark.parametrize("w,h,spp", [(8, 8, 1), (8, 8, 70), (20, 12, 2), (20, 12, 24), (9, 9, 9), (9, 9, 1), (2, 2, 3), (2, 2, 70),
                                     (64, 40, 2), (64, 40, 24)])
def test_tile_shapes_and_sample_counts(rt, orc, gpu, w, h, spp):
    _check(rt, orc, MIX, w, h, spp)


@pytest.mark.parametrize("max_depth", [0, 1, 2, 20])
@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_cameras_and_depths(rt, orc, gpu, camera, max_depth):
    w, h, spp = 20, 12, 9
    got, stats = _check(rt, orc, CAMERAS[camera], w, h, spp, max_depth=max_depth)
    n = w * h * spp
    if max_depth == 0:
        assert int(stats.segments) == 0                                  # renderer.rs:48-55: white without a segment
    elif max_depth == 1 or camera in ("background", "light"):
        assert int(stats.segments) == n                                  # every path is its primary segment
    elif camera == "inside":
        assert int(stats.segments) >= 2 * n                              # no path ends on its primary segment
    if camera == "background":                                           # (`got` is tone-mapped: Aces of white or of black)
        want = orc.tone_map(orc.ORC_TM_ACES, np.ones_like(got) if max_depth == 0 else np.zeros_like(got))
        assert np.array_equal(got, want)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_per_sample_identity_at_one_and_two_samples(rt, orc, gpu, seed):
    for spp in (1, 2):
        _check(rt, orc, MIX, 64, 40, spp, seed=seed)


@pytest.mark.parametrize("w,h,spp", [(20, 12, 24), (9, 9, 70)])
def test_aperture(rt, orc, gpu, w, h, spp):
    """With an aperture the ray origin is per entry: the lens samples travel through the ring with their entries."""
    _check(rt, orc, _with_camera(aperture=30.0, focus_distance=1000.0), w, h, spp)


def test_reference_arithmetic(rt, orc, gpu):
    """The RT_ARITH_REFERENCE copy of the variant takes the same road."""
    bundle, cam, _ = S.cornell_box()
    w, h, spp = 20, 12, 24
    camera = S.camera_for(cam, w, h)
    params = S.abi.render_params(w, h, spp)
    ref, ref_segs = orc.render(bundle.desc, camera, params)
    scene = rt.Scene(bundle, arithmetic=S.abi.RT_ARITH_REFERENCE)
    try:
        got = scene.render_frame(camera, params)
        stats = scene.last_stats()
    finally:
        scene.close()
    _assert_parity(orc.tone_map(orc.ORC_TM_ACES, ref), orc.tone_map(orc.ORC_TM_ACES, got))
    assert stats.samples == w * h * spp and int(stats.segments) == ref_segs


@pytest.mark.parametrize("rows", [8, 5])
def test_strips(rt, orc, gpu, rows):
    """Two strips of 8 rows (whole item tiles: the very same sums) and of 5 rows (strips that cut tiles: other tiles,
    another order of the additions), assembled and held as test_gpu_parity_proofs holds them."""
    bundle, cam, _ = S.cornell_box()
    w, h, spp = 20, 21, 24
    camera = S.camera_for(cam, w, h)
    scene = rt.Scene(bundle)
    try:
        full = scene.render_frame(camera, S.abi.render_params(w, h, spp))
        acc = np.full_like(full, -1.0)
        traced = 0
        for idx in range(2):
            part = scene.render_frame(camera, S.abi.render_params(w, h, spp, strip_rows=rows, strip_count=2, strip_index=idx))
            traced += int(scene.last_stats().samples)
            own = ((np.arange(h) // rows) % 2) == idx
            assert (part[~own] == 0).all()
            acc[own] = part[own]
    finally:
        scene.close()
    if rows % 8 == 0:
        assert np.array_equal(acc, full)
    else:
        assert np.abs(acc - full).max() < 1e-12
    assert traced == w * h * spp


def test_adaptive_pass_over_a_tile_list(rt, gpu):
    """rt_render_adaptive's passes run over lists of tiles; with the threshold off every tile runs every pass and the
    frame is the one-shot frame."""
    bundle, cam, _ = S.cornell_box()
    w, h, spp = 36, 20, 48
    camera = S.camera_for(cam, w, h)
    params = S.abi.render_params(w, h, spp)
    scene = rt.Scene(bundle)
    try:
        want = scene.render_frame(camera, params)
        frame, samples, _err, _frames = scene.render_adaptive(camera, params, threshold=0.0, pass_samples=24)
        stats = scene.last_stats()
        prog = scene.render_progressive(camera, params, 24)
    finally:
        scene.close()
    assert np.array_equal(frame, want) and (samples == spp).all()
    assert stats.samples == w * h * spp
    assert np.array_equal(prog[-1][1], want)


def test_tile_stream_on_a_two_by_two_grid(rt, gpu):
    bundle, cam, _ = S.cornell_box()
    w, h, spp = 36, 20, 24
    camera = S.camera_for(cam, w, h)
    params = S.abi.render_params(w, h, spp, tiles_w=2, tiles_h=2)
    scene = rt.Scene(bundle)
    try:
        frame = scene.render_frame(camera, params)
        tiles = scene.render_tiles(camera, params)
        stats = scene.last_stats()
    finally:
        scene.close()
    assert len(tiles) == 4
    stitched = np.full_like(frame, -1.0)
    for r, c, tw, th, arr in tiles:
        stitched[r:r + th, c:c + tw] = arr
    assert np.array_equal(stitched, frame)
    assert stats.samples == w * h * spp


def test_the_same_call_twice_is_bit_equal(rt, gpu):
    bundle, cam, _ = S.cornell_box()
    w, h, spp = 64, 40, 70
    camera = S.camera_for(cam, w, h)
    params = S.abi.render_params(w, h, spp)
    scene = rt.Scene(bundle)
    try:
        a = scene.render_frame(camera, params)
        b = scene.render_frame(camera, params)
    finally:
        scene.close()
    assert np.array_equal(a, b)
