"""Rects no camera ray of an item can hit (racer-tracer_amd/csrc/rt_trace_pool_kernel.hip: start_item of the rects-only plain
variant forms a mask per 8x8 item from the host's per-record pixel rectangles, rt_primary_bounds.h: primary_rects, and
closest_hit_rects<false> steps over the records whose bit is clear in the item's camera batches).

The yardstick is tests/test_gpu_primary_cull.py's: the same scene with the masks off BY CONSTRUCTION — cornell_box plus
a decoy behind the camera, which makes the scene's own rectangle the whole frame and with it every record's (ONE decision
per render), so every batch runs every rect test.  Raw f64 frames, `samples` and `segments` must be BIT-IDENTICAL between
the two scenes: a stepped-over test would have changed no `best` and no `best_t`.  That the plain scene's renders do
have items with a proper, non-empty mask is asserted here through the host's own code (tests/primary_rect_bounds_driver.cpp)."""
import numpy as np
import pytest

import primary_bounds_model as M
import scenes_py as S
from test_gpu_parity import _both
from test_gpu_primary_cull import FAR, _Pair, _assert_identical, _camera, _frames
from test_primary_rect_bounds_cpu import AXIS_OF_KIND, N_RECTS, _cam, driver, tile_histogram   # noqa: F401 (driver: a fixture)

pytestmark = pytest.mark.gpu

abi = S.abi
BG = (0.1, 0.2, 0.3)
SHAPES = [(128, 24), (64, 40), (61, 21)]


@pytest.fixture(scope="module")
def pairs(rt, gpu):
    p = _Pair(rt)
    yield p
    p.close()


def _rects_of(prims):
    return [(AXIS_OF_KIND[p.kind], p.p[0], p.p[1], p.p[2], p.p[3], p.p[4]) for p in prims]


def test_the_shapes_have_items_with_a_proper_mask_and_the_decoy_has_none(pairs, driver):
    for scene in pairs.get():
        v = scene.variant()
        assert v["kernel"] == abi.RT_KERNEL_POOL and v["prims_class"] == 0 and not v["textured"] and not v["specular"] and not v["use_bvh"]
    rects = _rects_of(list(S.cornell_box()[0].primitives)[:6])
    for w, h in SHAPES:
        (n, scene_rect, rectangles), = driver([dict(cam=_cam(M.C3_CAMERA, w, h), w=w, h=h, rects=rects)])
        hist = tile_histogram(scene_rect, rectangles[:n], w, h)
        print(w, h, hist)
        assert n == 6 and sum(v for k, v in hist.items() if 0 < k < 6) >= 10
        (n, scene_rect, rectangles), = driver([dict(cam=_cam(M.C3_CAMERA, w, h), w=w, h=h, rects=rects + [(2, 0.0, 1e-6, 0.0, 1e-6, -1e7)])])
        assert n == 0 and scene_rect == (0, w - 1, 0, h - 1) and all(r == scene_rect for r in rectangles)


# edge tiles and n_valid < 64 (61x21); spp 1 and 2: the per-sample values, a pool smaller than a batch on the cut tiles;
# 9: one chunk; 24 and 70: the taper and several chunks
@pytest.mark.parametrize("spp", [1, 2, 9, 24, 70])
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_and_sample_counts(pairs, w, h, spp):
    _, samples, _ = _assert_identical(pairs, w, h, spp)
    assert samples == w * h * spp


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeds(pairs, seed):
    for w, h in SHAPES:
        _assert_identical(pairs, w, h, 9, seed=seed)


@pytest.mark.parametrize("max_depth", [0, 1, 2, 20])
def test_depth_limits(pairs, max_depth):
    for w, h in ((128, 24), (61, 21)):
        _, samples, segments = _assert_identical(pairs, w, h, 9, max_depth=max_depth)
        assert samples == w * h * 9
        assert segments == max_depth * w * h * 9 if max_depth <= 1 else segments > w * h * 9


@pytest.mark.parametrize("arithmetic", [abi.RT_ARITH_FAST, abi.RT_ARITH_REFERENCE])
@pytest.mark.parametrize("background", [(0.0, 0.0, 0.0), (0.25, 0.5, 0.125), BG])
def test_backgrounds_in_both_arithmetics(pairs, arithmetic, background):
    for w, h, spp in ((128, 24, 24), (61, 21, 9)):
        _assert_identical(pairs, w, h, spp, background=background, arithmetic=arithmetic)


@pytest.mark.parametrize("rows", [3, 8])
def test_strips_on_two_shares(pairs, rows):
    """Strips of 8 rows keep the item tiles whole; strips of 3 rows scatter an item's rows over the image, so its mask
    has to come from its pixels, not from a tile's box."""
    for idx in range(2):
        for w, h in ((128, 24), (61, 21), (64, 40)):
            _assert_identical(pairs, w, h, 9, background=BG, strip_rows=rows, strip_count=2, strip_index=idx)


def test_tile_stream_on_a_two_by_two_grid(pairs):
    w, h, spp = 128, 24, 24
    camera, params = _camera(w, h), abi.render_params(w, h, spp, tiles_w=2, tiles_h=2)
    got = []
    for scene in pairs.get(BG):
        tiles = scene.render_tiles(camera, params)
        stats = scene.last_stats()
        got.append((sorted((r, c, tw, th, arr.tobytes()) for r, c, tw, th, arr in tiles), int(stats.samples), int(stats.segments)))
    assert len(got[0][0]) == 4 and got[0] == got[1]


def test_progressive_passes(pairs):
    w, h, spp = 64, 40, 24
    camera, params = _camera(w, h), abi.render_params(w, h, spp)
    got = []
    for scene in pairs.get(BG):
        frames = scene.render_progressive(camera, params, 8)
        stats = scene.last_stats()
        got.append(([(n, arr.tobytes()) for n, arr in frames], int(stats.samples), int(stats.segments)))
    assert len(got[0][0]) >= 2 and got[0] == got[1]


def test_an_adaptive_pass_over_a_tile_list(pairs):
    w, h, spp = 64, 40, 48
    camera, params = _camera(w, h), abi.render_params(w, h, spp)
    got = []
    for scene in pairs.get(BG):
        frame, samples, err, frames = scene.render_adaptive(camera, params, threshold=0.0, pass_samples=24)
        stats = scene.last_stats()
        got.append((frame.tobytes(), samples.tobytes(), err.tobytes(), len(frames), int(stats.samples), int(stats.segments)))
        assert (samples == spp).all()
    assert got[0][3] >= 2 and got[0] == got[1]


def test_a_preview_scale(pairs):
    """The preview's grid cells are every `scale`-th pixel: the rectangles are in image pixels, like the cells."""
    for w, h in ((128, 24), (61, 21)):
        _assert_identical(pairs, w, h, 9, background=BG, scale=2)


def test_a_camera_far_away(pairs):
    for spp in (2, 24):
        _assert_identical(pairs, 128, 24, spp, background=BG, cam=FAR)


def test_an_aperture_turns_the_masks_off(pairs):
    _assert_identical(pairs, 128, 24, 24, background=BG, cam=dict(aperture=30.0, focus_distance=1000.0))


def _scene_of(rt, prims):
    bundle = S.cornell_box()[0]
    return rt.Scene(abi.SceneBundle(prims, list(bundle.materials)[:4], list(bundle.textures)[:4], abi.solid_background(BG)))


def _same_frames(scenes, w, h, spp, cam=None):
    camera, params = _camera(w, h, **(cam or {})), abi.render_params(w, h, spp)
    try:
        got = [_frames(scene, camera, params) for scene in scenes]
    finally:
        for scene in scenes:
            scene.close()
    for frame, samples, segments in got[1:]:
        assert np.array_equal(frame, got[0][0]) and (samples, segments) == got[0][1:]
    return got[0]


def test_one_record_more_than_there_are_rectangles(rt, gpu):
    """Fillers no ray reaches (1e-6 wide, behind the back wall): with N records every one has a rectangle, with N + 1
    none has — and with the decoy none either."""
    walls = list(S.cornell_box()[0].primitives)[:6]
    filler = lambda j: abi.rect((abi.RT_PRIM_XY_RECT, abi.RT_PRIM_XZ_RECT, abi.RT_PRIM_YZ_RECT)[j % 3], 100.0 + j, 100.0 + j + 1e-6, 600.0, 600.0 + 1e-6, 600.0, 2, 10 + j)
    at_n = walls + [filler(j) for j in range(N_RECTS - 6)]
    decoy = abi.rect(abi.RT_PRIM_XY_RECT, 0.0, 1e-6, 0.0, 1e-6, -1e7, 2, 7)
    for w, h in ((128, 24), (61, 21)):
        frame, samples, _ = _same_frames([_scene_of(rt, at_n), _scene_of(rt, at_n + [filler(N_RECTS)]), _scene_of(rt, at_n[:-1] + [decoy])], w, h, 9)
        assert samples == w * h * 9
        plain, _, _ = _same_frames([_scene_of(rt, walls)], w, h, 9)
        assert np.array_equal(frame, plain)   # (the fillers change nothing but the records' indices)


@pytest.mark.parametrize("name,cam", [
    # one rect, the light, seen from below and to the side: its image leaves the frame at one edge
    ("partly off the frame", dict(look_from=(278.0, 100.0, 279.5), look_at=(150.0, 554.0, 280.0), vfov=40.0)),
    # ... and from its own plane y = 554: the rectangle is a row or two, or the doubt of an ill-conditioned corner
    ("edge-on", dict(look_from=(278.0, 554.0, -800.0), look_at=(278.0, 554.0, 0.0), vfov=40.0)),
])
def test_a_single_rect_with_a_degenerate_rectangle(rt, orc, gpu, name, cam):
    light = list(S.cornell_box()[0].primitives)[5:6]
    decoy = abi.rect(abi.RT_PRIM_XY_RECT, 0.0, 1e-6, 0.0, 1e-6, -1e7, 2, 7)
    for w, h in ((64, 40), (61, 21)):
        frame, samples, segments = _same_frames([_scene_of(rt, light), _scene_of(rt, light + [decoy])], w, h, 9, cam=cam)
        assert samples == w * h * 9 and segments == samples   # a light and a background: every path is one segment
        hit = (frame != np.sqrt(np.array(BG))).any(axis=-1)
        if name == "partly off the frame":
            # (the camera looks up along y, so the image's vertical axis is x: the light's x = 213..343 is 63..193 beside
            # the axis through x = 150, and the frame ends 165 = 454 tan 20 from it)
            assert (hit[0].any() or hit[-1].any()) and not hit[:, 0].any() and not hit[:, -1].any()


@pytest.mark.parametrize("w,h,spp", [(64, 40, 2), (61, 21, 9)])
def test_parity_with_the_oracle(rt, orc, gpu, w, h, spp):
    """Raw frames (tone map None would be the same test: 1e-9 on the tone-mapped values of cornell's Aces), equal segment counts."""
    ref, got, ref_segs, stats = _both(rt, orc, S.cornell_box, w, h, spp)
    diff = float(np.abs(ref - got).max())
    print("max |delta| %.3g, segments %d / %d" % (diff, int(stats.segments), ref_segs))
    assert diff <= 1e-9
    assert int(stats.segments) == ref_segs and stats.samples == w * h * spp
