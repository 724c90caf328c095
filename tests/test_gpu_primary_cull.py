"""Items no camera ray can hit (racer-tracer_amd/csrc/rt_trace_pool_kernel.hip: start_item of the rects-only plain variant;
rt_primary_bounds.h): an 8x8 item without a pixel inside the host's rectangle takes none of the camera batches — its sums
are the background added once per sample, its counters grow as the batches count.

The yardstick is the same scene with the cull off BY CONSTRUCTION: cornell_box plus a decoy, a 1e-6-wide Lambertian XY
rect at z = -1e7, behind the camera.  One corner of the scene's box is then not in front of the camera, so the rectangle
is the whole frame and every item runs its batches; no ray reaches the decoy (its solid angle is about 1e-26).  Raw f64
frames, `samples` and `segments` must be BIT-IDENTICAL between the two scenes.  That the plain scene's renders do have
culled items is held on the CPU (tests/test_primary_bounds_cpu.py: every shape used here has tiles wholly outside the
rectangle) and counted here with the same numpy model."""
import numpy as np
import pytest

import primary_bounds_model as M
import scenes_py as S
from test_gpu_pretrace import _check

pytestmark = pytest.mark.gpu

abi = S.abi
FAR = dict(look_from=(278.0, 278.0, -20000.0))   # the box covers a few pixels: nearly every tile is culled


def _bundle(decoy, background=(0.0, 0.0, 0.0)):
    bundle, cam, tm = S.cornell_box()
    prims = list(bundle.primitives)[:6]
    if decoy:
        prims.append(abi.rect(abi.RT_PRIM_XY_RECT, 0.0, 1e-6, 0.0, 1e-6, -1e7, 2, 7))
    return abi.SceneBundle(prims, list(bundle.materials)[:4], list(bundle.textures)[:4], abi.solid_background(background)), cam, tm


class _Pair:
    """The scene and the scene with the decoy, kept for the module (one pair per background and arithmetic)."""

    def __init__(self, rt):
        self.rt, self.scenes = rt, {}

    def get(self, background=(0.0, 0.0, 0.0), arithmetic=abi.RT_ARITH_FAST):
        key = (tuple(background), arithmetic)
        if key not in self.scenes:
            self.scenes[key] = tuple(self.rt.Scene(_bundle(decoy, background)[0], arithmetic=arithmetic) for decoy in (False, True))
        return self.scenes[key]

    def close(self):
        for pair in self.scenes.values():
            for scene in pair:
                scene.close()


@pytest.fixture(scope="module")
def pairs(rt, gpu):
    p = _Pair(rt)
    yield p
    p.close()


def _camera(w, h, **overrides):
    return S.camera_for(dict(S.cornell_box()[1], **overrides), w, h)


def _culled_tiles(w, h, **overrides):
    spec = dict(M.C3_CAMERA, **overrides)
    cam = M.camera(spec["look_from"], spec["look_at"], spec["vfov"], spec["aperture"], spec["focus_distance"], w, h)
    rect = M.model_rect(cam, w, h, *M.CORNELL_BOX)
    return 0 if rect is None else M.tiles_outside(rect, w, h)[0]


def _frames(scene, camera, params):
    frame = scene.render_frame(camera, params)
    stats = scene.last_stats()
    return frame, int(stats.samples), int(stats.segments)


def _assert_identical(pairs, w, h, spp, background=(0.0, 0.0, 0.0), arithmetic=abi.RT_ARITH_FAST, cam=None, **params_kw):
    plain, decoy = pairs.get(background, arithmetic)
    camera = _camera(w, h, **(cam or {}))
    params = abi.render_params(w, h, spp, **params_kw)
    a, a_samples, a_segments = _frames(plain, camera, params)
    b, b_samples, b_segments = _frames(decoy, camera, params)
    assert np.array_equal(a, b), "max |diff| %g in %d pixels" % (np.abs(a - b).max(), int((a != b).any(axis=-1).sum()))
    assert (a_samples, a_segments) == (b_samples, b_segments)
    return a, a_samples, a_segments


def test_the_scenes_run_the_rects_only_plain_variant_and_have_culled_tiles(pairs):
    for scene in pairs.get():
        v = scene.variant()
        assert v["kernel"] == abi.RT_KERNEL_POOL and v["prims_class"] == 0 and not v["textured"] and not v["specular"] and not v["use_bvh"]
    assert _culled_tiles(128, 24) == 36 and _culled_tiles(64, 40) > 0 and _culled_tiles(61, 21) > 0
    assert _culled_tiles(128, 24, **FAR) >= 44
    assert _culled_tiles(128, 24, aperture=30.0, focus_distance=1000.0) == 0


# 128x24: 12 of the 16 tile columns are culled; 61x21: tiles cut by the image edge inside culled columns.  spp 1 and 2: the
# per-sample values; 9: one chunk; 24 and 70: the taper and several chunks
@pytest.mark.parametrize("w,h,spp", [(128, 24, 1), (128, 24, 2), (128, 24, 24), (128, 24, 70), (64, 40, 9), (61, 21, 9)])
def test_shapes_and_sample_counts(pairs, w, h, spp):
    _, samples, _ = _assert_identical(pairs, w, h, spp)
    assert samples == w * h * spp


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeds(pairs, seed):
    _assert_identical(pairs, 128, 24, 24, seed=seed)
    _assert_identical(pairs, 61, 21, 9, seed=seed)


@pytest.mark.parametrize("max_depth", [0, 1, 2, 20])
def test_depth_limits(pairs, max_depth):
    """max_depth 0 keeps the batches (white, no segment); 1 ends every path on its primary segment."""
    w, h, spp = 128, 24, 24
    frame, samples, segments = _assert_identical(pairs, w, h, spp, max_depth=max_depth)
    assert samples == w * h * spp
    if max_depth <= 1:
        assert segments == max_depth * w * h * spp
    else:
        assert segments > w * h * spp
    if max_depth == 0:
        assert (frame == 1.0).all()


@pytest.mark.parametrize("arithmetic", [abi.RT_ARITH_FAST, abi.RT_ARITH_REFERENCE])
@pytest.mark.parametrize("background", [(0.0, 0.0, 0.0), (0.25, 0.5, 0.125), (0.1, 0.2, 0.3)])
def test_backgrounds_in_both_arithmetics(pairs, arithmetic, background):
    """(0.1, 0.2, 0.3) pins the repeated addition: n additions of 0.1 are not n * 0.1."""
    for w, h, spp in ((128, 24, 70), (61, 21, 9)):
        frame, _, _ = _assert_identical(pairs, w, h, spp, background=background, arithmetic=arithmetic)
        # a culled column shows the background alone: sqrt(sum / spp) of spp equal terms, up to the sums' rounding
        assert np.allclose(frame[:, 0], np.sqrt(np.array(background)), rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("rows", [3, 8])
def test_strips_on_two_shares(pairs, rows):
    """Strips of 8 rows keep the item tiles whole; strips of 3 rows cut them (the per-lane row map)."""
    for idx in range(2):
        for w, h in ((128, 24), (61, 21)):
            _assert_identical(pairs, w, h, 24, background=(0.1, 0.2, 0.3), strip_rows=rows, strip_count=2, strip_index=idx)


def test_tile_stream_on_a_two_by_two_grid(pairs):
    w, h, spp = 128, 24, 24
    camera, params = _camera(w, h), abi.render_params(w, h, spp, tiles_w=2, tiles_h=2)
    got = []
    for scene in pairs.get((0.1, 0.2, 0.3)):
        tiles = scene.render_tiles(camera, params)
        stats = scene.last_stats()
        got.append((sorted((r, c, tw, th, arr.tobytes()) for r, c, tw, th, arr in tiles), int(stats.samples), int(stats.segments)))
    assert len(got[0][0]) == 4 and got[0] == got[1]


def test_progressive_passes(pairs):
    w, h, spp = 128, 24, 24
    camera, params = _camera(w, h), abi.render_params(w, h, spp)
    got = []
    for scene in pairs.get((0.1, 0.2, 0.3)):
        frames = scene.render_progressive(camera, params, 8)
        stats = scene.last_stats()
        got.append(([(n, arr.tobytes()) for n, arr in frames], int(stats.samples), int(stats.segments)))
    assert len(got[0][0]) >= 2 and got[0] == got[1]


def test_an_adaptive_pass_over_a_tile_list(pairs):
    """With the threshold off every tile runs every pass: the passes behind the first run over a list of tiles."""
    w, h, spp = 128, 24, 48
    camera, params = _camera(w, h), abi.render_params(w, h, spp)
    got = []
    for scene in pairs.get((0.1, 0.2, 0.3)):
        frame, samples, err, frames = scene.render_adaptive(camera, params, threshold=0.0, pass_samples=24)
        stats = scene.last_stats()
        got.append((frame.tobytes(), samples.tobytes(), err.tobytes(), len(frames), int(stats.samples), int(stats.segments)))
        assert (samples == spp).all()
    assert got[0][3] >= 2 and got[0] == got[1]


def test_a_camera_far_away(pairs):
    for spp in (2, 24):
        frame, samples, _ = _assert_identical(pairs, 128, 24, spp, background=(0.1, 0.2, 0.3), cam=FAR)
        assert samples == 128 * 24 * spp
        assert (frame[:, :56] == frame[0, 0]).all() and (frame[:, 72:] == frame[0, 0]).all()   # the background, left and right of the box


def test_an_aperture_turns_the_cull_off(pairs):
    _assert_identical(pairs, 128, 24, 24, background=(0.1, 0.2, 0.3), cam=dict(aperture=30.0, focus_distance=1000.0))


@pytest.mark.parametrize("w,h,spp", [(128, 24, 24), (61, 21, 9)])
def test_parity_with_the_oracle(rt, orc, gpu, w, h, spp):
    _check(rt, orc, S.cornell_box, w, h, spp)
