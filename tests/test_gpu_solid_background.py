"""What a path adds to its pixel when it leaves the scene, in the path loop of the rects-only plain variant of the pooled
kernel (racer-tracer_amd/csrc/rt_trace_pool_kernel.hip: A BLACK BACKGROUND).  With a solid background whose components
all compare equal to 0.0 the host sets TraceArgs.bg_black and the lanes that miss take no part in the additions: the
frame must be what adding their zeros gave.  Any other solid colour is multiplied into the throughput as scalar
operands, a sky keeps its arm.

The scene is the Cornell box seen from outside (tests/scenes_py.py): a path that scatters off a wall leaves through the
open front, at any depth, so every sample count and depth limit below has lanes in the miss arm.  Everything goes
through the C ABI against the CPU oracle with the parity tests' own helpers and tolerances; segment and sample counts as
tests/test_gpu_pretrace.py holds them."""
import functools

import numpy as np
import pytest

import scenes_py as S
from test_gpu_parity import _assert_parity

pytestmark = pytest.mark.gpu

W = H = 16
BACKGROUNDS = {
    "black": lambda: S.abi.solid_background((0.0, 0.0, 0.0)),
    "minus_zero": lambda: S.abi.solid_background((-0.0, 0.0, 0.0)),
    "colour": lambda: S.abi.solid_background((0.3, 0.5, 0.7)),
    "tiny_blue": lambda: S.abi.solid_background((0.0, 0.0, 1e-300)),     # not black: the flag is off
    "sky": lambda: S.abi.sky(),
}
FLAVOURS = {"fast": S.abi.RT_ARITH_FAST, "reference": S.abi.RT_ARITH_REFERENCE}


def _bundle(background):
    cornell, cam, _ = S.cornell_box()
    bundle = S.abi.SceneBundle(list(cornell.primitives)[:6], list(cornell.materials)[:4], list(cornell.textures)[:4], BACKGROUNDS[background]())
    return bundle, S.camera_for(cam, W, H)


@functools.lru_cache(maxsize=None)
def _oracle(orc, background, spp, max_depth):
    """The oracle's frame and segment count: computed once, shared by the flavours, never written to."""
    bundle, camera = _bundle(background)
    frame, segments = orc.render(bundle.desc, camera, S.abi.render_params(W, H, spp, max_depth=max_depth))
    frame.setflags(write=False)
    return frame, segments


def _render(rt, background, flavour, spp, max_depth):
    bundle, camera = _bundle(background)
    scene = rt.Scene(bundle, arithmetic=FLAVOURS[flavour])
    try:
        got = scene.render_frame(camera, S.abi.render_params(W, H, spp, max_depth=max_depth))
        return got, scene.last_stats()
    finally:
        scene.close()


@pytest.mark.parametrize("max_depth", [2, 20])
@pytest.mark.parametrize("spp", [1, 2, 40])
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("background", sorted(BACKGROUNDS))
def test_backgrounds_against_the_oracle(rt, orc, gpu, background, flavour, spp, max_depth):
    ref, ref_segs = _oracle(orc, background, spp, max_depth)
    got, stats = _render(rt, background, flavour, spp, max_depth)
    _assert_parity(orc.tone_map(orc.ORC_TM_ACES, ref), orc.tone_map(orc.ORC_TM_ACES, got))
    assert stats.samples == W * H * spp
    assert abs(int(stats.segments) - ref_segs) <= max(4, ref_segs // 100000)   # (test_gpu_parity's allowance for flips)


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_both_zeros_give_the_same_frame(rt, gpu, flavour):
    """(-0.0, 0, 0) compares equal to zero: the flag is set, and the frame is the (0, 0, 0) frame bit for bit — in the
    batches too, where the entries that miss do add their -0.0 to a sum that starts at +0.0."""
    for spp, max_depth in ((1, 20), (40, 2), (40, 20)):
        black, black_stats = _render(rt, "black", flavour, spp, max_depth)
        minus, minus_stats = _render(rt, "minus_zero", flavour, spp, max_depth)
        assert np.array_equal(black.view(np.uint64), minus.view(np.uint64))
        assert int(black_stats.segments) == int(minus_stats.segments) and black_stats.samples == minus_stats.samples


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_the_flag_on_one_side_only(rt, gpu, flavour):
    """(0, 0, 1e-300) is not black, so its missing lanes multiply and add: zeros to the red and green sums, which must
    then be the sums of the (0, 0, 0) frame, whose missing lanes add nothing, bit for bit.  The paths are the same
    paths: equal counts."""
    for spp, max_depth in ((1, 20), (40, 2), (40, 20)):
        black, black_stats = _render(rt, "black", flavour, spp, max_depth)
        tiny, tiny_stats = _render(rt, "tiny_blue", flavour, spp, max_depth)
        assert black.dtype == np.float64 and black.shape == (H, W, 3)
        assert np.array_equal(black[..., :2].view(np.uint64), tiny[..., :2].view(np.uint64))
        assert int(black_stats.segments) == int(tiny_stats.segments) and black_stats.samples == tiny_stats.samples
    assert (black > 0).any()    # (not a black frame: the walls and the light are on it)
