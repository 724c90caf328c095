"""The PRETRACE ring with its fill level kept as a counter and one comparison for "a batch is due"
(racer-tracer_amd/csrc/rt_ring_level.h, rt_trace_pool_kernel.hip) against the CPU oracle.

A level that is off by one entry hands out a slot no batch wrote, or lets a batch write over entries that wait; a batch
rule that fires one batch early does the same, one that never fires again leaves pool entries undrawn.  Each of these
gives other paths than the oracle's: another frame, other sample and segment counts.  The frames are the ones at which
the ring's bookkeeping takes another road:

  cornell_box with the camera INSIDE the box (every entry of every batch lives, so the ring fills to its brim and wraps):
    16 x 16 at 16 spp; 33 x 21 at 4 spp in strips of 3 rows (edge tiles with n_valid != 64 and pools under 64 entries);
    8 x 8 at 1 spp (one batch);
  max_depth 0, 1, 2 and 20 (0 and 1: every entry ends in its batch and the level never leaves 0);
  the camera OUTSIDE (batches most of whose entries end: the hand-out goes short and two batches run in a row);
  an aperture; a coloured background and the sky; seeds 1 - 3; the same call twice;
  a spheres-only scene and a textured, specular one (four sampler rounds), which share the item code around the loop.

Every case in both flavours.  All these forms sum in f64, so the bar is tests/test_gpu_pretrace.py's: every pixel within
1e-9 of the oracle's, sample and segment counts EQUAL to the oracle's."""
import functools

import numpy as np
import pytest

import scenes_py as S
import variant_scenes as V

pytestmark = pytest.mark.gpu
abi = S.abi

TIGHT = 1e-9
FLAVOURS = {"fast": abi.RT_ARITH_FAST, "reference": abi.RT_ARITH_REFERENCE}
_CORNELL_CAMERA = S.cornell_box()[1]
INSIDE = dict(_CORNELL_CAMERA, look_from=(278.0, 278.0, 100.0), look_at=(278.0, 278.0, 555.0))
OUTSIDE = _CORNELL_CAMERA
LENS = dict(INSIDE, aperture=40.0, focus_distance=300.0)
RECTS = (V.RECTS, 0, 0)

# name -> dict(w, h, spp, strips of 3 rows?, camera, max_depth, background, form the scene must select)
def _case(w, h, spp, camera="inside", strips=False, max_depth=20, background="black", scene="cornell"):
    return dict(w=w, h=h, spp=spp, camera=camera, strips=strips, max_depth=max_depth, background=background, scene=scene)


CASES = {
    "inside_16x16_spp16": _case(16, 16, 16),
    "inside_33x21_spp4_strips": _case(33, 21, 4, strips=True),
    "inside_8x8_spp1": _case(8, 8, 1),
    "depth0": _case(16, 16, 4, max_depth=0),
    "depth1": _case(16, 16, 4, max_depth=1),
    "depth2": _case(16, 16, 4, max_depth=2),
    "depth20_outside": _case(24, 16, 8, camera="outside"),
    "depth2_outside": _case(24, 16, 8, camera="outside", max_depth=2),
    "aperture": _case(16, 16, 8, camera="lens"),
    "coloured_background": _case(24, 16, 8, camera="outside", background="coloured"),
    "sky": _case(24, 16, 8, camera="outside", background="sky"),
    "spheres_only": _case(16, 16, 4, scene="spheres"),
    "textured_specular": _case(16, 16, 4, scene="textured_specular"),
}
SEEDED = ("inside_16x16_spp16", "inside_33x21_spp4_strips", "depth20_outside")  # the cases that also run at seeds 2 and 3
BACKGROUNDS = {"black": lambda: abi.solid_background((0.0, 0.0, 0.0)), "coloured": lambda: abi.solid_background((0.1, 0.2, 0.3)),
               "sky": abi.sky}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(bundle, camera dict, form the scene must select) of a case: built once."""
    c = CASES[name]
    if c["scene"] == "cornell":
        cornell = S.cornell_box()[0]
        bundle = abi.SceneBundle(list(cornell.primitives)[:6], list(cornell.materials)[:4], list(cornell.textures)[:4],
                                 BACKGROUNDS[c["background"]]())
        return bundle, {"inside": INSIDE, "outside": OUTSIDE, "lens": LENS}[c["camera"]], RECTS
    form = (V.SPHERES, 0, 0) if c["scene"] == "spheres" else (V.SPHERES, 1, 1)
    bundle, cam = V.build(form + (0,))
    return bundle, cam, form


def _params(name, seed, **strip):
    c = CASES[name]
    return abi.render_params(c["w"], c["h"], c["spp"], max_depth=c["max_depth"], seed=seed, **strip)


@functools.lru_cache(maxsize=None)
def _oracle(orc, name, seed):
    """The oracle's tone-mapped frame and segment count: computed once per case and seed, shared by the flavours."""
    c = CASES[name]
    bundle, cam, _ = _scene(name)
    frame, segments = orc.render(bundle.desc, S.camera_for(cam, c["w"], c["h"]), _params(name, seed))
    frame = orc.tone_map(orc.ORC_TM_ACES, frame)
    frame.setflags(write=False)
    return frame, segments


def _render(rt, name, seed, flavour):
    """-> (frame, samples, segments); a frame in strips is put together from its two strips, the counts added up."""
    c = CASES[name]
    w, h = c["w"], c["h"]
    bundle, cam, form = _scene(name)
    scene = rt.Scene(bundle, arithmetic=FLAVOURS[flavour])
    try:
        v = scene.variant()
        assert v["kernel"] == abi.RT_KERNEL_POOL and (v["prims_class"], v["textured"], v["specular"], v["use_bvh"]) == form + (0,)
        assert v["exact"] == int(flavour == "reference")
        camera = S.camera_for(cam, w, h)
        if not c["strips"]:
            got = scene.render_frame(camera, _params(name, seed))
            stats = scene.last_stats()
            return got, int(stats.samples), int(stats.segments)
        acc, samples, segments = np.full((h, w, 3), -1.0), 0, 0
        for idx in range(2):
            part = scene.render_frame(camera, _params(name, seed, strip_rows=3, strip_count=2, strip_index=idx))
            stats = scene.last_stats()
            own = ((np.arange(h) // 3) % 2) == idx
            assert (part[~own] == 0).all()
            acc[own] = part[own]
            samples += int(stats.samples)
            segments += int(stats.segments)
        return acc, samples, segments
    finally:
        scene.close()


def _seeds_and_names():
    return [(name, seed) for name in sorted(CASES) for seed in ((1, 2, 3) if name in SEEDED else (1,))]


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("name,seed", _seeds_and_names())
def test_the_ring_hands_out_the_oracles_paths(rt, orc, gpu, name, seed, flavour):
    c = CASES[name]
    n = c["w"] * c["h"] * c["spp"]
    ref, ref_segments = _oracle(orc, name, seed)
    got, samples, segments = _render(rt, name, seed, flavour)
    assert np.isfinite(got).all()
    d = float(np.abs(orc.tone_map(orc.ORC_TM_ACES, got) - ref).max())
    print("%s %s seed %d: max |delta| %.3g, samples %d of %d, segments %d, oracle %d" % (name, flavour, seed, d, samples, n, segments, ref_segments))
    assert d < TIGHT, "max |delta| = %g" % d
    assert samples == n
    assert segments == ref_segments
    if c["scene"] == "cornell" and c["camera"] != "outside" and c["max_depth"] >= 2:
        assert segments >= 2 * samples  # inside the box no path ends on its primary segment: every entry of a batch lives


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("name", ["inside_16x16_spp16", "inside_33x21_spp4_strips", "depth20_outside", "depth1"])
def test_the_same_call_twice_is_bit_identical(rt, gpu, name, flavour):
    a, a_samples, a_segments = _render(rt, name, 1, flavour)
    b, b_samples, b_segments = _render(rt, name, 1, flavour)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert (a_samples, a_segments) == (b_samples, b_segments)
