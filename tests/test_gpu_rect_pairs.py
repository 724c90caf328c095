"""The path loop of the rects-only plain variant runs ONE rect test per lane for a facing pair of rects — two rects on
parallel planes with bit-identical bounds, marked by rt_scene_create (racer-tracer_amd/csrc/rt_rect_pairs.h,
rt_pool_coop.h: closest_hit_rects<true>) — and the parent's two whenever a lane's other plane does not lie behind t_min.
Only the fast flavour has the pair form; every case runs the reference flavour too.

What these tests hold, through the C ABI, on the smallest shapes that reach it:
  * cornell_box from inside the box (two marked pairs, every path bounces between them) against the CPU oracle, the same
    addressed draws on both sides: every pixel within 1e-9, sample and segment counts equal (the bounds and shapes of
    tests/test_gpu_primary_point.py), at 16 x 16 spp 16 and at 33 x 21 spp 4 in strips of 3 rows, seeds 1 - 3, max_depth
    2, 3 and 20;
  * the same scene with the pairing DEFEATED — a far-away decoy rect in front of each pair in its group, so that no pair
    starts at an even distance from its group's first record: bit-identical frames, equal counts.  (The decoys lie where
    no ray of this camera can reach them, so the two scenes differ in table positions only);
  * a scene whose facing pair has path origins OUTSIDE its slab: two small facing YZ walls standing on a floor that extends
    well beyond both, under a light.  Paths that leave the floor outside the slab towards a wall's outer face have the
    NEARER plane ahead of them: such a lane is not settled and its wave falls back to both tests.  A numpy model of this
    shape (16 x 16 pixels, 16 samples each, jittered camera rays and normal + unit-sphere directions off the floor, its own
    random numbers) finds 3 112 of the 4 096 primary hits on the floor, 2 282 second segments starting outside the slab
    and 73 of those ending on a wall's outer face;
  * a pair that only LOOKS facing (one bound one ulp off): the unmarked route, against the oracle;
  * the same call twice."""
import functools
import struct

import numpy as np
import pytest

import scenes_py as S

pytestmark = pytest.mark.gpu
abi = S.abi

TIGHT = 1e-9      # f64 against f64 with the same draws (tests/test_gpu_parity.py)
FLAVOURS = {"fast": abi.RT_ARITH_FAST, "reference": abi.RT_ARITH_REFERENCE}
INSIDE = dict(S.cornell_box()[1], look_from=(278.0, 278.0, 100.0), look_at=(278.0, 278.0, 555.0))
ABOVE = dict(look_from=(278.0, 320.0, -250.0), look_at=(278.0, 0.0, 278.0), vfov=60.0, aperture=0.0, focus_distance=10000.0)


def _next_up(x):
    return struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", float(x)))[0] + 1))[0]


def _cornell(decoys=False, one_ulp_off=False):
    c = S.cornell_box()[0]
    prims = list(c.primitives)[:6]
    if one_ulp_off:  # the red wall's y1 and the ceiling's x1: neither pair is one any more
        prims[1] = abi.rect(abi.RT_PRIM_YZ_RECT, 0, _next_up(555), 0, 555, 0, 1, 2)
        prims[3] = abi.rect(abi.RT_PRIM_XZ_RECT, 0, _next_up(555), 0, 555, 555, 2, 4)
    if decoys:       # in front of each group's pair, far behind the camera and tiny
        prims = [abi.rect(abi.RT_PRIM_YZ_RECT, -1e6, -1e6 + 1, -1e6, -1e6 + 1, -1e6, 2, 7),
                 abi.rect(abi.RT_PRIM_XZ_RECT, -1e6, -1e6 + 1, -1e6, -1e6 + 1, -1e6, 2, 8)] + prims
    return abi.SceneBundle(prims, list(c.materials)[:4], list(c.textures)[:4], abi.solid_background((0.0, 0.0, 0.0)))


def _walls_on_a_floor():
    c = S.cornell_box()[0]
    prims = [abi.rect(abi.RT_PRIM_YZ_RECT, 0, 120, 200, 355, 355, 0, 1),        # two facing walls, 155 apart ...
             abi.rect(abi.RT_PRIM_YZ_RECT, 0, 120, 200, 355, 200, 1, 2),
             abi.rect(abi.RT_PRIM_XZ_RECT, -500, 1055, -500, 1055, 0, 2, 3),    # ... on a floor that extends well beyond both
             abi.rect(abi.RT_PRIM_XZ_RECT, 100, 455, 100, 455, 400, 3, 4)]      # the light, above
    return abi.SceneBundle(prims, list(c.materials)[:4], list(c.textures)[:4], abi.solid_background((0.05, 0.05, 0.08)))


SCENES = {"cornell": (_cornell, INSIDE), "decoys": (functools.partial(_cornell, decoys=True), INSIDE),
          "one_ulp_off": (functools.partial(_cornell, one_ulp_off=True), INSIDE), "walls": (_walls_on_a_floor, ABOVE)}


@functools.lru_cache(maxsize=None)
def _oracle(orc, scene, w, h, spp, max_depth, seed):
    """The oracle's frame (tone-mapped) and segment count: computed once, shared by the tests, never written to."""
    make, camera = SCENES[scene]
    frame, segments = orc.render(make().desc, S.camera_for(camera, w, h), abi.render_params(w, h, spp, max_depth=max_depth, seed=seed))
    frame = orc.tone_map(orc.ORC_TM_ACES, frame)
    frame.setflags(write=False)
    return frame, segments


def _render(rt, scene, w, h, spp, max_depth=20, seed=1, flavour="fast", **strips):
    make, camera = SCENES[scene]
    sc = rt.Scene(make(), arithmetic=FLAVOURS[flavour])
    try:
        v = sc.variant()
        assert v["kernel"] == abi.RT_KERNEL_POOL and v["prims_class"] == 0 and not v["textured"] and not v["specular"] and not v["use_bvh"]
        got = sc.render_frame(S.camera_for(camera, w, h), abi.render_params(w, h, spp, max_depth=max_depth, seed=seed, **strips))
        return got, sc.last_stats()
    finally:
        sc.close()


def _held(orc, what, got, samples, segments, ref, ref_segments, n):
    got = orc.tone_map(orc.ORC_TM_ACES, got)
    d = float(np.abs(got - ref).max())
    print("%s: max |delta| %.3g, samples %d of %d, segments %d, oracle %d" % (what, d, samples, n, segments, ref_segments))
    assert np.isfinite(got).all()
    assert d < TIGHT, "max |delta| = %g" % d
    assert samples == n
    assert segments == ref_segments


@pytest.mark.parametrize("flavour", ["fast", "reference"])
@pytest.mark.parametrize("max_depth", [2, 3, 20])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cornell_from_inside_against_the_oracle(rt, orc, gpu, seed, max_depth, flavour):
    ref, ref_segments = _oracle(orc, "cornell", 16, 16, 16, max_depth, seed)
    got, stats = _render(rt, "cornell", 16, 16, 16, max_depth=max_depth, seed=seed, flavour=flavour)
    _held(orc, "16x16 seed %d depth %d %s" % (seed, max_depth, flavour), got, int(stats.samples), int(stats.segments), ref, ref_segments, 16 * 16 * 16)


@pytest.mark.parametrize("flavour", ["fast", "reference"])
@pytest.mark.parametrize("max_depth", [2, 3, 20])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_strips_of_three_rows_against_the_oracle(rt, orc, gpu, seed, max_depth, flavour):
    w, h, spp = 33, 21, 4
    ref, ref_segments = _oracle(orc, "cornell", w, h, spp, max_depth, seed)
    acc, samples, segments = np.full((h, w, 3), -1.0), 0, 0
    for idx in range(2):
        part, stats = _render(rt, "cornell", w, h, spp, max_depth=max_depth, seed=seed, flavour=flavour, strip_rows=3, strip_count=2, strip_index=idx)
        own = ((np.arange(h) // 3) % 2) == idx
        acc[own] = part[own]
        samples += int(stats.samples)
        segments += int(stats.segments)
    _held(orc, "strips seed %d depth %d %s" % (seed, max_depth, flavour), acc, samples, segments, ref, ref_segments, w * h * spp)


@pytest.mark.parametrize("flavour", ["fast", "reference"])
@pytest.mark.parametrize("w,h,spp", [(16, 16, 16), (33, 21, 4)])
def test_the_pairing_defeated_changes_no_bit(rt, gpu, w, h, spp, flavour):
    paired, paired_stats = _render(rt, "cornell", w, h, spp, flavour=flavour)
    single, single_stats = _render(rt, "decoys", w, h, spp, flavour=flavour)
    assert np.array_equal(paired.view(np.uint64), single.view(np.uint64))
    assert int(paired_stats.segments) == int(single_stats.segments) and paired_stats.samples == single_stats.samples == w * h * spp


@pytest.mark.parametrize("flavour", ["fast", "reference"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_origins_outside_the_pairs_slab(rt, orc, gpu, seed, flavour):
    ref, ref_segments = _oracle(orc, "walls", 16, 16, 16, 20, seed)
    got, stats = _render(rt, "walls", 16, 16, 16, seed=seed, flavour=flavour)
    _held(orc, "walls seed %d %s" % (seed, flavour), got, int(stats.samples), int(stats.segments), ref, ref_segments, 16 * 16 * 16)


@pytest.mark.parametrize("flavour", ["fast", "reference"])
def test_a_pair_that_only_looks_facing(rt, orc, gpu, flavour):
    ref, ref_segments = _oracle(orc, "one_ulp_off", 16, 16, 16, 20, 1)
    got, stats = _render(rt, "one_ulp_off", 16, 16, 16, flavour=flavour)
    _held(orc, "one ulp off %s" % flavour, got, int(stats.samples), int(stats.segments), ref, ref_segments, 16 * 16 * 16)


@pytest.mark.parametrize("scene", ["cornell", "walls"])
def test_the_same_call_twice_is_bit_equal(rt, gpu, scene):
    a, a_stats = _render(rt, scene, 33, 21, 4)
    b, b_stats = _render(rt, scene, 33, 21, 4)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert int(a_stats.segments) == int(b_stats.segments) and a_stats.samples == b_stats.samples
