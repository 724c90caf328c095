"""Waves that take work item after work item (rt_trace_pool_kernel.hip: start_item, OVERLAP; rt_pool_deliver.h;
rt_nee_stream.h), at the size of the small tests.

A persistent launch has min(resident blocks, (items + 3) / 4) blocks of four waves.  On a card with thousands of resident
waves a frame of a few hundred items therefore gives every wave ONE item: what start_item re-sets between two items (the
path state, the LDS pixel sums, the batch bookkeeping, the ring of the rects-only variant, the lens and time tables), the
two items the any-primitive and BVH forms keep in flight, and the last-chunk-has-landed step of the delivering launch
are then run by full-size frames alone.  RtSceneOptions.launch_blocks caps the grid (a test switch; include/rt_abi.h):
with a cap of c blocks, 4 c waves share the frame's items.

Every capped case first asserts, from rtdev_scene_variant's last_launch_blocks / last_launch_items, that the cap took
effect and that the launch had at least 8 items per wave (FLOOR items per block).  Where a source test's frame is too small
for that, the frame here is larger and the docstring says so; the floor is never lowered.

What is held: a capped frame equals the uncapped frame BIT FOR BIT, with equal sample and segment counts.  That is what
the code promises for both kinds of sums: an item's f64 sums go to the item's own slice and the slices are added in chunk
order (rt_trace_pool_kernel.hip, idea 2), and the fixed-point sums of the two-item forms are integers (rt_abi.h).  The
uncapped frame meets the oracle at the bar of the test its shape comes from, imported from there."""
import functools
import types

import numpy as np
import pytest

import adaptive_model as M
import nee_model as NM
import scenes_py as S
import variant_scenes as V
from test_gpu_adaptive import _assert_threshold_off_is_one_shot
from test_gpu_group_sizes import TIGHT
from test_gpu_group_sizes import _scene as _group_sizes_scene
from test_gpu_nee_stream import _check_stream
from test_gpu_parity import _assert_parity
from test_gpu_pretrace import CAMERAS
from test_gpu_progressive import _assert_last_is_one_shot
from test_gpu_variants import LENS_CAM, assert_parity, lds_scene

pytestmark = pytest.mark.gpu
abi = S.abi

FLOOR = 8 * 4   # items per block of four waves: eight items per wave


def _form_id(form):
    return "%s%s%s%s" % ("RSA"[form[0]], "t" if form[1] else "", "s" if form[2] else "", "-bvh" if form[3] else "")


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _assert_capped(scene, cap, what=""):
    """The scene's most recent persistent launch had `cap` blocks and at least FLOOR items for each."""
    v = scene.variant()
    blocks, items = v["last_launch_blocks"], v["last_launch_items"]
    print("%s cap %d: %d blocks, %d items, %.1f items per wave" % (what, cap, blocks, items, items / (4.0 * max(blocks, 1))))
    assert blocks == cap, (what, cap, blocks, items)
    assert items >= FLOOR * cap, (what, cap, blocks, items)


def _assert_uncapped(scene, caps, what=""):
    """... and without the cap the grid is larger than every cap the case uses (or the caps would prove nothing)."""
    v = scene.variant()
    print("%s uncapped: %d blocks, %d items" % (what, v["last_launch_blocks"], v["last_launch_items"]))
    assert v["last_launch_blocks"] > max(caps) and v["last_launch_items"] >= FLOOR * max(caps), (what, v)


def _flavour_options(flavour):
    return dict(arithmetic=abi.RT_ARITH_REFERENCE if flavour == "exact" else abi.RT_ARITH_FAST)


# ---- a. every pooled instantiation --------------------------------------------------------------------------------------

A_SPP = 24          # chunk_plan(24): chunks of 12, 8 and 4 samples (a taper); 40 tiles x 3 chunks = 120 items
A_CAPS = (1, 3)     # 3 divides neither 120 nor the wave count of 1: the waves finish at different times


@functools.lru_cache(maxsize=None)
def _variant_oracle(orc, form):
    """The oracle's frame of V.build(form) at 64x36x24 and its segment count: once per form, shared by the flavours."""
    bundle, cam = V.build(form)
    ref, segments = orc.render(bundle.desc, S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, A_SPP, max_depth=V.DEPTH),
                               use_bvh=V.oracle_use_bvh(bundle))
    ref.setflags(write=False)
    return ref, segments


@pytest.mark.parametrize("flavour", ["fast", "exact"])
@pytest.mark.parametrize("form", list(V.SPECS), ids=_form_id)
def test_every_pooled_instantiation_with_waves_that_take_items_in_a_row(rt, orc, gpu, form, flavour):
    """All 16 forms in both flavours at 64x36x24: launch_blocks 1 (four waves, 30 items each) and 3 (twelve waves, ten each,
    uneven) against the uncapped launch (one item per wave), bit for bit; the uncapped frame against the oracle at
    test_gpu_variants' bars, the oracle's segment count exact in the reference flavour."""
    bundle, cam = V.build(form)
    camera, params = S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, A_SPP, max_depth=V.DEPTH)
    got = {}
    for cap in (0,) + A_CAPS:
        scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR, launch_blocks=cap,
                         **_flavour_options(flavour))
        try:
            v = scene.variant()
            assert (v["kernel"], v["prims_class"], v["textured"], v["specular"], v["use_bvh"], v["exact"]) == \
                (abi.RT_KERNEL_POOL,) + form + (int(flavour == "exact"),)
            assert (v["last_launch_blocks"], v["last_launch_items"]) == (0, 0)     # nothing launched yet
            frame = scene.render_frame(camera, params)
            if cap:
                _assert_capped(scene, cap, "%s %s" % (_form_id(form), flavour))
            else:
                _assert_uncapped(scene, A_CAPS, "%s %s" % (_form_id(form), flavour))
            got[cap] = (frame, scene.last_stats())
        finally:
            scene.close()
    whole, stats = got[0]
    for cap in A_CAPS:
        frame, st = got[cap]
        differing = int((frame.view(np.uint64) != whole.view(np.uint64)).sum())
        assert differing == 0, "launch_blocks %d: %d of %d values differ, max |delta| = %g" % (
            cap, differing, whole.size, np.abs(frame - whole).max())
        assert (st.samples, st.segments) == (stats.samples, stats.segments), cap
    ref, ref_segments = _variant_oracle(orc, form)
    assert_parity(orc, whole, stats, ref, ref_segments, V.W, V.H, A_SPP, flavour == "exact")
    assert whole.std() > 0.05   # a picture, not a flat background


# ---- b. the shapes the small tests were written for, with succession ------------------------------------------------------

B_CAPS = (1, 2)
# one scene per item loop of the kernel: name -> form it must select
LOOPS = {"rects": (V.RECTS, 0, 0, 0),            # the PRETRACE loop; test_gpu_group_sizes' camera inside the Cornell box
         "spheres_ts": (V.SPHERES, 1, 1, 0),     # one item at a time, f64 sums, four sampler rounds
         "any": (V.ANY, 0, 0, 0),                # two items in flight, linear loop
         "bvh": (V.ANY, 0, 0, 1)}                # two items in flight, the tree


@functools.lru_cache(maxsize=None)
def _loop_scene(name):
    """-> (bundle, camera dict, Scene options without the cap, the oracle's use_bvh)"""
    if name == "rects":
        bundle, cam = _group_sizes_scene("cornell_8x8")
        return bundle, cam, {}, 1
    bundle, cam = V.build(LOOPS[name])
    return bundle, cam, dict(closest_hit=abi.RT_HIT_BVH if LOOPS[name][3] else abi.RT_HIT_LINEAR), V.oracle_use_bvh(bundle)


def _open(rt, name, cap, **more):
    bundle, _, options, _ = _loop_scene(name)
    scene = rt.Scene(bundle, launch_blocks=cap, **dict(options, **more))
    v = scene.variant()
    assert (v["kernel"], v["prims_class"], v["textured"], v["specular"], v["use_bvh"]) == (abi.RT_KERNEL_POOL,) + LOOPS[name], v
    return scene


def _assert_same_bits(got, caps):
    """got: cap -> (frame, samples, segments); every capped entry equals entry 0."""
    whole, samples, segments = got[0]
    for cap in caps:
        frame, n, s = got[cap]
        differing = int((frame.view(np.uint64) != whole.view(np.uint64)).sum())
        assert differing == 0, "launch_blocks %d: %d of %d values differ, max |delta| = %g" % (
            cap, differing, whole.size, np.abs(frame - whole).max())
        assert (n, s) == (samples, segments), (cap, n, s, samples, segments)


STRIPS = (97, 69, 4)    # test_gpu_group_sizes' 33x21x4 in two strips of 3 rows has 10 items a strip; 97x69 has 13 x 5 = 65,
                        # still 8 k + 1 pixels wide, tiles cut by the bottom edge and by every strip


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_strips_that_cut_tiles_with_succession(rt, orc, gpu, name):
    """Two strips of 3 rows: items of a few pixels each, 65 per strip, through four and eight waves.  The rects scene is the
    one test_gpu_group_sizes renders and meets its bar (every pixel within 1e-9, the oracle's counts); the three
    variant_scenes scenes meet test_gpu_variants' bar, the one they are held to there."""
    w, h, spp = STRIPS
    bundle, cam, _, use_bvh = _loop_scene(name)
    camera = S.camera_for(cam, w, h)
    got = {}
    for cap in (0,) + B_CAPS:
        scene = _open(rt, name, cap)
        try:
            acc, samples, segments = np.full((h, w, 3), -1.0), 0, 0
            for idx in range(2):
                part = scene.render_frame(camera, abi.render_params(w, h, spp, strip_rows=3, strip_count=2, strip_index=idx))
                if cap:
                    _assert_capped(scene, cap, "%s strip %d" % (name, idx))
                else:
                    _assert_uncapped(scene, B_CAPS, "%s strip %d" % (name, idx))
                stats = scene.last_stats()
                own = ((np.arange(h) // 3) % 2) == idx
                assert (part[~own] == 0).all()
                acc[own] = part[own]
                samples += int(stats.samples)
                segments += int(stats.segments)
            got[cap] = (acc, samples, segments)
        finally:
            scene.close()
    _assert_same_bits(got, B_CAPS)
    whole, samples, segments = got[0]
    ref, ref_segments = orc.render(bundle.desc, camera, abi.render_params(w, h, spp), use_bvh=use_bvh)
    d = float(np.abs(orc.tone_map(orc.ORC_TM_ACES, whole) - orc.tone_map(orc.ORC_TM_ACES, ref)).max())
    print("%s: max |delta| %.3g, samples %d, segments %d, oracle %d" % (name, d, samples, segments, ref_segments))
    assert samples == w * h * spp
    if name == "rects":
        assert d < TIGHT and segments == ref_segments and segments >= 2 * samples
    else:
        assert_parity(orc, whole, types.SimpleNamespace(samples=samples, segments=segments), ref, ref_segments, w, h, spp, False)


# test_gpu_pretrace's frames: 64x40x70 as it stands (40 tiles x 5 chunks); 36x20x48 has 15 tiles x 4 chunks = 60 items,
# short of the 64 that two blocks ask for, so it is 44x20x48 here (18 x 4 = 72; still cut by the right and the bottom edge)
PRETRACE_FRAMES = [(44, 20, 48), (64, 40, 70)]


@pytest.mark.parametrize("camera_name", sorted(CAMERAS))
@pytest.mark.parametrize("w,h,spp", PRETRACE_FRAMES, ids=["%dx%dx%d" % f for f in PRETRACE_FRAMES])
def test_pretrace_cameras_with_succession(rt, orc, gpu, w, h, spp, camera_name):
    """The rects-only plain variant through test_gpu_pretrace's four cameras — a mix, only misses (every item culled or
    ended in its batches), only the light, only walls (the ring always full): ring_head, ring_level, batch_below and
    the rect mask are per item, and here a wave sets them up many times over.  The bar is test_gpu_pretrace._check's."""
    bundle, cam, tm = CAMERAS[camera_name]()
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, spp)
    got = {}
    for cap in (0,) + B_CAPS:
        scene = rt.Scene(bundle, launch_blocks=cap)
        try:
            v = scene.variant()
            assert (v["prims_class"], v["textured"], v["specular"], v["use_bvh"], v["exact"]) == (V.RECTS, 0, 0, 0, 0)
            frame = scene.render_frame(camera, params)
            if cap:
                _assert_capped(scene, cap, camera_name)
            else:
                _assert_uncapped(scene, B_CAPS, camera_name)
            stats = scene.last_stats()
            got[cap] = (frame, int(stats.samples), int(stats.segments))
        finally:
            scene.close()
    _assert_same_bits(got, B_CAPS)
    whole, samples, segments = got[0]
    ref, ref_segments = orc.render(bundle.desc, camera, params)
    kind = {"None": orc.ORC_TM_NONE, "Aces": orc.ORC_TM_ACES}[tm]
    _assert_parity(orc.tone_map(kind, ref), orc.tone_map(kind, whole))
    assert samples == w * h * spp
    assert abs(segments - ref_segments) <= max(4, ref_segments // 100000)


PREVIEW = (263, 107, 10, 5, 4)   # test_gpu_preview's 103x47 with tiles 10x5 and scale 4 has a grid of 51 x 15 cells: 14 items.
                                 # 263x107 keeps its steps (2 across, 3 down) and its uncovered edge: 131 x 35 cells, 85 items


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_the_preview_scale_with_succession(rt, orc, gpu, name):
    """RtRenderParams.scale: step_x, step_y > 1 in the item's pixel set-up, the two-pass resolve that fills the blocks, and
    the tile stream of the scaled frame.  test_gpu_preview's bar."""
    w, h, tw, th, scale = PREVIEW
    bundle, cam, _, use_bvh = _loop_scene(name)
    camera = S.camera_for(cam, w, h)
    params = abi.render_params(w, h, 5, max_depth=10, tiles_w=tw, tiles_h=th, scale=scale)
    got = {}
    for cap in (0,) + B_CAPS:
        scene = _open(rt, name, cap)
        try:
            frame = scene.render_frame(camera, params)
            if cap:
                _assert_capped(scene, cap, name)
            else:
                _assert_uncapped(scene, B_CAPS, name)
            stats = scene.last_stats()
            tiles = scene.render_tiles(camera, params)
            if cap:
                _assert_capped(scene, cap, name + " tiles")
            stitched = np.zeros_like(frame)
            for r, c, tw_, th_, arr in tiles:
                stitched[r:r + th_, c:c + tw_] = arr
            assert _bits_equal(stitched, frame), cap
            got[cap] = (frame, int(stats.samples), int(stats.segments))
        finally:
            scene.close()
    _assert_same_bits(got, B_CAPS)
    whole, _, segments = got[0]
    ref, ref_segments = orc.render(bundle.desc, camera, params, use_bvh=use_bvh)
    d = np.abs(ref - whole)
    assert d.max() < 1e-3 and float((d.max(axis=-1) > 1e-9).mean()) < 2e-3
    assert np.array_equal(ref == 0, whole == 0)                     # the uncovered edge stays black on both sides
    assert abs(segments - ref_segments) <= 4


@pytest.mark.parametrize("closest_hit", ["linear", "bvh"])
def test_lens_and_moving_sphere_tables_with_succession(rt, orc, gpu, closest_hit):
    """test_gpu_variants' lds_scene(ANY, 0) through its lens camera at 48x27x24 (24 tiles x 3 chunks = 72 items): the
    lens-disk samples and the ray times of the camera batches live in per-wave LDS tables that every item fills again, and
    with two items in flight the tables of the next item are drawn while the last paths of the old one still read theirs.
    test_gpu_variants' bar for this scene (assert_parity, fast arithmetic)."""
    w, h, spp = 48, 27, A_SPP
    bundle = lds_scene(V.ANY, 0)
    camera, params = S.camera_for(LENS_CAM, w, h), abi.render_params(w, h, spp, max_depth=V.DEPTH)
    got = {}
    for cap in (0,) + B_CAPS:
        scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if closest_hit == "bvh" else abi.RT_HIT_LINEAR, launch_blocks=cap)
        try:
            v = scene.variant()
            assert (v["prims_class"], v["textured"], v["use_bvh"], v["has_moving"], v["exact"]) == \
                (V.ANY, 1, int(closest_hit == "bvh"), 1, 0)
            frame = scene.render_frame(camera, params)
            if cap:
                _assert_capped(scene, cap, closest_hit)
            else:
                _assert_uncapped(scene, B_CAPS, closest_hit)
            got[cap] = (frame, scene.last_stats())
        finally:
            scene.close()
    whole, stats = got[0]
    _assert_same_bits({cap: (f, int(st.samples), int(st.segments)) for cap, (f, st) in got.items()}, B_CAPS)
    ref, ref_segments = orc.render(bundle.desc, camera, params)
    assert_parity(orc, whole, stats, ref, ref_segments, w, h, spp, False)


# ---- c. the delivering launch -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_box_boxes", "bvh"])
def test_the_delivering_launch_with_succession(rt, gpu, name):
    """rt_render's tile stream with a 7x3 and a 1x1 grid at 160x90x24 (240 tiles x 3 chunks): with a cap the three chunks
    of a tile land one after another through the same few waves, and the wave that lands the last one resolves the tile
    (rt_pool_deliver.h).  Stitched tiles = the capped frame = the uncapped frame, bit for bit."""
    w, h, spp = 160, 90, A_SPP
    if name == "bvh":
        bundle, cam, options, _ = _loop_scene("bvh")
    else:
        (bundle, cam, _), options = S.cornell_box_boxes(), {}
    camera = S.camera_for(cam, w, h)
    frames = {}
    for cap in (0,) + B_CAPS:
        scene = rt.Scene(bundle, launch_blocks=cap, **options)
        try:
            v = scene.variant()
            assert (v["prims_class"], v["use_bvh"], v["exact"]) == (V.ANY, int(name == "bvh"), 0)
            frames[cap] = scene.render_frame(camera, abi.render_params(w, h, spp))
            if cap:
                _assert_capped(scene, cap, name)
            else:
                _assert_uncapped(scene, B_CAPS, name)
            for tw, th in ((7, 3), (1, 1)):
                tiles = scene.render_tiles(camera, abi.render_params(w, h, spp, tiles_w=tw, tiles_h=th))
                if cap:
                    _assert_capped(scene, cap, "%s %dx%d tiles" % (name, tw, th))
                assert len(tiles) == tw * th
                stitched = np.full_like(frames[cap], -1.0)
                for r, c, tw_, th_, arr in tiles:
                    stitched[r:r + th_, c:c + tw_] = arr
                assert _bits_equal(stitched, frames[cap]), (cap, tw, th)
        finally:
            scene.close()
    assert frames[0].std() > 0.05
    for cap in B_CAPS:
        assert _bits_equal(frames[cap], frames[0]), cap


# ---- d. passes ----------------------------------------------------------------------------------------------------------

PASS_CASES = [(name, "fast") for name in sorted(LOOPS)] + [("any_ts", "exact")]


def _pass_case(name):
    """-> (bundle, camera dict, Scene options without cap and flavour)"""
    if name == "any_ts":    # the RT_ARITH_REFERENCE case of test_gpu_progressive / test_gpu_adaptive
        bundle, cam = V.build((V.ANY, 1, 1, 0))
        return bundle, cam, dict(closest_hit=abi.RT_HIT_LINEAR)
    return _loop_scene(name)[:3]


@pytest.mark.parametrize("name,flavour", PASS_CASES, ids=["%s-%s" % c for c in PASS_CASES])
def test_progressive_and_adaptive_passes_with_succession(rt, gpu, name, flavour):
    """rt_render_progressive's passes and rt_render_adaptive's tile-list launches (threshold off: every tile in every
    list) at 64x36x96 through ONE block: a pass of one chunk is a launch of 40 items for four waves.  The identities are
    test_gpu_progressive's and test_gpu_adaptive's own, run with launch_blocks = 1; the capped one-shot frame they compare
    with equals the uncapped one."""
    bundle, cam, options = _pass_case(name)
    options = dict(options, **_flavour_options(flavour))
    camera, params = S.camera_for(cam, V.W, V.H), abi.render_params(V.W, V.H, 96, max_depth=V.DEPTH)
    scene = rt.Scene(bundle, launch_blocks=1, **options)
    try:
        assert scene.variant()["exact"] == int(flavour == "exact")
        frames = scene.render_progressive(camera, params, 1)
        _assert_capped(scene, 1, name + " progressive")
        frame, samples, _, _ = scene.render_adaptive(camera, params, threshold=0.0, pass_samples=1)
        _assert_capped(scene, 1, name + " adaptive")
        capped = scene.render_frame(camera, params)
        _assert_capped(scene, 1, name + " one-shot")
    finally:
        scene.close()
    scene = rt.Scene(bundle, **options)
    try:
        whole = scene.render_frame(camera, params)
        _assert_uncapped(scene, (1,), name)
    finally:
        scene.close()
    assert _bits_equal(capped, whole) and _bits_equal(frames[-1][1], whole) and _bits_equal(frame, whole)
    assert (samples == 96).all()
    _assert_last_is_one_shot(rt, bundle, camera, params, (1, 30), launch_blocks=1, **options)
    _assert_threshold_off_is_one_shot(rt, bundle, camera, params, launch_blocks=1, **options)


# test_gpu_adaptive's scenes and pass lengths.  Its frames (64x48, 37x29, 2x2) have 48, 20 and 1 tiles, and a tile-list
# launch holds only the tiles that still run: the last launch of a call falls short of 32 items.  The frames here are
# larger (192 and 80 tiles, 75x61 keeping the odd edges of 37x29); the 2x2 frame is one tile, which no size-preserving
# change brings to several items per wave: enlarged it is the first case.
ADAPTIVE_CASES = [(S.three_balls, 128, 96, 1), (S.three_balls, 75, 61, 64), (S.cornell_box_boxes, 128, 96, 64),
                  (S.cornell_box_boxes, 75, 61, 1)]


@pytest.mark.parametrize("scene_fn,w,h,pass_samples", ADAPTIVE_CASES,
                         ids=["%s-%dx%d-p%d" % (c[0].__name__, c[1], c[2], c[3]) for c in ADAPTIVE_CASES])
def test_an_intermediate_threshold_with_succession(rt, gpu, scene_fn, w, h, pass_samples):
    """rt_render_adaptive with test_gpu_adaptive's threshold (the 30th percentile of the tiles' final errors): launches over
    shrinking tile lists, n_list x chunks items each.  The capped call against the scene's own uncapped call: frame, sample
    counts, tile errors and every callback's frame, bit for bit."""
    bundle, cam, _ = scene_fn()
    n = 256
    camera, params = S.camera_for(cam, w, h), abi.render_params(w, h, n, seed=9)
    got = {}
    thr = None
    for cap in (0, 1):
        scene = rt.Scene(bundle, launch_blocks=cap)
        try:
            if thr is None:
                prog_list = scene.render_progressive(camera, params, 1)
                bounds = [d for d, _ in prog_list]
                S_all, Q_all = M.sums_at_boundaries([f for _, f in prog_list], bounds)
                thr = float(np.quantile(M.tile_errors(S_all[-1], Q_all[-1], n, len(bounds)), 0.3))
            got[cap] = scene.render_adaptive(camera, params, threshold=thr, pass_samples=pass_samples)
            if cap:
                _assert_capped(scene, cap, "%s %dx%d p%d" % (scene_fn.__name__, w, h, pass_samples))
            got[cap] += (scene.last_stats(),)
        finally:
            scene.close()
    (frame, samples, err, frames, st), (c_frame, c_samples, c_err, c_frames, c_st) = got[0], got[1]
    tiles = samples[::8, ::8]
    assert tiles.min() < n and tiles.max() == n           # some tile stops early, another runs to the end: lists shrink
    assert _bits_equal(c_frame, frame) and np.array_equal(c_samples, samples) and _bits_equal(c_err, err)
    assert [d for d, _ in c_frames] == [d for d, _ in frames] and len(frames) >= 2
    for (done, a), (_, b) in zip(c_frames, frames):
        assert _bits_equal(a, b), done
    assert (c_st.samples, c_st.segments, c_st.kernel_launches) == (st.samples, st.segments, st.kernel_launches)


# ---- e. the NEE stream ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("closest_hit", ["linear", "bvh"])
@pytest.mark.parametrize("lights", ["plain", "extended"])
def test_the_nee_stream_with_succession(rt, gpu, lights, closest_hit):
    """k_nee_stream_f64 and k_nee_lights_stream_f64 draw ONE item per tile from the same queue: 72x64 is 72 tiles, which one
    and two blocks take 18 and 9 to a wave.  test_gpu_nee_stream's identity under the cap — the stream equals the
    one-shot frame equals rt_render_ex's tile sequence — and the capped stream equals the uncapped one-shot frame."""
    w, h, spp = 72, 64, 40
    bundle, cam = NM.mixed_scene(abi)
    c = S.camera_for(cam, w, h)
    p = abi.render_params(w, h, spp, max_depth=10, tiles_w=3, tiles_h=2, seed=7)

    def open_scene(cap):
        scene = rt.Scene(bundle, closest_hit=abi.RT_HIT_BVH if closest_hit == "bvh" else abi.RT_HIT_LINEAR, launch_blocks=cap)
        if lights == "extended":     # the moving emitter joins the list and the pick is by power: the extended-light kernels
            listed = len(scene.lights())
            scene.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_POWER)
            assert len(scene.lights()) > listed
        return scene

    scene = open_scene(0)
    try:
        assert scene.variant()["use_bvh"] == int(closest_hit == "bvh")
        want = scene.render_frame_nee(c, p)
        frame, _ = scene.render_tiles_nee(c, p)
        _assert_uncapped(scene, B_CAPS, "%s %s" % (lights, closest_hit))
        assert _bits_equal(frame, want) and want.std() > 0.05
    finally:
        scene.close()
    for cap in B_CAPS:
        scene = open_scene(cap)
        try:
            frame, order = scene.render_tiles_nee(c, p)
            _assert_capped(scene, cap, "%s %s" % (lights, closest_hit))
            assert len(order) == 6 and _bits_equal(frame, want), cap
            assert _bits_equal(_check_stream(scene, c, p), want), cap
        finally:
            scene.close()
