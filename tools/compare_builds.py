#!/usr/bin/env python3
"""Developer probe: do two builds of the library render bit-identical frames?
usage: tools/compare_builds.py <other .so> [spp] [fast|reference] [max |diff| that still counts as equal, default 0]
       tools/compare_builds.py <other .so> --entry-points
(the default build is the other side)

Without --entry-points: rt_render_frame (the pooled kernel) on the shipped scenes at 480x270.

--entry-points: the per-pixel kernels, through every entry point that launches them, on the small scenes of
tests/variant_scenes.py (every form, plain and light2=True; several have a lens) at 40x24 and 17x9, 6 spp, in both
arithmetics: the v1 kernel (rt_render_frame with RT_KERNEL_V1, and two strip shares through rt_render_frame_device), the
NEE kernels (rt_render_frame_nee, two strip shares through rt_render_frame_nee_strips_device, the last frame of
rt_render_progressive_nee at 2 samples a pass, the tiles of rt_render_nee), the same three after rt_scene_set_lights(all
kinds, pick by power) on the PRIMS_ANY forms, max_depth 0 and 1 on one form, and every plane of rt_render_guides_device
(fast arithmetic: its kernel has no other; it keeps no statistics, so the planes alone are compared).  Frames AND
rt_scene_last_stats' segments / samples must be equal; exits 1 otherwise."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rt = importlib.import_module("racer-tracer_amd")
host = importlib.import_module("racer-tracer_amd.host")
abi = rt.abi


def shipped_scenes(other, spp, arith, tol):
    bad = 0
    for scene_name in ("cornell_box.yml", "three_balls.yml", "noise_and_textures.yml", "emissive.yml", "clown.yml", "cornell_box_boxes.yml", "random"):
        path = scene_name if scene_name == "random" else os.path.join(ROOT, "scenes", scene_name)
        s = host.Session(os.path.join(ROOT, "scenes", "config_c2.yml"), scene=path)
        p = s.params
        p.width, p.height, p.samples = 480, 270, spp
        frames = []
        for lib in (None, other):
            sc = rt.Scene(s, library=lib, arithmetic=arith)
            frames.append(sc.render_frame(s.camera, p))
            sc.close()
        same = np.array_equal(frames[0], frames[1])
        bad += not same and not float(np.abs(frames[0] - frames[1]).max()) <= tol
        differ = int((np.abs(frames[0] - frames[1]).max(axis=-1) > 0).sum())
        print("%-24s %s  max |diff| %.3g  (%d of %d pixels differ)" % (scene_name, "bit-identical" if same else "DIFFERENT", float(np.abs(frames[0] - frames[1]).max()),
                                                                      differ, p.width * p.height))
    return bad


SHAPES = ((40, 24), (17, 9))  # 2.5 x 1.5 blocks of 16x16 and 5 x 3 tiles of 8x8; a partial block and partial tiles both ways
SPP = 6


def entry_points(other):
    """-> (cases, cases that differ).  A case is one call (or one pair of strip shares) in one build; its result is the
    frame (or the guide planes) and the segments / samples of rt_scene_last_stats."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nee_lights_scenes as LS
    import scenes_py as S
    import variant_scenes as V

    def stats(scene):
        st = scene.last_stats()
        return (int(st.segments), int(st.samples))

    def strips(scene, call, cam, w, h, depth):
        """Two shares of 8-row strips into one device frame: the second owned-row grid starts at image row 8."""
        out = torch.zeros((h, w, 3), dtype=torch.float64, device=torch.device("cuda", 0))
        seen = []
        for index in range(2):
            q = abi.render_params(w, h, SPP, max_depth=depth, strip_rows=8, strip_count=2, strip_index=index)
            call(scene)(cam, q, out.data_ptr())
            torch.cuda.synchronize()
            seen.append(stats(scene))
        return [out.cpu().numpy()], seen

    def frame_of(method, **kw):
        def run(scene, cam, p):
            got = getattr(scene, method)(cam, p, **kw)
            return [got], stats(scene)
        return run

    def last_pass(scene, cam, p):
        frames = scene.render_progressive_nee(cam, p, 2)
        assert frames[-1][0] == p.samples
        return [frames[-1][1]], stats(scene)

    def tiles(scene, cam, p):
        frame, order = scene.render_tiles_nee(cam, p)
        return [frame], (stats(scene), sorted(order))

    def guides(scene, cam, p):
        planes = scene.render_guides(cam, p)
        return [planes[k] for k in sorted(planes)], sorted(planes)

    nee_calls = (("nee", frame_of("render_frame_nee")), ("nee passes", last_pass), ("nee stream", tiles))
    cases = bad = 0

    def compare(what, make_scene, run):
        nonlocal cases, bad
        got = []
        for lib in (None, other):
            scene = make_scene(lib)
            try:
                got.append(run(scene))
            finally:
                scene.close()
        same = got[0][1] == got[1][1] and len(got[0][0]) == len(got[1][0]) and \
            all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[0][0], got[1][0]))
        cases += 1
        bad += not same
        if not same:
            print("DIFFERENT  %s: %s | %s" % (what, got[0][1], got[1][1]))

    for arith_name, arith in (("fast", abi.RT_ARITH_FAST), ("reference", abi.RT_ARITH_REFERENCE)):
        for form in V.SPECS:
            hit = abi.RT_HIT_BVH if form[3] else abi.RT_HIT_LINEAR
            for light2 in (False, True):
                bundle, cam_spec = V.build(form, light2=light2)
                name = "%s %s%s" % (arith_name, form, " light2" if light2 else "")
                # (every lambda below is called before its loop moves on; the defaults bind what it uses all the same)
                nee_scene = lambda lib, b=bundle, hit=hit, a=arith: rt.Scene(b, closest_hit=hit, arithmetic=a, library=lib)  # noqa: E731
                v1_scene = lambda lib, b=bundle, hit=hit, a=arith: rt.Scene(b, closest_hit=hit, arithmetic=a, kernel=abi.RT_KERNEL_V1, library=lib)  # noqa: E731
                first = form == (V.ANY, 0, 1, 0) and light2  # the form that also runs the depth and strip cases
                for w, h in SHAPES:
                    cam = S.camera_for(cam_spec, w, h)
                    for depth in ((V.DEPTH, 0, 1) if first and (w, h) == SHAPES[0] else (V.DEPTH,)):
                        p = abi.render_params(w, h, SPP, max_depth=depth)
                        p.tiles_w, p.tiles_h = 3, 2
                        at = "%s %dx%d depth %d" % (name, w, h, depth)
                        if not form[3]:  # k_trace_f64 has the linear loop only
                            compare("v1 " + at, v1_scene, lambda s, cam=cam, p=p: frame_of("render_frame")(s, cam, p))
                        for label, run in (nee_calls if depth == V.DEPTH else nee_calls[:1]):
                            compare(label + " " + at, nee_scene, lambda s, run=run, cam=cam, p=p: run(s, cam, p))
                    if first:
                        compare("v1 strips %s %dx%d" % (name, w, h), v1_scene,
                                lambda s, cam=cam, w=w, h=h: strips(s, lambda sc: sc.render_frame_device, cam, w, h, V.DEPTH))
                        compare("nee strips %s %dx%d" % (name, w, h), nee_scene,
                                lambda s, cam=cam, w=w, h=h: strips(s, lambda sc: sc.render_frame_nee_strips_device, cam, w, h, V.DEPTH))
            if form[0] == V.ANY:  # rt_scene_set_lights' list: box, wrapped and moving lights, picked by power
                bundle, cam_spec = LS.variant_case(form)

                def lights_scene(lib, bundle=bundle, hit=hit, arith=arith):
                    scene = rt.Scene(bundle, closest_hit=hit, arithmetic=arith, library=lib)
                    scene.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_POWER)
                    return scene
                for w, h in SHAPES:
                    cam = S.camera_for(cam_spec, w, h)
                    p = abi.render_params(w, h, SPP, max_depth=V.DEPTH)
                    p.tiles_w, p.tiles_h = 3, 2
                    for label, run in nee_calls:
                        compare("%s lights %s %s %dx%d" % (label, arith_name, form, w, h), lights_scene, lambda s, run=run, cam=cam, p=p: run(s, cam, p))
            if arith == abi.RT_ARITH_FAST and form in ((V.ANY, 1, 1, 0), (V.ANY, 1, 1, 1)):  # k_guides_f64 exists in the fast arithmetic only
                bundle, cam_spec = V.build(form)
                for w, h in SHAPES:
                    cam = S.camera_for(cam_spec, w, h)
                    p = abi.render_params(w, h, SPP, max_depth=V.DEPTH)
                    compare("guides %s %dx%d" % (form, w, h),
                            lambda lib, b=bundle, hit=hit: rt.Scene(b, closest_hit=hit, library=lib), lambda s, cam=cam, p=p: guides(s, cam, p))
    print("%d cases, %d differ" % (cases, bad))
    return bad


if __name__ == "__main__":
    other = rt.load_library(sys.argv[1])
    if len(sys.argv) > 2 and sys.argv[2] == "--entry-points":
        sys.exit(1 if entry_points(other) else 0)
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    arith = abi.RT_ARITH_REFERENCE if len(sys.argv) > 3 and sys.argv[3] == "reference" else abi.RT_ARITH_FAST
    sys.exit(1 if shipped_scenes(other, spp, arith, float(sys.argv[4]) if len(sys.argv) > 4 else 0.0) else 0)
