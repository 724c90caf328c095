"""Cost and benefit of rt_scene_set_lights ("the extended list") on one MI355X, at 1920x1080 (config_c3.yml):
every time is the median of 3 timed calls after a warm-up, host clock around the whole call.

  * lights/cornell_box_lamp (lit by a Box inside RotateY + Translate): ms at 256 and 1024 spp for the plain frame, NEE with the
    default list (the lamp unlisted) and NEE with RT_LIGHTS_ALL; their gamma RMSE against a 16384-spp plain frame at another
    seed; and the RMSE of NEE with ALL at the sample count that takes the plain frame's time at 1024 spp.
  * cornell_box_boxes with RT_PICK_POWER: its one plain light gives the same samples through the extended kernel, so the
    difference to rt_render_frame_nee with the default list — measured here, and with --parent-lib on the library of the
    commit before — is what the extended code costs when it buys nothing.  With the default list the same scene is also
    timed through rt_render_nee and rt_render_progressive_nee (pass_samples 256), on both libraries, and the frames are
    compared bit for bit: the stream and pass kernels share their bodies with the extended ones since this list exists.

    python tools/time_nee_lights.py [--out profiles/nee_lights_timings.json] [--parent-lib path/to/libracer_tracer_amd.so]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rt = importlib.import_module("racer-tracer_amd")
host = importlib.import_module("racer-tracer_amd.host")
abi = rt.abi


def timed(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def other_roads(scene, frame, row, prefix):
    """The kernels behind rt_render_nee (k_nee_stream_f64) and rt_render_progressive_nee (k_nee_pass_f64), default list, at
    1024 spp (the stream at 256 too): ms into row[prefix + ...] -> (stream frame, last progressive frame)."""
    for spp in (256, 1024):
        row["%sstream_ms_%d" % (prefix, spp)], tiles = timed(lambda: frame(lambda c, p: scene.render_tiles_nee(c, p)[0], spp, 1))
    row["%sprogressive_ms_1024" % prefix], last = timed(lambda: frame(lambda c, p: scene.render_progressive_nee(c, p, 256)[-1][1], 1024, 1))
    return tiles, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nee_lights_timings.json"))
    ap.add_argument("--parent-lib", default=None, help="the library of the parent commit, for the cost comparison")
    args = ap.parse_args()
    if rt.device_count() < 1:
        raise SystemExit("time_nee_lights.py needs a GPU")
    results = {}

    def open_scene(name, library=None):
        session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", *name.split("/")) + ".yml")
        return session, rt.Scene(session, library=library)

    # ---- what listing the lamp buys
    session, scene = open_scene("lights/cornell_box_lamp")
    cam, p = session.camera, session.params
    row = {"width": p.width, "height": p.height}

    def frame(fn, spp, seed):
        p.samples, p.seed = spp, seed
        return fn(cam, p)

    ref = frame(scene.render_frame, 16384, 12345)
    rmse = lambda f: float(np.sqrt(np.mean((f - ref) ** 2)))  # noqa: E731
    for spp in (256, 1024):
        scene.set_lights()
        row["plain_ms_%d" % spp], f = timed(lambda: frame(scene.render_frame, spp, 1))
        row["plain_rmse_%d" % spp] = rmse(f)
        row["nee_default_ms_%d" % spp], f = timed(lambda: frame(scene.render_frame_nee, spp, 1))
        row["nee_default_rmse_%d" % spp] = rmse(f)
        scene.set_lights(abi.RT_LIGHTS_ALL, abi.RT_PICK_UNIFORM)
        row["lights"] = scene.lights()
        row["nee_all_ms_%d" % spp], f = timed(lambda: frame(scene.render_frame_nee, spp, 1))
        row["nee_all_rmse_%d" % spp] = rmse(f)
    equal = max(4, int(round(1024 * row["plain_ms_1024"] / row["nee_all_ms_1024"] / 4.0)) * 4)
    row["nee_all_equal_time_spp"] = equal
    row["nee_all_equal_time_ms"], f = timed(lambda: frame(scene.render_frame_nee, equal, 1))
    row["nee_all_rmse_equal_time"] = rmse(f)
    scene.close()
    session.close()
    results["cornell_box_lamp"] = row
    print("cornell_box_lamp", json.dumps(row), flush=True)

    # ---- what the extended code costs when it buys nothing
    session, scene = open_scene("cornell_box_boxes")
    cam, p = session.camera, session.params
    row = {"width": p.width, "height": p.height}
    for spp in (256, 1024):
        scene.set_lights()
        row["nee_default_ms_%d" % spp], a = timed(lambda: frame(scene.render_frame_nee, spp, 1))
        scene.set_lights(abi.RT_LIGHTS_PLAIN, abi.RT_PICK_POWER)
        row["nee_power_pick_ms_%d" % spp], b = timed(lambda: frame(scene.render_frame_nee, spp, 1))
        row["max_abs_difference_%d" % spp] = float(np.abs(a - b).max())
    scene.set_lights()
    tree = other_roads(scene, frame, row, "")
    scene.close()
    session.close()
    if args.parent_lib:
        import ctypes as C
        rt.lib()   # the default library (and torch's HIP runtime) first
        parent = C.CDLL(args.parent_lib)   # (it has no rt_scene_set_lights: bind what it exports)
        for name, (res, argtypes) in list(abi.PROTOTYPES.items()) + list(abi.DEV_PROTOTYPES.items()):
            if hasattr(parent, name):
                getattr(parent, name).restype, getattr(parent, name).argtypes = res, argtypes
        session, scene = open_scene("cornell_box_boxes", library=parent)
        cam, p = session.camera, session.params
        for spp in (256, 1024):
            row["parent_nee_ms_%d" % spp], c = timed(lambda: frame(scene.render_frame_nee, spp, 1))
        row["parent_frame_equals_default_list_frame_1024"] = bool(np.array_equal(a, c))
        old = other_roads(scene, frame, row, "parent_")
        row["parent_stream_frame_equals_1024"] = bool(np.array_equal(tree[0], old[0]))
        row["parent_progressive_frame_equals_1024"] = bool(np.array_equal(tree[1], old[1]))
        row["stream_frame_equals_one_shot_1024"] = bool(np.array_equal(tree[0], a))
        scene.close()
        session.close()
    results["cornell_box_boxes"] = row
    print("cornell_box_boxes", json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
