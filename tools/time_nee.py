"""Cost and benefit of rt_render_frame_nee on one MI355X, at the scenes' own 1080p size (config_c3.yml):

  * ms per frame, plain (rt_render_frame) and NEE, at 256 and 1024 spp: the median of 3 timed calls after a warm-up,
    host clock around the whole call (the frame is in host memory when it returns);
  * gamma RMSE against a 16384-spp plain frame at another seed, for plain at 1024 spp and for NEE at the sample count
    that takes the same time (1024 * t_plain / t_nee, rounded to a multiple of 4).

    python tools/time_nee.py [--out profiles/nee_timings.json] [--scenes cornell_box,cornell_box_boxes,emissive]
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


def timed(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nee_timings.json"))
    ap.add_argument("--scenes", default="cornell_box,cornell_box_boxes,emissive")
    args = ap.parse_args()
    if rt.device_count() < 1:
        raise SystemExit("time_nee.py needs a GPU")
    results = {}
    for name in args.scenes.split(","):
        session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", name + ".yml"))
        scene = rt.Scene(session)
        cam, p = session.camera, session.params
        row = {"width": p.width, "height": p.height}

        def frame(fn, spp, seed):
            p.samples, p.seed = spp, seed
            return fn(cam, p)

        for spp in (256, 1024):
            row["plain_ms_%d" % spp], _ = timed(lambda: frame(scene.render_frame, spp, 1))
            row["nee_ms_%d" % spp], _ = timed(lambda: frame(scene.render_frame_nee, spp, 1))
            row["nee_cost_per_sample_%d" % spp] = row["nee_ms_%d" % spp] / row["plain_ms_%d" % spp]
        ref = frame(scene.render_frame, 16384, 12345)
        rmse = lambda f: float(np.sqrt(np.mean((f - ref) ** 2)))  # noqa: E731
        row["plain_rmse_1024"] = rmse(frame(scene.render_frame, 1024, 1))
        equal = max(4, int(round(1024 * row["plain_ms_1024"] / row["nee_ms_1024"] / 4.0)) * 4)
        row["nee_equal_time_spp"] = equal
        row["nee_equal_time_ms"], f = timed(lambda: frame(scene.render_frame_nee, equal, 1), reps=1)
        row["nee_rmse_equal_time"] = rmse(f)
        row["nee_rmse_1024"] = rmse(frame(scene.render_frame_nee, 1024, 1))
        scene.close()
        session.close()
        results[name] = row
        print(name, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
