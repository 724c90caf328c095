"""Cost and benefit of rt_render_progressive_nee / rt_render_adaptive_nee on one MI355X, at the scenes' own
1080p size (config_c3.yml), N = 1024, host clock around the whole call, the median of 3 timed calls after a warm-up:

  * one-shot rt_render_frame_nee, progressive NEE in passes of 64 (nothing stops) and the overhead of the passes;
  * adaptive NEE at the default threshold: ms, the share of the samples traced and the gamma RMSE against a 16384-spp plain
    frame at another seed, beside a uniform NEE frame that takes the same time;
  * the time from raising cancel, in the middle of a pass, to the call's return.

    python tools/time_nee_progressive.py [--out profiles/nee_progressive.json] [--scenes a,b] [--one-shot-only]

--one-shot-only times rt_render_frame_nee alone and needs nothing newer than it: with RACER_TRACER_AMD_LIB pointing at a
library built from an older commit it gives the baseline of the same machine and session.
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
N = 1024


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nee_progressive.json"))
    ap.add_argument("--scenes", default="cornell_box,cornell_box_boxes,emissive")
    ap.add_argument("--one-shot-only", action="store_true")
    args = ap.parse_args()
    if args.one_shot_only:
        for name in ("rt_render_progressive_nee", "rt_render_adaptive_nee"):
            rt.abi.PROTOTYPES.pop(name, None)
    if rt.device_count() < 1:
        raise SystemExit("time_nee_progressive.py needs a GPU")
    results = {}
    for name in args.scenes.split(","):
        session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", name + ".yml"))
        scene = rt.Scene(session)
        cam, p = session.camera, session.params
        row = {"width": p.width, "height": p.height, "samples": N, "library": os.path.relpath(rt.LIB_PATH, ROOT)}

        def at(spp, seed):
            p.samples, p.seed = spp, seed
            return p

        row["one_shot_ms"], one_shot = timed(lambda: scene.render_frame_nee(cam, at(N, 1)))
        if not args.one_shot_only:
            row["progressive_ms"], frames = timed(lambda: scene.render_progressive_nee(cam, at(N, 1), 64))
            row["passes"] = len(frames)
            row["progressive_equals_one_shot"] = bool(np.array_equal(frames[-1][1], one_shot))
            row["overhead_ms"] = row["progressive_ms"] - row["one_shot_ms"]
            row["overhead_percent"] = 100.0 * row["overhead_ms"] / row["one_shot_ms"]
            st = scene.last_stats()
            row["progressive_kernel_ms"], row["progressive_resolve_ms"] = st.kernel_ms, st.resolve_ms
            row["adaptive_ms"], (frame, samples, _err, a_frames) = timed(lambda: scene.render_adaptive_nee(cam, at(N, 1)))
            row["adaptive_threshold"] = rt.adaptive_params().threshold
            row["adaptive_share_traced"] = float(samples.sum()) / (samples.size * N)
            row["adaptive_passes"] = len(a_frames)
            ref = scene.render_frame(cam, at(16384, 12345))
            rmse = lambda f: float(np.sqrt(np.mean((f - ref) ** 2)))  # noqa: E731
            row["adaptive_rmse"] = rmse(frame)
            row["one_shot_rmse"] = rmse(one_shot)
            equal = max(4, int(round(N * row["adaptive_ms"] / row["one_shot_ms"] / 4.0)) * 4)
            row["uniform_equal_time_spp"] = equal
            row["uniform_equal_time_ms"], f = timed(lambda: scene.render_frame_nee(cam, at(equal, 1)), reps=1)
            row["uniform_equal_time_rmse"] = rmse(f)
            # cancel raised about two and a half passes in, i.e. in the middle of pass 2 or 3
            lat = []
            for _ in range(3):
                t0 = time.perf_counter()
                raise_at = t0 + 2.5 * row["progressive_ms"] / row["passes"] / 1e3
                raised = []

                def cancel():
                    if time.perf_counter() < raise_at:
                        return False
                    if not raised:
                        raised.append(time.perf_counter())
                    return True

                scene.render_progressive_nee(cam, at(N, 1), 64, cancel=cancel)
                lat.append((time.perf_counter() - raised[0]) * 1e3)
            row["cancel_to_return_ms"] = statistics.median(lat)
            row["after_cancel_equals_one_shot"] = bool(np.array_equal(scene.render_frame_nee(cam, at(N, 1)), one_shot))
        scene.close()
        session.close()
        results[name] = row
        print(name, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
