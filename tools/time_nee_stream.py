"""Cost of rt_render_nee on one MI355X, at the scenes' own 1080p size (config_c3.yml), 256 and 1024 spp,
host clock around the whole call, the median of 3 timed calls after a warm-up:

  * one-shot rt_render_frame_nee beside the streamed frame with the 10x10 grid (a cancel hook armed that never fires, as the
    reference's callers always pass one) and the time to the first tile callback;
  * the time from raising the hook, in the middle of the frame, to the call's return;
  * the chunk length the library was built with (rtdev_nee_stream_chunk).

    python tools/time_nee_stream.py [--out profiles/nee_stream.json] [--scenes a,b] [--one-shot-only] [--tag NAME]
                                    [--library-note TEXT]

--one-shot-only times rt_render_frame_nee alone and needs nothing newer than it: with RACER_TRACER_AMD_LIB pointing at a
library built from an older commit it gives the baseline of the same machine and session.  --tag names the row set in the
output file (rows of other tags already in the file are kept), e.g. a build with another -DRT_NEE_STREAM_CHUNK.
--library-note goes into every row beside the library's path: what that library was built from.
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
NEW = ("rt_render_nee",)
NEW_DEV = ("rtdev_nee_stream_chunk", "rtdev_nee_stream_chunk_exact")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nee_stream.json"))
    ap.add_argument("--scenes", default="cornell_box,cornell_box_boxes,emissive")
    ap.add_argument("--spp", default="256,1024")
    ap.add_argument("--one-shot-only", action="store_true")
    ap.add_argument("--tag", default="this_build")
    ap.add_argument("--library-note", default="")
    args = ap.parse_args()
    if args.one_shot_only:
        for name in NEW:
            rt.abi.PROTOTYPES.pop(name, None)
        for name in NEW_DEV:
            rt.abi.DEV_PROTOTYPES.pop(name, None)
    if rt.device_count() < 1:
        raise SystemExit("time_nee_stream.py needs a GPU")
    rows = {}
    for name in args.scenes.split(","):
        session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", name + ".yml"))
        scene = rt.Scene(session)
        cam, p = session.camera, session.params
        for n in [int(x) for x in args.spp.split(",")]:
            p.samples, p.seed = n, 1
            row = {"width": p.width, "height": p.height, "samples": n, "library": os.path.relpath(rt.LIB_PATH, ROOT)}
            if args.library_note:
                row["library_note"] = args.library_note
            row["one_shot_ms"], one_shot = timed(lambda: scene.render_frame_nee(cam, p))
            if not args.one_shot_only:
                row["chunk"] = rt.nee_stream_chunk()
                first = []

                def stream():
                    t0 = time.perf_counter()
                    del first[:]
                    return scene.render_tiles_nee(cam, p, cancel=lambda: False,
                                                  on_tile=lambda *t: first or first.append((time.perf_counter() - t0) * 1e3))

                firsts = []
                ts = []
                stream()
                for _ in range(3):
                    t0 = time.perf_counter()
                    frame, order = stream()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    firsts.append(first[0])
                row["stream_ms"], row["first_tile_ms"] = statistics.median(ts), statistics.median(firsts)
                row["stream_kernel_ms"] = scene.last_stats().kernel_ms
                row["stream_equals_one_shot"] = bool(np.array_equal(frame, one_shot))
                row["stream_over_one_shot_percent"] = 100.0 * (row["stream_ms"] - row["one_shot_ms"]) / row["one_shot_ms"]
                lat = []
                for _ in range(3):  # the hook rises 45 % into the frame
                    t0 = time.perf_counter()
                    raise_at = t0 + 0.45 * row["stream_ms"] / 1e3
                    raised = []

                    def cancel():
                        if time.perf_counter() < raise_at:
                            return False
                        if not raised:
                            raised.append(time.perf_counter())
                        return True

                    _, order = scene.render_tiles_nee(cam, p, cancel=cancel)
                    lat.append((time.perf_counter() - raised[0]) * 1e3)
                    row["tiles_before_cancel"] = len(order)
                row["cancel_to_return_ms"] = statistics.median(lat)
                row["after_cancel_equals_one_shot"] = bool(np.array_equal(scene.render_tiles_nee(cam, p)[0], one_shot))
            rows["%s@%d" % (name, n)] = row
            print(args.tag, name, n, json.dumps(row), flush=True)
        scene.close()
        session.close()
    results = {}
    if os.path.exists(args.out):
        results = json.load(open(args.out))
    results[args.tag] = rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
