"""What the several-share NEE calls cost on ONE MI355X, at the scenes' own 1080p size (config_c3.yml):

  * single: rt_render_frame_nee and rt_render_nee (10x10 grid), kernel_ms of rt_scene_last_stats, the best of 5 calls after a
    warm-up, with all five beside it, and a digest of the frame.  With --single-only and RACER_TRACER_AMD_LIB pointing at
    a library built from the parent commit this is the baseline of the same machine and session: run the two alternately,
    twice each, and the difference between the two runs of one library is the spread a difference has to beat.
  * shares: rt_render_frame_nee_multi with 1, 2 and 4 scenes on device 0: wall time of the call (best of 5) and the shares'
    kernel_ms summed.  NOT a scaling figure: the shares queue behind each other on one card.

    python tools/time_nee_multi.py [--out profiles/nee_multi_timings.json] [--tag NAME] [--single-only] [--spp 256]
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rt = importlib.import_module("racer-tracer_amd")
host = importlib.import_module("racer-tracer_amd.host")
NEW = ("rt_render_frame_nee_strips_device", "rt_render_frame_nee_multi", "rt_render_frame_nee_multi_device", "rt_render_nee_multi")


def kernel_ms(scene, call, reps=5):
    out = call()
    ms = []
    for _ in range(reps):
        out = call()
        ms.append(scene.last_stats().kernel_ms)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nee_multi_timings.json"))
    ap.add_argument("--scenes", default="cornell_box,cornell_box_boxes")
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--tag", default="this_build")
    ap.add_argument("--single-only", action="store_true")
    args = ap.parse_args()
    if args.single_only:
        for name in NEW:
            rt.abi.PROTOTYPES.pop(name, None)
    if rt.device_count() < 1:
        raise SystemExit("time_nee_multi.py needs a GPU")
    rows = {}
    for name in args.scenes.split(","):
        session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", name + ".yml"))
        cam, p = session.camera, session.params
        p.samples, p.seed, p.tiles_w, p.tiles_h = args.spp, 1, 10, 10
        scene = rt.Scene(session)
        row = {"width": p.width, "height": p.height, "samples": p.samples}
        ms, frame = kernel_ms(scene, lambda: scene.render_frame_nee(cam, p))
        row["frame_nee_kernel_ms"], row["frame_nee_kernel_ms_all"] = min(ms), ms
        row["frame_sha256"] = hashlib.sha256(frame.tobytes()).hexdigest()
        ms, streamed = kernel_ms(scene, lambda: scene.render_tiles_nee(cam, p)[0])
        row["render_nee_kernel_ms"], row["render_nee_kernel_ms_all"] = min(ms), ms
        row["stream_equals_frame"] = bool((streamed == frame).all())
        if not args.single_only:
            scenes = [scene] + [rt.Scene(session) for _ in range(3)]
            for n in (1, 2, 4):
                rt.render_frame_nee_multi(scenes[:n], cam, p)
                wall, summed = [], []
                for _ in range(5):
                    t0 = time.perf_counter()
                    got = rt.render_frame_nee_multi(scenes[:n], cam, p)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    summed.append(sum(s.last_stats().kernel_ms for s in scenes[:n]))
                row["shares_%d" % n] = {"wall_ms": min(wall), "wall_ms_all": wall, "summed_kernel_ms": min(summed),
                                        "equals_frame": bool((got == frame).all())}
            for s in scenes[1:]:
                s.close()
        rows[name] = row
        print(args.tag, name, json.dumps(row), flush=True)
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
