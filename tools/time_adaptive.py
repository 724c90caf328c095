#!/usr/bin/env python3
"""Times rt_render_adaptive on 1920x1080x1024 frames of cornell_box (C3) and three_balls against rt_render_frame and
rt_render_progressive with the same pass size, and measures what the samples it leaves out cost in error.

Per scene:
  * wall ms of rt_render_frame, rt_render_progressive(pass_samples), rt_render_adaptive(threshold 0, same pass size) — the
    overhead of the adaptive machinery when no tile stops — and rt_render_adaptive at the default threshold, with the
    fraction of the frame's samples it traced; calls alternate over the rounds, medians with the spread;
  * RMSE of the gamma-encoded frame against a 16384-spp frame at another seed, for the adaptive frame and for a uniform
    frame of about the same wall time (the spp that fraction of N rounds to, a multiple of 8).

    python tools/time_adaptive.py [--rounds 5] [--pass-samples 64] [--out profiles/r07_adaptive.txt]
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rt = importlib.import_module("racer-tracer_amd")
host = importlib.import_module("racer-tracer_amd.host")
abi = importlib.import_module("racer-tracer_amd.abi")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pass-samples", type=int, default=64)
    ap.add_argument("--reference-spp", type=int, default=16384)
    ap.add_argument("--scenes", default="cornell_box,three_balls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_adaptive.txt"))
    args = ap.parse_args()
    if rt.device_count() < 1:
        raise SystemExit("time_adaptive.py needs a GPU")
    defaults = rt.adaptive_params()
    ps = args.pass_samples
    lines = ["rt_render_adaptive, 1920x1080x1024, device 0, %d rounds, medians [min - max]; pass_samples %d, default threshold %g"
             % (args.rounds, ps, defaults.threshold), ""]

    def med(xs):
        return "%8.2f [%.2f - %.2f]" % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3)

    for name in args.scenes.split(","):
        session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", name + ".yml"))
        p, cam = session.params, session.camera
        w, h, n = p.width, p.height, p.samples
        scene = rt.Scene(session, device=0)
        lib = scene._lib
        out = np.ones((h, w, 3))
        out_ptr = out.ctypes.data_as(C.POINTER(C.c_double))
        counts = np.zeros((h, w), dtype=np.int32)
        errs = np.zeros(((h + 7) // 8, (w + 7) // 8))
        no_cancel = C.cast(None, abi.RtCancelCallback)
        no_frame = C.cast(None, abi.RtFrameCallback)
        cb = abi.RtFrameCallback(lambda *_: None)

        def frame(params=p):
            t0 = time.perf_counter()
            rt.check(lib.rt_render_frame(scene._h, C.byref(cam), C.byref(params), out_ptr), "rt_render_frame")
            return time.perf_counter() - t0

        def progressive():
            t0 = time.perf_counter()
            rt.check(lib.rt_render_progressive(scene._h, C.byref(cam), C.byref(p), ps, cb, None, no_cancel, None),
                     "rt_render_progressive")
            return time.perf_counter() - t0, scene.last_stats()

        def adaptive(threshold):
            a = rt.adaptive_params(threshold=threshold, pass_samples=ps)
            t0 = time.perf_counter()
            rt.check(lib.rt_render_adaptive(scene._h, C.byref(cam), C.byref(p), C.byref(a), out_ptr,
                                            counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                            errs.ctypes.data_as(C.POINTER(C.c_double)), no_frame, None, no_cancel, None),
                     "rt_render_adaptive")
            return time.perf_counter() - t0, scene.last_stats()

        frame()
        want = out.copy()
        adaptive(0.0)
        same = bool(np.array_equal(out, want))
        runs = {"frame": [], "progressive": [], "adaptive0": [], "adaptive": []}
        for _ in range(args.rounds):
            runs["frame"].append(frame())
            t, st_p = progressive()
            runs["progressive"].append(t)
            t, st0 = adaptive(0.0)
            runs["adaptive0"].append(t)
            t, st = adaptive(defaults.threshold)
            runs["adaptive"].append(t)
        adaptive_frame, adaptive_counts = out.copy(), counts.copy()
        frac = float(adaptive_counts.sum()) / (w * h * n)
        t_frame, t_prog = statistics.median(runs["frame"]), statistics.median(runs["progressive"])
        t_a0, t_a = statistics.median(runs["adaptive0"]), statistics.median(runs["adaptive"])
        lines.append("%s %dx%dx%d" % (name, w, h, n))
        lines.append("  rt_render_frame                      wall ms %s" % med(runs["frame"]))
        lines.append("  rt_render_progressive (pass %4d)     wall ms %s  %+5.1f %% vs rt_render_frame; trace ms %.2f, fold ms %.2f"
                     % (ps, med(runs["progressive"]), 100 * (t_prog / t_frame - 1), st_p.kernel_ms, st_p.resolve_ms))
        lines.append("  rt_render_adaptive threshold 0        wall ms %s  %+5.1f %% vs progressive; trace ms %.2f, fold ms %.2f; "
                     "frame == rt_render_frame's: %s" % (med(runs["adaptive0"]), 100 * (t_a0 / t_prog - 1), st0.kernel_ms,
                                                         st0.resolve_ms, same))
        lines.append("  rt_render_adaptive threshold %-8g wall ms %s  %+5.1f %% vs rt_render_frame; %.1f %% of the samples traced, "
                     "%d passes, trace ms %.2f, fold ms %.2f" % (defaults.threshold, med(runs["adaptive"]), 100 * (t_a / t_frame - 1),
                                                                 100 * frac, st.kernel_launches, st.kernel_ms, st.resolve_ms))
        hist = {int(b): float((adaptive_counts == b).mean()) for b in np.unique(adaptive_counts)}
        lines.append("  pixels by samples: " + ", ".join("%d: %.1f %%" % (b, 100 * f) for b, f in sorted(hist.items())))
        # error against a high-spp frame at another seed, next to a uniform frame of the adaptive frame's time
        ref_p = abi.render_params(w, h, args.reference_spp, max_depth=p.max_depth, seed=p.seed + 1000)
        frame(ref_p)
        ref = out.copy()
        n_eq = max(8, int(round(n * t_a / t_frame / 8.0)) * 8)
        eq_p = abi.render_params(w, h, n_eq, max_depth=p.max_depth, seed=p.seed)
        t_eq = statistics.median(frame(eq_p) for _ in range(3))
        uniform = out.copy()

        def rmse(x):
            return float(np.sqrt(np.mean((x - ref) ** 2)))

        lines.append("  RMSE vs %d spp (seed +1000): adaptive %.5f (%.2f ms) | uniform %d spp %.5f (%.2f ms) | uniform %d spp %.5f"
                     % (args.reference_spp, rmse(adaptive_frame), t_a * 1e3, n_eq, rmse(uniform), t_eq * 1e3, n, rmse(want)))
        lines.append("")
        scene.close()
        print("\n".join(lines[-7:]), flush=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
