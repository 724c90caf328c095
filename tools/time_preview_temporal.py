"""Cost of the jittered preview accumulation on one MI355X -> profiles/preview_temporal.json, or the
file that --out names (a run of another library, RACER_TRACER_AMD_LIB, beside this tree's).

    python tools/time_preview_temporal.py --cost    # kernel times under a rocprofv3 kernel trace of its own
    python tools/time_preview_temporal.py --wall    # host clock of rt_render_preview_temporal beside the two calls it joins

Both at the 1080p size of scenes/config_c3.yml on cornell_box with C3's camera orbiting its look_at by 1 degree per call,
the config's preview block with tiles 10x10 and scale 4 (blocks of 4x4).

--cost: a child process (this file with --trace-run) runs under `rocprofv3 --kernel-trace`, no counters: seven times the
preview frame of the frame's phase camera on the device, the full-resolution guides of the unshifted camera,
rt_preview_accumulate_device into one of two histories, and on the same frame and guides rt_temporal_accumulate_device and
rt_upsample_preview_device.  The medians of the last six launches of k_preview_accumulate, k_temporal_accumulate and
k_upsample_preview are reported side by side, with the sum of the latter two: the new kernel reads what those two read
together, so that same-run sum is its yardstick.

--wall: in one process, after one call of each to warm up, six rounds of rt_render_preview_temporal,
rt_render_preview_upsampled and rt_render_temporal (full resolution at the preview's samples per pixel), one after the other
in every round, host frame to host frame; the medians.
"""
import argparse
import csv
import glob
import importlib
import json
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "preview_temporal.json")
KERNELS = r"k_(preview_accumulate|temporal_accumulate|upsample_preview)"
LOOK_FROM, LOOK_AT = (278.0, 278.0, -800.0), (278.0, 278.0, 0.0)


def save(section, rows, out):
    results = json.load(open(out)) if os.path.exists(out) else {}
    results[section] = rows
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(results, open(out, "w"), indent=1)


def _setup():
    rt = importlib.import_module("racer-tracer_amd")
    host = importlib.import_module("racer-tracer_amd.host")
    pv = importlib.import_module("racer-tracer_amd.preview")
    pt = importlib.import_module("racer-tracer_amd.preview_temporal")
    if rt.device_count() < 1:
        raise SystemExit("time_preview_temporal.py needs a GPU")
    session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", "cornell_box.yml"))
    p = session.preview_params
    p.tiles_w = p.tiles_h = 10
    p.scale = 4

    def camera(k):
        """C3's camera turned by k degrees about the vertical axis through its look_at."""
        a = math.radians(float(k))
        d = [LOOK_FROM[i] - LOOK_AT[i] for i in range(3)]
        r = (d[0] * math.cos(a) + d[2] * math.sin(a), d[1], -d[0] * math.sin(a) + d[2] * math.cos(a))
        return host.camera_new(tuple(LOOK_AT[i] + r[i] for i in range(3)), LOOK_AT, 40.0, 0.0, 10000.0, p.width, p.height)
    return rt, pv, pt, session, camera, p


def _full(rt, p):
    return rt.abi.render_params(p.width, p.height, p.samples, max_depth=p.max_depth, tiles_w=p.tiles_w, tiles_h=p.tiles_h, seed=p.seed)


def trace_run(reps=6):
    """The workload rocprofv3 traces: every kernel reps + 1 times at 1080p."""
    import ctypes as C
    import torch
    rt, pv, pt, session, camera, p = _setup()
    scene = rt.Scene(session)
    h, w = p.height, p.width
    full = _full(rt, p)
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)

    def history():
        return {"radiance": torch.zeros((h, w, 3), **f64), "moments": torch.zeros((h, w, 2), **f64),
                "length": torch.zeros((h, w), **f64), "normal": torch.zeros((h, w, 3), **f64),
                "position": torch.zeros((h, w, 3), **f64), "obj_id": torch.zeros((h, w), dtype=torch.int32, device=dev)}
    guides = {"normal": torch.zeros((h, w, 3), **f64), "position": torch.zeros((h, w, 3), **f64),
              "albedo": torch.zeros((h, w, 3), **f64), "footprint": torch.zeros((h, w), **f64),
              "obj_id": torch.zeros((h, w), dtype=torch.int32, device=dev)}
    preview, up = (torch.zeros((h, w, 3), **f64) for _ in range(2))
    hist, other = [history(), history()], history()
    g = rt.guides_struct(guides)
    torch.cuda.synchronize(dev)
    prev_cam = None
    for k in range(reps + 1):
        cam = camera(k)
        p.seed = session.preview_params.seed + k
        jx, jy = pt.phase(p, k)
        cur, old = hist[k & 1], hist[(k & 1) ^ 1]
        scene.render_frame_device(pt.phase_camera(cam, p, jx, jy), p, preview.data_ptr())
        rt.check(scene._lib.rt_render_guides_device(scene._h, C.byref(cam), C.byref(full), C.byref(g), None), "guides")
        prev = rt.history_struct(old) if prev_cam is not None else None
        pt.accumulate_device(scene, p, jx, jy, preview.data_ptr(), g, rt.history_struct(cur), prev_cam, prev)
        scene.temporal_accumulate_device(full, preview.data_ptr(), g, rt.history_struct(other), prev_cam, prev)
        pv.upsample_preview_device(scene, p, preview.data_ptr(), g, up.data_ptr())
        torch.cuda.synchronize(dev)
        prev_cam = cam
    scene.close()


def cost(out):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--trace-run"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if run.returncode != 0 or not found:
            raise SystemExit("rocprofv3 failed (%d): %s" % (run.returncode, run.stderr[-2000:]))
        spans = {}
        for row in csv.DictReader(open(found[0])):
            m = re.search(KERNELS, row["Kernel_Name"])
            if m:
                spans.setdefault(m.group(0), []).append((int(row["Start_Timestamp"]),
                                                         (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows = {}
    for name, v in sorted(spans.items()):
        v.sort()
        us = [t for _, t in v][-6:]      # the first pass of the loop (no previous history) aside
        rows[name] = {"median_us": statistics.median(us), "launches": len(us)}
    if "k_temporal_accumulate" in rows and "k_upsample_preview" in rows:
        rows["sum_of_the_two_it_joins_us"] = rows["k_temporal_accumulate"]["median_us"] + rows["k_upsample_preview"]["median_us"]
    print(json.dumps(rows), flush=True)
    save("kernels_1920x1080_scale4", rows, out)


def wall(out, reps=6):
    rt, pv, pt, session, camera, p = _setup()
    scene = rt.Scene(session)
    full = _full(rt, p)
    states = {name: rt.Temporal(p.width, p.height) for name in ("rt_render_preview_temporal", "rt_render_temporal")}
    seed = session.preview_params.seed

    def routes(k):
        cam = camera(k)
        p.seed = full.seed = seed + k
        return {"rt_render_preview_temporal": lambda: pt.render_preview_temporal(scene, states["rt_render_preview_temporal"], cam, p, k),
                "rt_render_preview_upsampled": lambda: pv.render_preview_upsampled(scene, cam, p),
                "rt_render_temporal": lambda: states["rt_render_temporal"].render(scene, cam, full)}
    rows = {"samples": p.samples, "max_depth": p.max_depth, "grid": list(pv.preview_grid(p))}
    ms = {name: [] for name in routes(0)}
    for k in range(reps + 1):       # round 0 warms every route up
        for name, call in routes(k).items():
            t0 = time.perf_counter()
            call()
            if k:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in ms.items():
        rows[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "calls": len(v)}
    for t in states.values():
        t.close()
    scene.close()
    print(json.dumps(rows), flush=True)
    save("wall_1920x1080_scale4", rows, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=OUT, help="the JSON file the results are merged into")
    args = ap.parse_args()
    if args.trace_run:
        trace_run()
    if args.cost:
        cost(args.out)
    if args.wall:
        wall(args.out)
