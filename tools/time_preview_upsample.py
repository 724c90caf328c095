"""Cost of the preview upsampler on one MI355X -> profiles/preview_upsample_timings.json.

    python tools/time_preview_upsample.py --cost    # kernel times under a rocprofv3 kernel trace of its own
    python tools/time_preview_upsample.py --wall    # wall time of rt_render_preview_upsampled next to rt_render_frame

Both at the 1080p size of scenes/config_c3.yml on cornell_box with C3's camera, the config's preview block with tiles 10x10
and scale 4 (blocks of 4x4).

--cost: a child process (this file with --trace-run) runs under `rocprofv3 --kernel-trace`, no counters: seven times the
preview frame on the device, the full-resolution guides, the upsample and one a-trous level (rt_denoise_device with one
iteration).  The medians of the last six launches of k_upsample_preview, k_guides_f64 and k_denoise_atrous are reported side
by side.

--wall: in one process, after one call of each to warm up, the medians of six calls of rt_render_frame (the replicated
preview: today's route) and of rt_render_preview_upsampled (levels 0) with the same params, host frame to host frame.
"""
import argparse
import csv
import glob
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "preview_upsample_timings.json")
KERNELS = r"k_(upsample_preview|guides_f64|denoise_atrous)"


def save(section, rows):
    results = json.load(open(OUT)) if os.path.exists(OUT) else {}
    results[section] = rows
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(results, open(OUT, "w"), indent=1)


def _setup():
    rt = importlib.import_module("racer-tracer_amd")
    host = importlib.import_module("racer-tracer_amd.host")
    pv = importlib.import_module("racer-tracer_amd.preview")
    if rt.device_count() < 1:
        raise SystemExit("time_preview_upsample.py needs a GPU")
    session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", "cornell_box.yml"))
    p = session.preview_params
    p.tiles_w = p.tiles_h = 10
    p.scale = 4
    cam = host.camera_new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 0.0, 10000.0, p.width, p.height)
    return rt, pv, session, cam, p


def trace_run(reps=6):
    """The workload rocprofv3 traces: every kernel reps + 1 times at 1080p."""
    import ctypes as C
    import torch
    rt, pv, session, cam, p = _setup()
    abi = rt.abi
    scene = rt.Scene(session)
    h, w = p.height, p.width
    full = abi.render_params(w, h, p.samples, max_depth=p.max_depth, tiles_w=p.tiles_w, tiles_h=p.tiles_h, seed=p.seed)
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    guides = {"normal": torch.zeros((h, w, 3), **f64), "position": torch.zeros((h, w, 3), **f64),
              "albedo": torch.zeros((h, w, 3), **f64), "footprint": torch.zeros((h, w), **f64),
              "obj_id": torch.zeros((h, w), dtype=torch.int32, device=dev)}
    preview, up, dst = (torch.zeros((h, w, 3), **f64) for _ in range(3))
    g = rt.guides_struct(guides)
    one_level = rt.denoise_params(iterations=1)
    torch.cuda.synchronize(dev)
    for _ in range(reps + 1):
        scene.render_frame_device(cam, p, preview.data_ptr())
        rt.check(scene._lib.rt_render_guides_device(scene._h, C.byref(cam), C.byref(full), C.byref(g), None), "guides")
        pv.upsample_preview_device(scene, p, preview.data_ptr(), g, up.data_ptr())
        scene.denoise_device(full, up.data_ptr(), g, dst.data_ptr(), one_level)
        torch.cuda.synchronize(dev)
    scene.close()


def cost():
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
        us = [t for _, t in v][-6:]      # the first pass of the loop aside
        rows[name] = {"median_us": statistics.median(us), "launches": len(us)}
    print(json.dumps(rows), flush=True)
    save("kernels_1920x1080_scale4", rows)


def wall(reps=6):
    rt, pv, session, cam, p = _setup()
    scene = rt.Scene(session)
    routes = {"rt_render_frame": lambda: scene.render_frame(cam, p),
              "rt_render_preview_upsampled": lambda: pv.render_preview_upsampled(scene, cam, p)}
    rows = {"samples": p.samples, "max_depth": p.max_depth, "grid": list(pv.preview_grid(p))}
    for name, call in routes.items():
        call()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        rows[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "calls": reps}
    scene.close()
    print(json.dumps(rows), flush=True)
    save("wall_1920x1080_scale4", rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    args = ap.parse_args()
    if args.trace_run:
        trace_run()
    if args.cost:
        cost()
    if args.wall:
        wall()
