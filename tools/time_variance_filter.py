"""Quality and cost of the variance-guided filter of a still frame -> profiles/variance_filter.json.

    python tools/time_variance_filter.py --quality     # CPU only: the numpy model on oracle frames, and the sweep of the defaults
    python tools/time_variance_filter.py --cost        # one MI355X: kernel times under a rocprofv3 kernel trace

--quality: cornell_box_boxes and three_balls at 128x128 against a 2048-spp oracle frame, with oracle guides.  For every
N in 4, 8, 16, 32, 48, 64, 96, 256 the chunks of chunk_plan(N) are rendered as oracle frames of their own (independent seeds),
which gives the running sums S and Q = sum_j S_j^2 / n_j the adaptive renderer would hold.  Reported: the gamma RMSE of the raw
frame, of the spatial filter (denoise_model), of the variance-guided levels under the 7x7 spatial variance alone
(min_chunks above every k) and under the batch variance, the latter for sigma_luminance in 1, 2, 4, 8 and min_chunks in
2, 3, 4.

--cost: at the 1080p size of scenes/config_c3.yml on cornell_box, C3's camera.  A child process (this file with --trace-run)
runs under `rocprofv3 --kernel-trace`, no counters: seven times an accumulation and rt_denoise_history_device (for
k_temporal_accumulate and k_temporal_variance) and rt_batch_variance_device on the sums of a 48-spp adaptive frame; the
medians of the last six launches of each kernel are reported side by side.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "variance_filter.json")
SPPS = (4, 8, 16, 32, 48, 64, 96, 256)
SIGMAS = (1.0, 2.0, 4.0, 8.0)
MIN_CHUNKS = (2, 3, 4)


def save(section, rows):
    results = json.load(open(OUT)) if os.path.exists(OUT) else {}
    results[section] = rows
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(results, open(OUT, "w"), indent=1)


# ---- quality on the model -------------------------------------------------------------------------------------------------

def quality(size=128, truth_spp=2048):
    import numpy as np
    import denoise_model as M
    import scenes_py as S
    import variance_filter_model as VF
    from oracle import oracle_ctypes as orc
    rt = importlib.import_module("racer-tracer_amd")
    abi = S.abi
    dparams = M.params_kwargs(rt.denoise_params())
    results = {"size": size, "truth_spp": truth_spp, "defaults": VF.DEFAULTS, "scenes": {}}
    for name, make in (("cornell_box_boxes", S.cornell_box_boxes), ("three_balls", S.three_balls)):
        bundle, cam = make()[:2]
        camera = S.camera_for(cam, size, size)
        guides = M.oracle_guides(orc, bundle, camera, size, size)
        truth = orc.render(bundle.desc, camera, abi.render_params(size, size, truth_spp, seed=99))[0]
        print("%s: guides and the %d-spp frame are made" % (name, truth_spp), flush=True)
        rows = {}
        for n in SPPS:
            bounds = rt.progressive_passes(n, 1)
            counts = [b - a for a, b in zip([0] + bounds[:-1], bounds)]
            means = [orc.render(bundle.desc, camera, abi.render_params(size, size, c, seed=1000 * n + j))[0] ** 2
                     for j, c in enumerate(counts)]
            Ssum, Q = VF.chunk_sums(means, counts)
            k = len(counts)
            samples, chunks = np.full((size, size), n, dtype=np.int32), np.full((size, size), k, dtype=np.int32)
            raw = np.sqrt(Ssum / n)

            def rmse(sigma_luminance, min_chunks):
                out, _ = VF.filter_frame(Ssum, Q, samples, chunks, guides, dparams, sigma_luminance=sigma_luminance,
                                         min_chunks=min_chunks)
                return M.gamma_rmse(out, truth)

            row = {"chunks": k, "raw": M.gamma_rmse(raw, truth), "atrous": M.gamma_rmse(M.denoise(raw, guides, **dparams), truth),
                   "spatial_variance": {str(sl): rmse(sl, k + 1) for sl in SIGMAS},
                   "batch_variance": {"sigma_luminance=%g,min_chunks=%d" % (sl, mc): rmse(sl, mc)
                                      for sl in SIGMAS for mc in MIN_CHUNKS if k >= mc}}
            rows[str(n)] = row
            print(n, json.dumps(row), flush=True)
        results["scenes"][name] = rows
    save("quality", results)


# ---- cost on the device -----------------------------------------------------------------------------------------------------

def _setup():
    rt = importlib.import_module("racer-tracer_amd")
    host = importlib.import_module("racer-tracer_amd.host")
    if rt.device_count() < 1:
        raise SystemExit("time_variance_filter.py --cost needs a GPU")
    session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", "cornell_box.yml"))
    p = session.params
    cam = host.camera_new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 0.0, 10000.0, p.width, p.height)
    return rt, session, cam


def trace_run(reps=6):
    """The workload rocprofv3 traces: every kernel reps + 1 times at 1080p."""
    import ctypes as C
    import numpy as np
    import torch
    rt, session, cam = _setup()
    scene = rt.Scene(session)
    p = session.params
    p.samples = 48
    h, w = p.height, p.width
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    _, out, _ = scene.render_adaptive_filtered(cam, p, threshold=0.0)
    planes = {k: torch.from_numpy(np.ascontiguousarray(out[k])).to(dev) for k in ("sums", "squares", "samples", "chunks")}
    guides = {"normal": torch.zeros((h, w, 3), **f64), "position": torch.zeros((h, w, 3), **f64),
              "albedo": torch.zeros((h, w, 3), **f64), "footprint": torch.zeros((h, w), **f64),
              "obj_id": torch.zeros((h, w), dtype=torch.int32, device=dev)}
    hist = {"radiance": torch.zeros((h, w, 3), **f64), "moments": torch.zeros((h, w, 2), **f64),
            "length": torch.zeros((h, w), **f64), "normal": torch.zeros((h, w, 3), **f64),
            "position": torch.zeros((h, w, 3), **f64), "obj_id": torch.zeros((h, w), dtype=torch.int32, device=dev)}
    frame = torch.from_numpy(np.ascontiguousarray(out["raw_rgb"])).to(dev)
    rad, var, dst = torch.zeros((h, w, 3), **f64), torch.zeros((h, w), **f64), torch.zeros((h, w, 3), **f64)
    g = rt.guides_struct(guides)
    rt.check(scene._lib.rt_render_guides_device(scene._h, C.byref(cam), C.byref(p), C.byref(g), None), "guides")
    for _ in range(reps + 1):
        scene.temporal_accumulate_device(p, frame.data_ptr(), g, rt.history_struct(hist))
        scene.denoise_history_device(p, rt.history_struct(hist), g, dst.data_ptr())
        scene.batch_variance_device(p, rt.batch_planes_struct(planes), g, rad.data_ptr(), var.data_ptr())
        scene.denoise_variance_device(p, rad.data_ptr(), var.data_ptr(), g, dst.data_ptr())
        torch.cuda.synchronize(dev)
    scene.close()


def cost():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--trace-run"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if run.returncode != 0 or not found:
            raise SystemExit("rocprofv3 failed (%d): %s" % (run.returncode, run.stderr[-2000:]))
        spans = {}
        for row in csv.DictReader(open(found[0])):
            m = re.search(r"k_(batch_variance_spatial|batch_variance|temporal_variance|temporal_accumulate)", row["Kernel_Name"])
            if m:
                spans.setdefault(m.group(0), []).append((int(row["Start_Timestamp"]),
                                                         (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows = {}
    for name, v in sorted(spans.items()):
        v.sort()
        us = [t for _, t in v][-6:]      # the composed call's launch and the first pass of the loop aside
        rows[name] = {"median_us": statistics.median(us), "launches": len(us)}
    print(json.dumps(rows), flush=True)
    save("cost_1920x1080", rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    args = ap.parse_args()
    if args.trace_run:
        trace_run()
    if args.quality:
        quality()
    if args.cost:
        cost()
