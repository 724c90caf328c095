"""Cost and quality of temporal accumulation -> profiles/temporal.json.

    python tools/time_temporal.py --quality        # CPU only: the numpy model on oracle frames, and the sweep of the defaults
    python tools/time_temporal.py --cost           # one MI355X: kernel times under a rocprofv3 kernel trace, call overhead

--quality: cornell_box_boxes at 128x128, eight frames of 4 spp on an orbit of 1 degree per frame, against a 512-spp oracle
frame of the last camera (as DESIGN.md 4.6 did for the spatial filter): the gamma RMSE of the last raw frame, of the
spatial filter alone, of the history alone, of the history under the spatial filter and under the variance-guided one, and
the sweeps over sigma_luminance and the two tolerances that chose rt_temporal_params_default.

--cost: at the 1080p size of scenes/config_c3.yml on cornell_box.  A child process (this file with --trace-run) runs under
`rocprofv3 --kernel-trace`, no counters: six times the guides, rt_denoise_device's five levels, the accumulation onto a
history from a camera 1 degree away, and rt_denoise_history_device; the medians of each kernel's six launches are reported
next to the existing filter's levels of the same run.  Then, in this process and by the host's clock, rt_render_temporal
against rt_render_frame at 4 and 16 spp (the median of 6 calls on an orbiting camera).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "temporal.json")


def save(section, rows):
    results = json.load(open(OUT)) if os.path.exists(OUT) else {}
    results[section] = rows
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(results, open(OUT, "w"), indent=1)


# ---- quality on the model -------------------------------------------------------------------------------------------------

def quality(frames=8, spp=4, size=128, truth_spp=512):
    import denoise_model as M
    import scenes_py as S
    import temporal_model as T
    from oracle import oracle_ctypes as orc
    abi = S.abi
    bundle, cam = S.cornell_box_boxes()[:2]
    cams = [S.camera_for(T.orbit(cam, float(k)), size, size) for k in range(frames)]
    rgbs = [orc.render(bundle.desc, cams[k], abi.render_params(size, size, spp, seed=1 + k))[0] for k in range(frames)]
    guides = [M.oracle_guides(orc, bundle, c, size, size) for c in cams]
    truth = orc.render(bundle.desc, cams[-1], abi.render_params(size, size, truth_spp, seed=99))[0]
    print("frames, guides and the %d-spp frame are made" % truth_spp, flush=True)

    def history(**tp):
        h = None
        for k in range(frames):
            h, info = T.accumulate(rgbs[k], guides[k], h, T.camera_vectors(cams[k - 1]) if k else None, **dict(T.DEFAULTS, **tp))
        return h, info

    def rmse(x):
        return M.gamma_rmse(x, truth)

    g = guides[-1]
    h, info = history()
    hit = g["obj_id"] >= 0
    rows = {"scene": "cornell_box_boxes", "size": size, "frames": frames, "spp": spp, "truth_spp": truth_spp,
            "defaults": T.DEFAULTS,
            "continued_percent_of_hit_pixels": 100.0 * float((hit & ~info["fresh"]).sum()) / float(hit.sum()),
            "mean_history_length": float(h["length"][hit].mean()),
            "rmse_last_raw_frame": rmse(rgbs[-1]),
            "rmse_spatial_filter_alone": rmse(M.denoise(rgbs[-1], g)),
            "rmse_history_alone": rmse(T.denoise_history(h, g, iterations=0)),
            "rmse_history_spatial_filter": rmse(T.denoise_history(h, g, sigma_luminance=0.0)),
            "rmse_history_variance_guided": rmse(T.denoise_history(h, g, sigma_luminance=T.DEFAULTS["sigma_luminance"]))}
    print(json.dumps(rows), flush=True)
    rows["sweep_sigma_luminance"] = {str(sl): rmse(T.denoise_history(h, g, sigma_luminance=sl)) for sl in (0.5, 1.0, 2.0, 4.0, 8.0, 16.0)}
    print(json.dumps(rows["sweep_sigma_luminance"]), flush=True)
    sweep = {}
    for nt, pt in ((0.05, 2.0), (0.1, 2.0), (0.25, 2.0), (0.5, 2.0), (1.0, 2.0), (0.25, 0.5), (0.25, 1.0), (0.25, 4.0), (0.25, 16.0)):
        hh, ii = history(normal_tolerance=nt, plane_tolerance=pt)
        sweep["normal_tolerance=%g,plane_tolerance=%g" % (nt, pt)] = {
            "continued_percent": 100.0 * float((hit & ~ii["fresh"]).sum()) / float(hit.sum()),
            "rmse_history_alone": rmse(T.denoise_history(hh, g, iterations=0)),
            "rmse_history_variance_guided": rmse(T.denoise_history(hh, g))}
    rows["sweep_tolerances"] = sweep
    print(json.dumps(sweep), flush=True)
    sweep = {}
    for a in (0.05, 0.1, 0.2, 0.4):
        hh, _ = history(alpha=a, alpha_moments=a)
        sweep["alpha=%g" % a] = {"rmse_history_alone": rmse(T.denoise_history(hh, g, iterations=0)),
                                 "rmse_history_variance_guided": rmse(T.denoise_history(hh, g))}
    rows["sweep_alpha"] = sweep
    print(json.dumps(sweep), flush=True)
    save("quality", rows)


# ---- cost on the device -----------------------------------------------------------------------------------------------------

def _setup():
    rt = importlib.import_module("racer-tracer_amd")
    host = importlib.import_module("racer-tracer_amd.host")
    import temporal_model as T
    if rt.device_count() < 1:
        raise SystemExit("time_temporal.py --cost needs a GPU")
    session = host.Session(os.path.join(ROOT, "scenes", "config_c3.yml"), scene=os.path.join(ROOT, "scenes", "cornell_box.yml"))
    cam = dict(look_from=(278.0, 278.0, -800.0), look_at=(278.0, 278.0, 0.0), vfov=40.0, aperture=0.0, focus_distance=10000.0)
    p = session.params
    cams = [host.camera_new(T.orbit(cam, float(k))["look_from"], cam["look_at"], cam["vfov"], cam["aperture"],
                            cam["focus_distance"], p.width, p.height) for k in range(8)]
    return rt, session, cams


def trace_run(reps=6):
    """The workload rocprofv3 traces: every kernel `reps` times at 1080p."""
    import torch
    rt, session, cams = _setup()
    import ctypes as C
    scene = rt.Scene(session)
    p = session.params
    p.samples = 4
    h, w = p.height, p.width
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)

    def history():
        return {"radiance": torch.zeros((h, w, 3), **f64), "moments": torch.zeros((h, w, 2), **f64),
                "length": torch.zeros((h, w), **f64), "normal": torch.zeros((h, w, 3), **f64),
                "position": torch.zeros((h, w, 3), **f64), "obj_id": torch.zeros((h, w), dtype=torch.int32, device=dev)}

    guides = {"normal": torch.zeros((h, w, 3), **f64), "position": torch.zeros((h, w, 3), **f64),
              "albedo": torch.zeros((h, w, 3), **f64), "footprint": torch.zeros((h, w), **f64),
              "obj_id": torch.zeros((h, w), dtype=torch.int32, device=dev)}
    frame, out = torch.zeros((h, w, 3), **f64), torch.zeros((h, w, 3), **f64)
    hist = [history(), history()]
    g = rt.guides_struct(guides)
    prev_cam = None
    for k in range(reps + 1):     # the first pass makes a history; the others are traced alike
        cam = cams[k % len(cams)]
        p.seed = 1 + k
        cur, old = hist[k & 1], hist[(k & 1) ^ 1]
        scene.render_frame_device(cam, p, frame.data_ptr())
        rt.check(scene._lib.rt_render_guides_device(scene._h, C.byref(cam), C.byref(p), C.byref(g), None), "guides")
        scene.denoise_device(p, frame.data_ptr(), g, out.data_ptr())
        scene.temporal_accumulate_device(p, frame.data_ptr(), g, rt.history_struct(cur), prev_cam,
                                         rt.history_struct(old) if prev_cam is not None else None)
        scene.denoise_history_device(p, rt.history_struct(cur), g, out.data_ptr())
        torch.cuda.synchronize(dev)
        prev_cam = cam
    scene.close()


def cost():
    rows = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--trace-run"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if run.returncode != 0 or not found:
            raise SystemExit("rocprofv3 failed (%d): %s" % (run.returncode, run.stderr[-2000:]))
        spans = {}
        for row in csv.DictReader(open(found[0])):
            m = re.search(r"k_(temporal|denoise|guides)_[a-z0-9_]+", row["Kernel_Name"])
            if not m:
                continue
            name = m.group(0)
            spans.setdefault(name, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    for name, v in sorted(spans.items()):
        v.sort()
        if len(v) >= 7:
            us = [t for _, t in v]
            per_call = len(us) // 7 if len(us) >= 7 else 1       # 7 passes: launches of one pass are consecutive
            # launch i of a pass: the median over the last six passes
            rows[name] = [statistics.median(us[c * per_call + i] for c in range(1, len(us) // per_call)) for i in range(per_call)]
    print(json.dumps(rows), flush=True)
    # the whole call against rt_render_frame, host clock
    rt, session, cams = _setup()
    scene = rt.Scene(session)
    p = session.params
    t = rt.Temporal(p.width, p.height)
    for spp in (4, 16):
        p.samples = spp
        plain, temporal = [], []
        for k in range(8):
            p.seed = 1 + k
            t0 = time.perf_counter()
            scene.render_frame(cams[k], p)
            plain.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            t.render(scene, cams[k], p)
            temporal.append((time.perf_counter() - t0) * 1e3)
        rows["call_ms@%dspp" % spp] = {"rt_render_frame": statistics.median(plain[2:]), "rt_render_temporal": statistics.median(temporal[2:])}
    t.close()
    scene.close()
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
