"""Cost of the ray query on one MI355X next to k_guides_f64 -> profiles/ray_query_timings.json.

    python tools/time_rays.py

ONE run of a child process (this file with --trace-run) under `rocprofv3 --kernel-trace --stats`, no counters, the program
behind `--`.  The child launches every case seven times in a fixed order and prints that order; the medians of the last six
launches of each case are reported.  All at 1920 x 1080 = 2 073 600 rays:

  a  the pixel-centre rays of C3's cornell_box camera through rt_trace_rays_device, all planes requested, and
     k_guides_f64 (rt_render_guides_device) on the same camera;
  b  the same pair on `random` (the tree in LDS for renders; the query and the guides walk its global copy) and on
     tests/variant_scenes.py's large_bvh_scene (the tree in global memory);
  c  a's rays with origins and directions shuffled (one permutation for both planes);
  d  any mode on a's rays, the prim plane only.

Per case: microseconds, rays per second, and the bytes the kernel moves per ray (56 B of origin, direction and time read — the window is
the default, its planes NULL —, 100 B written with all planes, 4 B with prim alone; the guides read none and write 88 B) as a rate, next to the device's HBM rate (8 TB/s).
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
OUT = os.path.join(ROOT, "profiles", "ray_query_timings.json")
W, H, REPS = 1920, 1080, 6
HBM_BYTES_PER_S = 8.0e12
KERNELS = r"k_(trace_rays_f64|guides_f64)"
# bytes per ray: (read, written)
BYTES = {"rays_all": (56, 100), "rays_prim": (56, 4), "guides": (0, 88)}


def pixel_rays(cam, w, h):
    """k_guides_f64's rays: through the pixel centres, pinhole, at the middle of the shutter."""
    import numpy as np
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    u = ((px.ravel() + 0.5) / (w - 1))[:, None]
    v = ((py.ravel() + 0.5) / (h - 1))[:, None]
    o = np.array(cam.origin[:])
    d = np.array(cam.upper_left_corner[:]) + u * np.array(cam.horizontal[:]) - v * np.array(cam.vertical[:]) - o
    return np.ascontiguousarray(np.tile(o, (w * h, 1))), np.ascontiguousarray(d), np.full(w * h, (cam.time_a + cam.time_b) * 0.5)


def trace_run():
    """The workload rocprofv3 traces; prints the launch plan: [case, bytes key] per group of REPS + 1 launches, in order."""
    import ctypes as C
    import numpy as np
    import torch
    import variant_scenes as V
    rt = importlib.import_module("racer-tracer_amd")
    host = importlib.import_module("racer-tracer_amd.host")
    rays = importlib.import_module("racer-tracer_amd.rays")
    if rt.device_count() < 1:
        raise SystemExit("time_rays.py needs a GPU")
    abi = rt.abi
    dev = torch.device("cuda", 0)
    config = os.path.join(ROOT, "scenes", "config_c3.yml")
    cornell = host.Session(config, scene=os.path.join(ROOT, "scenes", "cornell_box.yml"))
    rand = host.Session(config, scene="random")
    large, large_cam = V.large_bvh_scene()
    scenes = {
        "cornell_box": (rt.Scene(cornell), host.camera_new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 0.0, 10000.0, W, H)),
        "random": (rt.Scene(rand), rand.camera),
        "large_bvh": (rt.Scene(large, closest_hit=abi.RT_HIT_BVH),
                      host.camera_new(large_cam["look_from"], large_cam["look_at"], large_cam["vfov"], 0.0,
                                      large_cam["focus_distance"], W, H)),
    }
    p = abi.render_params(W, H, 1)
    f64 = dict(dtype=torch.float64, device=dev)
    guides = {"normal": torch.zeros((H, W, 3), **f64), "position": torch.zeros((H, W, 3), **f64),
              "albedo": torch.zeros((H, W, 3), **f64), "footprint": torch.zeros((H, W), **f64),
              "obj_id": torch.zeros((H, W), dtype=torch.int32, device=dev)}
    g = rt.guides_struct(guides)
    out = {name: torch.zeros((W * H,) if width == 1 else (W * H, width), dtype=torch.float64 if dbl else torch.int32, device=dev)
           for name, (width, dbl) in rays.HIT_PLANES.items()}
    plan, variants = [], {}

    def repeat(case, key, call):
        for _ in range(REPS + 1):
            call()
            torch.cuda.synchronize(dev)
        plan.append([case, key])

    for name, (scene, cam) in scenes.items():
        variants[name] = scene.variant()
        o, d, t = (torch.tensor(a, **f64) for a in pixel_rays(cam, W, H))
        repeat(name + " rays closest, all planes", "rays_all", lambda: rays.trace_rays_torch(scene, o, d, time=t, out=out))
        repeat(name + " k_guides_f64", "guides", lambda: rt.check(
            scene._lib.rt_render_guides_device(scene._h, C.byref(cam), C.byref(p), C.byref(g), None), "guides"))
        if name == "cornell_box":
            perm = torch.tensor(np.random.default_rng(2026).permutation(W * H), device=dev)
            so, sd = o[perm].contiguous(), d[perm].contiguous()
            repeat(name + " rays closest, shuffled", "rays_all", lambda: rays.trace_rays_torch(scene, so, sd, time=t, out=out))
            repeat(name + " rays any, prim only", "rays_prim", lambda: rays.trace_rays_torch(
                scene, o, d, time=t, mode=rays.RT_RAYS_ANY, planes=("prim",), out=out))
    for scene, _ in scenes.values():
        scene.close()
    print("PLAN " + json.dumps({"plan": plan, "variants": variants}), flush=True)


def main():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--trace-run"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        m = re.search(r"^PLAN (.*)$", run.stdout, re.M)
        if run.returncode != 0 or not found or not m:
            raise SystemExit("rocprofv3 failed (%d): %s" % (run.returncode, run.stderr[-2000:]))
        info = json.loads(m.group(1))
        launches = []
        for row in csv.DictReader(open(found[0])):
            k = re.search(KERNELS, row["Kernel_Name"])
            if k:
                launches.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3,
                                 k.group(0)))
    launches.sort()
    if len(launches) != (REPS + 1) * len(info["plan"]):
        raise SystemExit("%d launches traced, %d planned" % (len(launches), (REPS + 1) * len(info["plan"])))
    n = W * H
    rows = {"rays": n, "hbm_bytes_per_s": HBM_BYTES_PER_S, "variants": info["variants"], "cases": {}}
    for i, (case, key) in enumerate(info["plan"]):
        group = launches[i * (REPS + 1):(i + 1) * (REPS + 1)]
        names = {name for _, _, name in group}
        assert len(names) == 1 and ("guides" in key) == ("guides" in next(iter(names))), (case, names)
        us = statistics.median(t for _, t, _ in group[1:])      # the first launch of a case aside
        read, written = BYTES[key]
        rate = n * (read + written) / (us * 1e-6)
        rows["cases"][case] = {"kernel": next(iter(names)), "median_us": us, "launches": REPS, "rays_per_s": n / (us * 1e-6),
                               "bytes_read_per_ray": read, "bytes_written_per_ray": written, "bytes_per_s": rate,
                               "share_of_hbm_rate": rate / HBM_BYTES_PER_S}
    for name in info["variants"]:
        q, gd = rows["cases"][name + " rays closest, all planes"], rows["cases"][name + " k_guides_f64"]
        rows["cases"][name + " rays closest, all planes"]["ratio_to_guides"] = q["median_us"] / gd["median_us"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(rows, open(OUT, "w"), indent=1)
    print(json.dumps(rows["cases"], indent=1), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    if ap.parse_args().trace_run:
        trace_run()
    else:
        main()
