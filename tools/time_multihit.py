"""Cost of the multi-hit query on one MI355X next to k_trace_rays_f64 -> profiles/multihit_timings.json.

    python tools/time_multihit.py

ONE run of a child process (this file with --trace-run) under `rocprofv3 --kernel-trace --stats`, no counters, the program
behind `--`, in the manner of tools/time_occlusion.py.  The child launches every case seven times in a fixed order and
prints that order; the medians of the last six launches of each case are reported.  All at 1920 x 1080 = 2 073 600
pixel-centre rays of the scene's camera with the default window, on cornell_box (linear), `random` (a tree that renders
stage in LDS; queries walk its global copy) and tests/variant_scenes.py's large_bvh_scene (ordered node arrays in global
memory).

Per scene: k_trace_rays_multi_f64 with k = 1, 4 and 8 and the t, prim and obj_id planes plus count (16 k + 4 B per ray),
and two yardsticks of the same run:

  closest  k_trace_rays_f64, RT_RAYS_CLOSEST, with the same three planes (16 B per ray): k = 1 asks the same question, so
           that ratio is what the list costs;
  peel     what a caller pays today for k answers: k successive closest launches, launch j + 1 with t_min moved just past
           launch j's t (a ray that has missed goes on with t_min = inf, an invalid ray, which leaves at once).  Its
           answers are not the multi-hit query's (a sphere answers again with its far root; ties are lost); only the cost
           is compared.  Reported as the sum of the medians of launches 0 .. k - 1.

Also reported: the mean number of filled slots per ray at each k.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "multihit_timings.json")
W, H, REPS = 1920, 1080, 6
KS = (1, 4, 8)
PLANES = ("t", "prim", "obj_id")
KERNELS = r"k_(trace_rays_multi_f64|trace_rays_f64)"


def trace_run():
    """The workload rocprofv3 traces; prints the launch plan: [case, launches] per group, in order."""
    import torch
    import variant_scenes as V
    from time_rays import pixel_rays
    rt = importlib.import_module("racer-tracer_amd")
    host = importlib.import_module("racer-tracer_amd.host")
    rays = importlib.import_module("racer-tracer_amd.rays")
    mh = importlib.import_module("racer-tracer_amd.multihit")
    if rt.device_count() < 1:
        raise SystemExit("time_multihit.py needs a GPU")
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
    f64 = dict(dtype=torch.float64, device=dev)
    n = W * H
    kmax = max(KS)
    near = {"t": torch.zeros(n, **f64), "prim": torch.zeros(n, dtype=torch.int32, device=dev),
            "obj_id": torch.zeros(n, dtype=torch.int32, device=dev)}
    slots = {"t": torch.zeros(kmax * n, **f64), "prim": torch.zeros(kmax * n, dtype=torch.int32, device=dev),
             "obj_id": torch.zeros(kmax * n, dtype=torch.int32, device=dev), "count": torch.zeros(n, dtype=torch.int32, device=dev)}
    plan, variants, filled = [], {}, {}

    def repeat(case, call, launches=REPS + 1):
        for _ in range(launches):
            call()
            torch.cuda.synchronize(dev)
        plan.append([case, launches])

    for name, (scene, cam) in scenes.items():
        variants[name] = scene.variant()
        o, d, t = (torch.tensor(a, **f64) for a in pixel_rays(cam, W, H))
        for k in KS:
            repeat("%s multi k=%d" % (name, k), lambda: mh.trace_rays_multi_torch(scene, o, d, k, time=t, planes=PLANES, out=slots))
            filled["%s k=%d" % (name, k)] = float(slots["count"].double().mean())
        t_min = torch.full((n,), 0.001, **f64)
        for j in range(kmax):
            repeat("%s peel %d" % (name, j), lambda: rays.trace_rays_torch(scene, o, d, t_min=t_min, time=t, planes=PLANES, out=near))
            t_min = torch.nextafter(near["t"], torch.full((n,), float("inf"), **f64)).contiguous()      # (inf stays inf)
    for scene, _ in scenes.values():
        scene.close()
    print("PLAN " + json.dumps({"plan": plan, "variants": variants, "filled": filled}), flush=True)


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
    if len(launches) != sum(count for _, count in info["plan"]):
        raise SystemExit("%d launches traced, %d planned" % (len(launches), sum(count for _, count in info["plan"])))
    at = 0
    medians = {}
    for case, count in info["plan"]:
        group, at = launches[at:at + count], at + count
        names = {name for _, _, name in group}
        assert len(names) == 1 and ("multi" in case) == ("multi" in next(iter(names))), (case, names)
        medians[case] = statistics.median(t for _, t, _ in group[1:])      # the first launch aside
    rows = {"rays": W * H, "launches": REPS, "planes": list(PLANES), "variants": info["variants"], "cases": {}}
    for name in info["variants"]:
        closest = medians["%s peel 0" % name]
        peel = [medians["%s peel %d" % (name, j)] for j in range(max(KS))]
        for k in KS:
            us = medians["%s multi k=%d" % (name, k)]
            rows["cases"]["%s k=%d" % (name, k)] = {
                "median_us": us, "closest_median_us": closest, "ratio_to_closest": us / closest,
                "peel_us": sum(peel[:k]), "ratio_to_peel": us / sum(peel[:k]), "peel_launches_us": peel[:k],
                "bytes_written_per_ray": 16 * k + 4, "filled_slots_per_ray": info["filled"]["%s k=%d" % (name, k)],
                "rays_per_s": W * H / (us * 1e-6)}
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
