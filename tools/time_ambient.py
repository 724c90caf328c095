"""Cost of the ambient-occlusion query on one MI355X next to k_occluded_f64 on the same rays
-> profiles/ambient_timings.json.

    python tools/time_ambient.py

ONE run of a child process (this file with --trace-run) under `rocprofv3 --kernel-trace --stats`, no counters, the program
behind `--`, in the manner of tools/time_occlusion.py.  The child launches every case seven times in a fixed order and prints
that order; the medians of the last six launches of each case are reported.  The points are the 1920 x 1080 guide points
(position, normal, the middle of the shutter) of the scene's camera, S = 16 samples each: 33 177 600 rays, on cornell_box
(linear), `random` (a tree that renders stage in LDS; queries walk its global copy) and tests/variant_scenes.py's
large_bvh_scene (ordered node arrays in global memory), with two windows per scene: radius inf and the finite RADIUS below.

Per scene and window:
  fused      k_ambient_f64 without an export: what rt_trace_ambient_device costs (4 B written per POINT);
  export     k_ambient_f64 with all five planes exported: the same launch plus 72 B written per ray;
  yardstick  k_occluded_f64 on those exported rays: the walk alone, on rays that someone else formed and wrote and that it
             reads back; it writes 4 B per RAY.
Reported: the medians in microseconds, fused / yardstick, the bytes each route writes per ray, the open share, whether the
fused counts equal the yardstick's on every point, and an end-to-end figure for the route a caller had before: (export -
fused), what writing the rays costs a kernel that has formed them, plus the yardstick — without the caller's own ray
generator and without its reduction of the answers, so a lower bound.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "ambient_timings.json")
W, H, S, REPS = 1920, 1080, 16, 6
KERNELS = r"k_(ambient_f64|occluded_f64)"
RADIUS = {"cornell_box": 100.0, "random": 1.0, "large_bvh": 3.0}      # world units: a fifth of the box; a big sphere's radius; a tenth of the spread


def trace_run():
    """The workload rocprofv3 traces; prints the launch plan: [case, launches] per group, in order."""
    import torch
    import variant_scenes as V
    rt = importlib.import_module("racer-tracer_amd")
    host = importlib.import_module("racer-tracer_amd.host")
    occ = importlib.import_module("racer-tracer_amd.occlusion")
    amb = importlib.import_module("racer-tracer_amd.ambient")
    if rt.device_count() < 1:
        raise SystemExit("time_ambient.py needs a GPU")
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
    n = W * H
    p = abi.render_params(W, H, 1)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    verdict = torch.zeros(n * S, dtype=torch.int32, device=dev)
    plan, variants, shares = [], {}, {}

    def repeat(case, call, launches=REPS + 1):
        for _ in range(launches):
            call()
            torch.cuda.synchronize(dev)
        plan.append([case, launches])

    for name, (scene, cam) in scenes.items():
        variants[name] = scene.variant()
        guides = scene.render_guides(cam, p)      # (its kernel is not one of KERNELS)
        points = torch.tensor(guides["position"].reshape(n, 3), dtype=torch.float64, device=dev)
        normals = torch.tensor(guides["normal"].reshape(n, 3), dtype=torch.float64, device=dev)
        time = torch.full((n,), (cam.time_a + cam.time_b) * 0.5, dtype=torch.float64, device=dev)
        for label, radius in (("inf", math.inf), ("finite", RADIUS[name])):
            key = "%s %s" % (name, label)
            kw = dict(samples=S, radius=radius, seed=1, time=time)
            walked = {}
            repeat(key + " export", lambda: walked.update(amb.ambient_torch(scene, points, normals, export=True, **kw)[1]))
            repeat(key + " ambient", lambda: amb.ambient_torch(scene, points, normals, out=counts, **kw))
            repeat(key + " occluded", lambda: occ.occluded_torch(scene, walked["origin"], walked["direction"], walked["t_min"],
                                                                 walked["t_max"], walked["time"], out=verdict))
            got, per_ray = counts.cpu(), verdict.cpu().view(n, S)
            valid = got >= 0
            shares[key] = {"radius": radius if math.isfinite(radius) else "inf", "valid_points": int(valid.sum()),
                           "open_share": float(got[valid].double().sum() / max(int(valid.sum()) * S, 1)),
                           "points_that_differ_from_the_yardstick": int((got[valid] != S - (per_ray[valid] == 1).sum(dim=1)).sum()),
                           "invalid_points_whose_rays_are_valid": int((per_ray[~valid] != -2).any(dim=1).sum())}
            del walked
    for scene, _ in scenes.values():
        scene.close()
    print("PLAN " + json.dumps({"plan": plan, "variants": variants, "shares": shares}), flush=True)


def main():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--trace-run"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
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
    rows = {"points": W * H, "samples": S, "rays": W * H * S, "launches": REPS, "variants": info["variants"],
            "bytes_written_per_ray": {"fused": 4.0 / S, "rays_written_then_occlusion_query": 9 * 8 + 4}, "cases": {}}
    at = 0
    medians = {}
    for case, count in info["plan"]:
        group, at = launches[at:at + count], at + count
        names = {name for _, _, name in group}
        assert len(names) == 1 and ("occluded" in case) == ("occluded" in next(iter(names))), (case, names)
        if count > 1:
            medians[case] = statistics.median(t for _, t, _ in group[1:])      # the first launch aside
    for key, share in info["shares"].items():
        us, ref_us, export_us = medians[key + " ambient"], medians[key + " occluded"], medians[key + " export"]
        rows["cases"][key] = dict(share, kernel="k_ambient_f64", median_us=us, yardstick="k_occluded_f64", yardstick_median_us=ref_us,
                                  ratio_to_yardstick=us / ref_us, rays_per_s=W * H * S / (us * 1e-6), export_median_us=export_us,
                                  rays_written_then_yardstick_us=export_us - us + ref_us,
                                  ratio_to_rays_written_then_yardstick=us / (export_us - us + ref_us))
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
