"""Cost of the occlusion query on one MI355X next to k_trace_rays_f64 -> profiles/occlusion_timings.json.

    python tools/time_occlusion.py

ONE run of a child process (this file with --trace-run) under `rocprofv3 --kernel-trace --stats`, no counters, the program
behind `--`, in the manner of tools/time_rays.py.  The child launches every case seven times in a fixed order and prints that
order; the medians of the last six launches of each case are reported.  All at 1920 x 1080 = 2 073 600 rays, on cornell_box
(linear), `random` (a tree that renders stage in LDS; queries walk its global copy) and tests/variant_scenes.py's
large_bvh_scene (ordered node arrays in global memory), with two ray sets per scene:

  a  the pixel-centre rays of the scene's camera with the default window [0.001, inf);
  b  shadow-like segments: from each pixel's first hit point (a closest query of set a, outside the timed launches; a pixel
     that misses starts at the camera) to the centre of the scene's first listed light — where the scene lists none, to
     look_from raised by the scene's spread (SPREAD) —, over the window [1e-3, 1 - 1e-3].

Per scene and set: k_occluded_f64 and, as the yardstick, k_trace_rays_f64 in any mode with the prim plane alone — on a tree
the closest walk, on a linear scene the same early-out loop.  Both write 4 B per ray.  Reported: the medians in microseconds,
their ratio, the occluded share of the set, and the share of its waves (64 consecutive rays) whose lanes are ALL occluded.
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
OUT = os.path.join(ROOT, "profiles", "occlusion_timings.json")
W, H, REPS = 1920, 1080, 6
KERNELS = r"k_(trace_rays_f64|occluded_f64)"
SPREAD = {"cornell_box": 250.0, "random": 10.0, "large_bvh": 30.0}      # (large_bvh: tests/ray_query_model.py's)
EPS = 1e-3


def light_centre(prim):
    """Centre of a plain rect or sphere of the description (the kinds the default light list holds)."""
    abi = importlib.import_module("racer-tracer_amd.abi")
    p = prim.p
    if prim.kind == abi.RT_PRIM_XY_RECT:
        return ((p[0] + p[1]) / 2, (p[2] + p[3]) / 2, p[4])
    if prim.kind == abi.RT_PRIM_XZ_RECT:
        return ((p[0] + p[1]) / 2, p[4], (p[2] + p[3]) / 2)
    if prim.kind == abi.RT_PRIM_YZ_RECT:
        return (p[4], (p[0] + p[1]) / 2, (p[2] + p[3]) / 2)
    return (p[0], p[1], p[2])


def trace_run():
    """The workload rocprofv3 traces; prints the launch plan: [case, launches] per group, in order."""
    import torch
    import variant_scenes as V
    from time_rays import pixel_rays
    rt = importlib.import_module("racer-tracer_amd")
    host = importlib.import_module("racer-tracer_amd.host")
    rays = importlib.import_module("racer-tracer_amd.rays")
    occ = importlib.import_module("racer-tracer_amd.occlusion")
    if rt.device_count() < 1:
        raise SystemExit("time_occlusion.py needs a GPU")
    abi = rt.abi
    dev = torch.device("cuda", 0)
    config = os.path.join(ROOT, "scenes", "config_c3.yml")
    cornell = host.Session(config, scene=os.path.join(ROOT, "scenes", "cornell_box.yml"))
    rand = host.Session(config, scene="random")
    large, large_cam = V.large_bvh_scene()
    # name -> (scene, camera, description)
    scenes = {
        "cornell_box": (rt.Scene(cornell), host.camera_new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 0.0, 10000.0, W, H),
                        cornell.desc),
        "random": (rt.Scene(rand), rand.camera, rand.desc),
        "large_bvh": (rt.Scene(large, closest_hit=abi.RT_HIT_BVH),
                      host.camera_new(large_cam["look_from"], large_cam["look_at"], large_cam["vfov"], 0.0,
                                      large_cam["focus_distance"], W, H), large.desc),
    }
    f64 = dict(dtype=torch.float64, device=dev)
    n = W * H
    answer = torch.zeros(n, dtype=torch.int32, device=dev)
    prim = {"prim": torch.zeros(n, dtype=torch.int32, device=dev)}
    plan, variants, shares, targets = [], {}, {}, {}

    def repeat(case, call, launches=REPS + 1):
        for _ in range(launches):
            call()
            torch.cuda.synchronize(dev)
        plan.append([case, launches])

    for name, (scene, cam, desc) in scenes.items():
        variants[name] = scene.variant()
        o, d, t = (torch.tensor(a, **f64) for a in pixel_rays(cam, W, H))
        # set b, from one closest query of set a (traced, not timed)
        first = {}
        repeat(name + " setup", lambda: first.update(rays.trace_rays_torch(scene, o, d, time=t, planes=("point", "prim"))), 1)
        lights = scene.lights()
        if len(lights):
            target = light_centre(desc.primitives[int(lights[0])])
            targets[name] = {"light": int(lights[0]), "point": list(target)}
        else:
            target = (cam.origin[0], cam.origin[1] + SPREAD[name], cam.origin[2])
            targets[name] = {"light": None, "point": list(target)}
        start = torch.where((first["prim"] >= 0)[:, None], first["point"], o).contiguous()
        seg = (torch.tensor(target, **f64)[None, :] - start).contiguous()
        lo, hi = torch.full((n,), EPS, **f64), torch.full((n,), 1.0 - EPS, **f64)
        sets = {"a": dict(origins=o, directions=d, time=t), "b": dict(origins=start, directions=seg, t_min=lo, t_max=hi, time=t)}
        for key, kw in sets.items():
            repeat("%s %s occluded" % (name, key), lambda: occ.occluded_torch(scene, out=answer, **kw))
            got = answer.cpu()
            # (n is a multiple of 64: a wave is 64 consecutive rays, and it leaves a tree early only if ALL its lanes are occluded)
            shares["%s %s" % (name, key)] = {"occluded": float((got == 1).double().mean()), "invalid": int((got < 0).sum()),
                                             "waves_all_occluded": float((got.view(-1, 64) == 1).all(dim=1).double().mean())}
            repeat("%s %s rays any, prim only" % (name, key),
                   lambda: rays.trace_rays_torch(scene, mode=rays.RT_RAYS_ANY, planes=("prim",), out=prim, **kw))
            assert bool(((prim["prim"].cpu() >= 0) == (got == 1)).all()), (name, key)      # the same answer, while we are here
    for scene, _, _ in scenes.values():
        scene.close()
    print("PLAN " + json.dumps({"plan": plan, "variants": variants, "shares": shares, "targets": targets}), flush=True)


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
    rows = {"rays": W * H, "launches": REPS, "variants": info["variants"], "targets": info["targets"], "cases": {}}
    at = 0
    medians = {}
    for case, count in info["plan"]:
        group, at = launches[at:at + count], at + count
        names = {name for _, _, name in group}
        assert len(names) == 1 and ("occluded" in case) == ("occluded" in next(iter(names))), (case, names)
        if count > 1:
            medians[case] = (statistics.median(t for _, t, _ in group[1:]), next(iter(names)))      # the first launch aside
    for key, share in info["shares"].items():
        (us, kernel), (ref_us, ref_kernel) = medians[key + " occluded"], medians[key + " rays any, prim only"]
        rows["cases"][key] = {"kernel": kernel, "median_us": us, "yardstick": ref_kernel, "yardstick_median_us": ref_us,
                              "ratio_to_yardstick": us / ref_us, "rays_per_s": W * H / (us * 1e-6),
                              "occluded_share": share["occluded"], "waves_all_occluded_share": share["waves_all_occluded"],
                              "invalid_rays": share["invalid"]}
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
