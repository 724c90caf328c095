"""The S family of tests/query_ray_sets.py through the three ray queries of ONE library, without assertions: per scene,
flavour, scale e and query, on how many rays the answer differs from the same device's answer at e = 0 (t rescaled).

    RACER_TRACER_AMD_LIB=<a library, e.g. the parent commit's> python tools/survey_query_ray_scales.py OUT.json [scene ...]

Only the entries that are not all zero are written (profiles/query_rays_scale_survey_parent.json is the parent commit's
library under this script); "clean" lists the cases without any.  Needs a GPU.
"""
import importlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np      # noqa: E402
import query_ray_sets as R      # noqa: E402
import test_gpu_query_rays as T      # noqa: E402


def differing_bits(a, b):
    return int((a.view(np.int64) != b.view(np.int64)).sum())


def main():
    out_path, names = sys.argv[1], sys.argv[2:] or R.SCENES
    rt = importlib.import_module("racer-tracer_amd")
    mods = {m: importlib.import_module("racer-tracer_amd." + m) for m in ("rays", "occlusion", "multihit")}
    out = {"columns": "closest prim / occluded / multi-hit count at k = 1, 4, 8 / closest t in bits", "cases": {}, "clean": []}
    for name in names:
        rays = R.s_base(name)
        for flavour in T.FLAVOURS:
            scene = T.open_scene(rt, name, flavour)
            try:
                answers = {e: T.rescaled(T.ask(mods, scene, R.scaled(rays, e)), e) for e in R.SCALES}
            finally:
                scene.close()
            unit, rows = answers[0], {}
            for e, a in answers.items():
                row = [int((a["prim"] != unit["prim"]).sum()), int((a["occluded"] != unit["occluded"]).sum())]
                row += [int((a["multi"][k]["count"] != unit["multi"][k]["count"]).sum()) for k in T.KS]
                row.append(differing_bits(a["t"], unit["t"]) if flavour == "exact" else 0)      # (bits are the reference flavour's promise)
                if any(row):
                    rows[str(e)] = row
            case = "%s %s" % (name, flavour)
            if rows:
                out["cases"][case] = {"rays": len(rays["origin"]), "hit_at_0": int((unit["prim"] >= 0).sum()), "by_e": rows}
            else:
                out["clean"].append(case)
            print(case, rows, flush=True)
    text = json.dumps(out, indent=1)      # (a row of six counts on one line)
    text = re.sub(r"\[\s+((?:-?\d+,\s+)*-?\d+)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
