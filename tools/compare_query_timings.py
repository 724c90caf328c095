"""Parent and tree side by side for the three query timing tools (tools/time_rays.py, time_occlusion.py, time_multihit.py).

    python tools/compare_query_timings.py PARENT_DIR TREE_DIR > profiles/query_rays_timings_parent_vs_tree.json

Each directory holds the three files those tools write (ray_query_timings.json, occlusion_timings.json,
multihit_timings.json): run the tools once with RACER_TRACER_AMD_LIB naming the parent commit's library and once without,
in one session, and copy profiles/*_timings.json aside after each.
"""
import json
import os
import sys

FILES = ("ray_query_timings.json", "occlusion_timings.json", "multihit_timings.json")


def main():
    parent_dir, tree_dir = sys.argv[1:3]
    out = {}
    for name in FILES:
        parent = json.load(open(os.path.join(parent_dir, name)))["cases"]
        tree = json.load(open(os.path.join(tree_dir, name)))["cases"]
        out[name] = {}
        for case, row in tree.items():
            a, b = parent[case].get("median_us"), row.get("median_us")
            if a is not None and b is not None:
                out[name][case] = {"kernel": row.get("kernel"), "parent_median_us": a, "tree_median_us": b, "tree_over_parent": round(b / a, 4)}
    json.dump({"note": "medians of 6 launches of 1920 x 1080 rays each, both libraries in one session on one MI355X", "files": out},
              sys.stdout, indent=1)


if __name__ == "__main__":
    main()
