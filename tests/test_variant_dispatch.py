"""The one place where a scene's flags become a kernel variant's template arguments (racer-tracer_amd/csrc/
rt_variant_dispatch.h), run on the CPU: tests/variant_dispatch_driver.cpp is compiled with the host compiler — the header
needs no HIP — and prints the pick for every combination of prims_class in {-1, 0, 1, 2, 7}, textured, specular and bvh.
The mapping: with a tree <PRIMS_ANY, t, s, true> whatever the class; without one PRIMS_RECTS and PRIMS_SPHERES map to
themselves and every other value to PRIMS_ANY, B = false."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECTS, SPHERES, ANY = 0, 1, 2


def expected(prims_class, textured, specular, bvh):
    if bvh:
        return (ANY, textured, specular, 1)
    return (prims_class if prims_class in (RECTS, SPHERES) else ANY, textured, specular, 0)


def test_every_combination_of_flags_picks_its_variant(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "variant_dispatch_driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "racer-tracer_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "variant_dispatch_driver.cpp")], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    want = ["%d %d %d %d -> %d %d %d %d" % ((c, t, s, b) + expected(c, t, s, b))
            for c in (-1, 0, 1, 2, 7) for t in (0, 1) for s in (0, 1) for b in (0, 1)]
    assert len(want) == 40
    assert lines == want
