"""The chunked host form that rt_trace_rays, rt_trace_occlusion and rt_trace_rays_multi share
(racer-tracer_amd/csrc/rt_query_stage.h: stage_query), on the CPU: tests/query_stage_driver.cpp is compiled with plain g++
against the ROCm headers and is NOT linked against the HIP runtime — it defines the runtime functions the header calls
itself (device memory from malloc, copies that must stay inside a live device allocation, counted synchronisations, a call
that fails on request) and a launcher that checks the planes it is handed and answers with values the driver then looks for,
entry by entry, in the caller's planes.  The driver checks every case itself and prints one line per case; it is built and
run twice, plain and under -fsanitize=address,undefined with leak detection."""
import os
import shutil
import subprocess

import pytest

from test_resources_cpu import CSRC, ROOT, rocm_include

# the driver's cases, in the order it runs them
CASES = ["closest", "occlusion", "multihit", "second_call_allocates_nothing", "failing_runtime_call"]


def build_driver(exe, extra=()):
    """g++ over the driver and rt_error.cpp (the text behind RT_HIP's refusals), no HIP runtime -> CompletedProcess."""
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", *extra, "-I" + rocm_include(),
           "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "query_stage_driver.cpp"), os.path.join(CSRC, "rt_error.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def check_run(exe, env=None):
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-500:], run.stderr[-3000:])
    assert run.stderr == "", run.stderr[-3000:]
    assert run.stdout.splitlines() == ["ok " + c for c in CASES]
    return run


@pytest.fixture(scope="module")
def toolchain():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if rocm_include() is None:
        pytest.skip("no ROCm headers")


def test_every_query_stages_its_planes_through_the_scene_buffers(toolchain, tmp_path):
    exe = str(tmp_path / "query_stage_driver")
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr[-3000:]
    check_run(exe)


def test_every_query_stages_its_planes_under_asan_and_ubsan(toolchain, tmp_path):
    exe = str(tmp_path / "query_stage_sanitize")
    build = build_driver(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("sanitizer runtimes not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = check_run(exe, env)
    assert "runtime error" not in run.stdout and "Sanitizer" not in run.stdout


def test_the_host_forms_have_one_home():
    """The structure the shared form buys: the library's units copy ray planes to and from the staging buffers in
    rt_query_stage.h alone, and rt_query.hip holds no copy loop of its own."""
    found = []
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            for no, line in enumerate(f, 1):
                code = line.split("//")[0]
                if name != "rt_query_stage.h" and ("rays_in" in code or "rays_out" in code or "rays_ids" in code) and "DevBuf" not in code:
                    found.append("%s:%d: %s" % (name, no, line.strip()))
                if name == "rt_query.hip" and "hipMemcpyAsync" in code:
                    found.append("%s:%d: %s" % (name, no, line.strip()))
    assert not found, "\n".join(found)
