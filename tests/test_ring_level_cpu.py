"""The fill level of the PRETRACE ring as a counter, and "a batch is due" as one comparison
(racer-tracer_amd/csrc/rt_ring_level.h), on the CPU: tests/ring_level_driver.cpp is compiled with the host compiler and
models the item loop of rt_trace_pool_kernel.hip — batches of 64 whose `lives` come from a seeded generator, hand-outs of
min(idle, level) — with the level re-formed from `next` (the expressions the kernel ran before) beside the counter.  Over
more than 10^5 seeded items it holds, at every step: equal levels, equal slots, equal batch decisions, equal "the pool is
dry", never more than RING_SLOTS entries, no slot written while it holds one, and next == total at the loop's exit.
The summary line says what the items covered: pools under one batch and not a multiple of 64, batches with no and with
64 lives, rings that wrapped hundreds of times, items of one batch.

The same driver is then built with -fsanitize=address,undefined -fno-sanitize-recover=all and run as the stand-alone
program it is (nothing preloaded)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "racer-tracer_amd", "csrc")
ITEMS = 120000


def ring_slots():
    """RING_SLOTS as the kernel's LDS layout states it."""
    text = open(os.path.join(CSRC, "rt_pool_lds.h")).read()
    return int(re.search(r"RING_SLOTS\s*=\s*(\d+)u", text).group(1))


def build_driver(exe, extra=()):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "ring_level_driver.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def run_driver(exe, slots, items, seed, env=None):
    run = subprocess.run([exe, str(slots), str(items), str(seed)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    words = run.stdout.split()
    assert words[0] == "ok", run.stdout
    return {k: int(v) for k, v in zip(words[1::2], words[2::2])}


def check_coverage(tally, items):
    print(tally)
    assert tally["items"] >= items
    assert tally["short"] > items // 10       # total below 64
    assert tally["ragged"] > items // 2       # total not a multiple of 64
    assert tally["one_batch"] > items // 10   # n_batches == 1
    assert tally["empty"] > 1000 and tally["full"] > 1000  # batches with zero and with 64 lives
    assert tally["most_wraps"] > 100          # a ring that wraps many times
    assert tally["full_ring"] > 0             # every slot in use


def test_the_kernel_uses_the_header():
    """The rules the driver runs are the ones the kernel calls (and the expressions they replace are gone from it)."""
    text = open(os.path.join(CSRC, "rt_trace_pool_kernel.hip")).read()
    for name in ("after_batch", "taken", "after_hand_out", "slot_at", "batch_below_of", "batch_is_due", "pool_is_dry"):
        assert "rt_ring::" + name + "(" in text, name
    assert "min(batches_done << 6, total) - next" not in text and "min(b << 6, total) - next" not in text


def test_counter_and_one_comparison_against_the_recomputed_level(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "ring_level_driver")
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr[-3000:]
    slots = ring_slots()
    assert slots == 67
    check_coverage(run_driver(exe, slots, ITEMS, 1), ITEMS)
    # (the rules take the ring's size as a number: a ring of exactly one batch, and a roomy one)
    for other, seed in ((64, 2), (200, 3)):
        tally = run_driver(exe, other, 20000, seed)
        assert tally["items"] >= 20000


def test_ring_level_driver_is_clean_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "ring_level_driver_san")
    build = build_driver(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("sanitizer runtimes not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    check_coverage(run_driver(exe, ring_slots(), ITEMS, 1, env=env), ITEMS)
