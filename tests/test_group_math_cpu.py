"""The group arithmetic of the wave-cooperative samplers (racer-tracer_amd/csrc/rt_pool_groups.h) on the CPU:
tests/group_math_driver.cpp is compiled with the host compiler and held to

  * the DEFINITION of the group size (the largest lg with n << lg <= 64) and the chain of comparisons the samplers ran
    before (`n > 32 ? 0 : n > 16 ? 1 : ...`), for every n in 1 .. 64;
  * the shift ladder that `lowest_in_groups` ran in every round before the table (`low |= low << ((q << k) & 63)`,
    `top = low << (q - 1)`) and the old width mask, for every lg in 1 .. 6 (and lg = 0, which the samplers never ask for but
    the table holds: every lane its own group);
  * the Python model of tests/test_philox_prefix.py for `lowest_in_groups`, on that test's word list, and the per-group
    `x & -x` itself.

The same driver is then built with -fsanitize=address,undefined -fno-sanitize-recover=all and run as the stand-alone
program it is (nothing preloaded): the table read and every shift stay inside their bounds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_philox_prefix as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "racer-tracer_amd", "csrc")
M64 = (1 << 64) - 1


def build_driver(exe, extra=()):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "group_math_driver.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def old_chain(n):
    return 0 if n > 32 else 1 if n > 16 else 2 if n > 8 else 3 if n > 4 else 4 if n > 2 else 5 if n > 1 else 6


def by_definition(n):
    return max(lg for lg in range(7) if n << lg <= 64)


def old_ladder(lg):
    """(low, top, width) as the device code formed them in every grouped round."""
    q = 1 << lg
    low = 1
    for k in range(6):
        low |= (low << ((q << k) & 63)) & M64
    top = (low << (q - 1)) & M64
    width = M64 if lg == 6 else (1 << q) - 1
    return low, top, width


def words():
    """The word list of test_philox_prefix.test_lowest_in_groups_picks_the_first_accepted_lane_of_every_group."""
    rng = np.random.default_rng(3)
    w = [0, (1 << 64) - 1, 1, 1 << 63, 0x8000000080000000, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA]
    w += [int(v) for v in rng.integers(0, 2**63, size=3000, dtype=np.uint64)]
    w += [int(a) & int(b) & int(c) for a, b, c in rng.integers(0, 2**63, size=(1000, 3), dtype=np.uint64)]
    w += [(x << 1 | 1) & M64 for x in w[:200]]
    return w


def commands():
    cmds = ["lg %d" % n for n in range(1, 65)]
    cmds += ["masks %d" % lg for lg in range(7)]
    cmds += ["lowest %x %d" % (x, lg) for lg in range(7) for x in words()]
    return cmds


def run_driver(exe, env=None):
    run = subprocess.run([exe], input="\n".join(commands()) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    return run.stdout.split("\n")[:-1]


def check(lines):
    assert len(lines) == len(commands())
    at = 0
    for n in range(1, 65):
        got = int(lines[at])
        assert got == by_definition(n) == old_chain(n), (n, got)
        at += 1
    for lg in range(7):
        low, top, width = (int(v, 16) for v in lines[at].split())
        if lg == 0:
            assert (low, top, width) == (M64, M64, 1)
        else:
            assert (low, top, width) == old_ladder(lg), lg
        assert low == sum(1 << b for b in range(0, 64, 1 << lg))
        at += 1
    ws = words()
    for lg in range(7):
        q = 1 << lg
        for x in ws:
            got = int(lines[at], 16)
            at += 1
            want = 0
            for g in range(0, 64, q):
                field = (x >> g) & ((1 << q) - 1)
                want |= (field & -field) << g
            assert got == want, (hex(x), lg)
            if lg >= 1:
                assert got == P.lowest_in_groups(x, lg), (hex(x), lg)
    assert at == len(lines)


def test_group_math_is_the_definition_the_old_chain_and_the_old_ladder(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "group_math_driver")
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr[-3000:]
    check(run_driver(exe))


def test_group_math_is_clean_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "group_math_driver_san")
    build = build_driver(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("sanitizer runtimes not installed: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    check(run_driver(exe, env=env))
