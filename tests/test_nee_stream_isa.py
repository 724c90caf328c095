"""The streaming form of the NEE kernel (csrc/rt_nee_stream_kernel.hip) compiled for gfx950 in both arithmetic flavours, as
the library builds it: every k_nee_stream_f64 instantiation is there, each is held to k_nee_f64 of the same key and flavour
IN THE SAME COMPILE for scratch memory and for its occupancy step, and the new source holds none of the instructions that
are off limits (the list is tests/test_nee_pass_isa.py's).

Where the build stands (printed by the tests): no scratch in any linear variant, and the occupancy step is
met everywhere but in EXCEPTIONS below."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

import kernel_asm
import test_nee_isa
import test_nee_pass_isa
from test_nee_pass_isa import waves_per_simd

CSRC = os.path.join(kernel_asm.ROOT, "racer-tracer_amd", "csrc")
SRC = os.path.join(CSRC, "rt_nee_stream_kernel.hip")
_KERNEL = re.compile(r"\.amdhsa_kernel _ZN\d+rtdev_(fast|exact)\d+k_nee_stream_f64ILi(\d)ELb([01])ELb([01])ELb([01])EE\w*\n(.*?)"
                     r"\.end_amdhsa_kernel", re.S)

# Variants that sit one occupancy step BELOW k_nee_f64 of the same key: (flavour, key) -> (k_nee_f64 VGPRs, k_nee_stream_f64
# VGPRs) as last compiled.  The goal is an empty table.  The one entry: held to 128 VGPRs this variant spills a double to
# scratch memory, and no scratch in the linear variants ranks above the step.
EXCEPTIONS = {("exact", (0, 0, 1, 0)): (126, 132)}


@functools.lru_cache(maxsize=None)
def stream_kernels(flavour):
    out = os.path.join(tempfile.mkdtemp(prefix="rt_nee_stream_asm_"), "nee_stream_%s.s" % flavour)
    cmd = [kernel_asm.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"] + \
        kernel_asm.FLAVOURS[flavour] + [SRC, "-o", out]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    text = open(out).read()
    found = {}
    for m in _KERNEL.finditer(text):
        assert m.group(1) == flavour
        body = m.group(6)
        found[tuple(int(m.group(k)) for k in (2, 3, 4, 5))] = (
            int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
            int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))
    return found, text


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_every_instantiation_is_compiled(flavour):
    want = {(p, t, s, 0) for p in (0, 1, 2) for t in (0, 1) for s in (0, 1)} | {(2, t, s, 1) for t in (0, 1) for s in (0, 1)}
    found, text = stream_kernels(flavour)
    assert set(found) == want
    assert "k_nee_f64" not in text and "k_nee_pass_f64" not in text  # a kernel of its own, in a file of its own


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_scratch(flavour):
    found, _ = stream_kernels(flavour)
    one_shot = test_nee_isa.nee_kernels(flavour)
    bad = []
    for key, (vgprs, scratch) in sorted(found.items()):
        print(flavour, key, "k_nee_stream_f64 %d VGPRs, %d B scratch; k_nee_f64 %d VGPRs, %d B scratch" % ((vgprs, scratch) + one_shot[key]))
        assert vgprs <= 256, (key, vgprs)
        if scratch > one_shot[key][1] or (key[3] == 0 and scratch != 0):  # the linear-loop variants: no scratch at all
            bad.append((key, scratch, one_shot[key][1]))
    assert not bad, bad


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_occupancy_step(flavour):
    found, _ = stream_kernels(flavour)
    one_shot = test_nee_isa.nee_kernels(flavour)
    for key, (vgprs, _scratch) in sorted(found.items()):
        want = waves_per_simd(one_shot[key][0])
        if (flavour, key) in EXCEPTIONS:
            assert waves_per_simd(vgprs) == want - 1, ("no longer an exception: drop it from the table", flavour, key, vgprs)
            assert EXCEPTIONS[(flavour, key)] == (one_shot[key][0], vgprs), ("the table's counts are stale", flavour, key, one_shot[key][0], vgprs)
        else:  # compared in the same compile, not against a fixed number
            assert waves_per_simd(vgprs) >= want, (flavour, key, vgprs, one_shot[key][0])
    assert {k for k in EXCEPTIONS if k[0] == flavour} <= {(flavour, key) for key in found}
    # the plain-colour rect variants are the ones cornell_box runs: 4 waves per SIMD in the fast flavour
    if flavour == "fast":
        for key in ((0, 0, 0, 0), (0, 0, 1, 0)):
            assert found[key][0] <= 128, (key, found[key])


def test_the_new_source_holds_no_forbidden_instruction(monkeypatch):
    # test_nee_pass_isa's own check, list and all, pointed at this file and this file's assembly
    real_open = open
    monkeypatch.setattr(test_nee_pass_isa, "pass_kernels", stream_kernels)
    redirect = {os.path.join(CSRC, n): SRC for n in ("rt_nee_pass_kernel.hip", "rt_nee_kernel.hip")}
    monkeypatch.setattr(test_nee_pass_isa, "open", lambda path, *a, **kw: real_open(redirect.get(path, path), *a, **kw), raising=False)
    test_nee_pass_isa.test_the_new_sources_hold_no_forbidden_instruction()


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_the_other_kernel_files_hold_no_stream_code(flavour):
    for kernel in ("pool", "v1"):
        assert "k_nee_stream" not in kernel_asm.asm_text(kernel, flavour)
    assert "k_nee_stream" not in test_nee_pass_isa.pass_kernels(flavour)[1]
