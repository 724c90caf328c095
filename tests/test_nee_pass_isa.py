"""The pass form of the NEE kernel (csrc/rt_nee_pass_kernel.hip) compiled for gfx950 in both arithmetic flavours, as the
library builds it: every k_nee_pass_f64 instantiation is there, the linear-loop ones use no scratch memory, each sits in the
occupancy step of k_nee_f64 of the same key and flavour (or a better one), the new sources hold none of the instructions
that are off limits, and the plain trace kernels' files hold no NEE code."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

import kernel_asm
import test_nee_isa

CSRC = os.path.join(kernel_asm.ROOT, "racer-tracer_amd", "csrc")
SRC = os.path.join(CSRC, "rt_nee_pass_kernel.hip")
_KERNEL = re.compile(r"\.amdhsa_kernel _ZN\d+rtdev_(fast|exact)\d+k_nee_pass_f64ILi(\d)ELb([01])ELb([01])ELb([01])EE\w*\n(.*?)"
                     r"\.end_amdhsa_kernel", re.S)


@functools.lru_cache(maxsize=None)
def pass_kernels(flavour):
    out = os.path.join(tempfile.mkdtemp(prefix="rt_nee_pass_asm_"), "nee_pass_%s.s" % flavour)
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


def waves_per_simd(vgprs):
    """gfx950: 512 VGPRs per SIMD lane, allocated in granules of 8: 4 waves up to 128, 3 up to 168, 2 up to 256."""
    allocated = (vgprs + 7) // 8 * 8
    assert allocated <= 256, vgprs
    return 4 if allocated <= 128 else 3 if allocated <= 168 else 2


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_every_instantiation_is_compiled(flavour):
    want = {(p, t, s, 0) for p in (0, 1, 2) for t in (0, 1) for s in (0, 1)} | {(2, t, s, 1) for t in (0, 1) for s in (0, 1)}
    found, text = pass_kernels(flavour)
    assert set(found) == want
    assert "k_nee_decide_f64" in text and "k_nee_chunk_f64" in text
    assert "k_nee_f64" not in text.replace("k_nee_pass_f64", "")  # a kernel of its own, in a file of its own


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_scratch_and_occupancy_step(flavour):
    found, _ = pass_kernels(flavour)
    one_shot = test_nee_isa.nee_kernels(flavour)
    for key, (vgprs, scratch) in sorted(found.items()):
        print(flavour, key, "k_nee_pass_f64 %d VGPRs, %d B scratch; k_nee_f64 %d VGPRs" % (vgprs, scratch, one_shot[key][0]))
        if key[3] == 0:  # the linear-loop variants: no scratch at all
            assert scratch == 0, (key, scratch)
        # compared in the same compile, not against a fixed number: no variant may lose a wave per SIMD to the pass form
        assert waves_per_simd(vgprs) >= waves_per_simd(one_shot[key][0]), (key, vgprs, one_shot[key][0])


def test_the_new_sources_hold_no_forbidden_instruction():
    words = ["s_" + "store_", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic_", "s_buffer_" + "atomic", "s_dcache_" + "wb",
             "s_dcache_" + "discard"]
    for name in ("rt_nee_pass_kernel.hip", "rt_nee_common.h", "rt_nee_kernel.hip"):
        text = open(os.path.join(CSRC, name)).read().lower()
        for w in words:
            assert w not in text, (name, w)
        assert "asm" not in text.replace("kernel_asm", ""), name  # no inline assembly at all
    for flavour in ("fast", "exact"):
        asm = pass_kernels(flavour)[1].lower()
        for w in words:
            assert w not in asm, (flavour, w)


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_the_plain_kernel_files_hold_no_nee_code(flavour):
    for kernel in ("pool", "v1"):
        text = kernel_asm.asm_text(kernel, flavour)
        assert "k_nee_" not in text
