"""The NEE kernel (csrc/rt_nee_kernel.hip) compiled for gfx950 in both arithmetic flavours, as the library builds it:
every k_nee_f64 instantiation is there, the linear-loop ones use no scratch memory and none spills, and the plain trace
kernels' files hold no NEE code (their inventories, tests/kernel_asm.py, are pinned by test_variant_matrix.py)."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

import kernel_asm

SRC = os.path.join(kernel_asm.ROOT, "racer-tracer_amd", "csrc", "rt_nee_kernel.hip")
_KERNEL = re.compile(r"\.amdhsa_kernel _ZN\d+rtdev_(fast|exact)\d+k_nee_f64ILi(\d)ELb([01])ELb([01])ELb([01])EE\w*\n(.*?)"
                     r"\.end_amdhsa_kernel", re.S)


@functools.lru_cache(maxsize=None)
def nee_kernels(flavour):
    out = os.path.join(tempfile.mkdtemp(prefix="rt_nee_asm_"), "nee_%s.s" % flavour)
    cmd = [kernel_asm.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"] + \
        kernel_asm.FLAVOURS[flavour] + [SRC, "-o", out]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    found = {}
    for m in _KERNEL.finditer(open(out).read()):
        assert m.group(1) == flavour
        body = m.group(6)
        found[tuple(int(m.group(k)) for k in (2, 3, 4, 5))] = (
            int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
            int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))
    return found


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_every_instantiation_is_compiled(flavour):
    # PRIMS x TEXTURED x SPECULAR for the linear loop, TEXTURED x SPECULAR for the BVH walk (PRIMS_ANY)
    want = {(p, t, s, 0) for p in (0, 1, 2) for t in (0, 1) for s in (0, 1)} | {(2, t, s, 1) for t in (0, 1) for s in (0, 1)}
    assert set(nee_kernels(flavour)) == want


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_registers_and_scratch(flavour):
    for key, (vgprs, scratch) in nee_kernels(flavour).items():
        assert vgprs <= 256, (key, vgprs)  # no spill: the whole path state stays in registers
        if key[3] == 0:  # the linear-loop variants: no scratch at all
            assert scratch == 0, (key, scratch)
    # the plain-colour linear variants (cornell_box's and the shipped rect / sphere scenes') fit 128 VGPRs
    kernels = nee_kernels(flavour)
    for key in ((0, 0, 0, 0), (0, 0, 1, 0)):
        assert kernels[key][0] <= 128, (key, kernels[key])


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_the_plain_kernel_files_hold_no_nee_code(flavour):
    for kernel in ("pool", "v1"):
        text = kernel_asm.asm_text(kernel, flavour)
        assert "k_nee_f64" not in text
        assert kernel_asm.inventory(kernel, flavour)
