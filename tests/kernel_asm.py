"""Device assembly of the trace kernels, compiled once per test session (hipcc cross-compiles gfx950 without a GPU):
shared by tests/test_kernel_isa.py and tests/test_variant_matrix.py."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SOURCES = {"pool": "rt_trace_pool_kernel.hip", "v1": "rt_trace_kernel.hip", "multihit": "rt_multihit_kernel.hip"}
# the Makefile's EXACT_FLAGS: the RT_ARITH_REFERENCE copy of the trace kernels
FLAVOURS = {"fast": [], "exact": ["-DRT_EXACT_DIV", "-ffp-contract=off"]}


def hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


@functools.lru_cache(maxsize=None)
def asm_text(kernel, flavour):
    """The gfx950 assembly of csrc/<SOURCES[kernel]> in one flavour, as text."""
    out = os.path.join(tempfile.mkdtemp(prefix="rt_asm_"), "%s_%s.s" % (kernel, flavour))
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"] + FLAVOURS[flavour] + [
        os.path.join(ROOT, "racer-tracer_amd", "csrc", SOURCES[kernel]), "-o", out]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    return open(out).read()


_TRACE = re.compile(r"\.amdhsa_kernel _ZN\d+rtdev_(fast|exact)\d+k_trace(?:_pool)?_f64ILi(\d)E((?:Lb[01]E)+)E\w*\n(.*?)\.end_amdhsa_kernel", re.S)


def inventory(kernel, flavour):
    """The trace-kernel instantiations in the compiled code: {(prims, textured, specular, bvh): static LDS bytes};
    bvh is 0 for the v1 kernel, which has no BVH parameter."""
    found = {}
    for m in _TRACE.finditer(asm_text(kernel, flavour)):
        assert m.group(1) == flavour
        flags = [int(b) for b in re.findall(r"Lb([01])E", m.group(3))]
        assert len(flags) == (3 if kernel == "pool" else 2), m.group(0)[:200]
        key = (int(m.group(2)), flags[0], flags[1], flags[2] if kernel == "pool" else 0)
        found[key] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(4)).group(1))
    return found
