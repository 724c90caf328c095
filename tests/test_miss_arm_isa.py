"""The miss arm of the path loop in the rects-only plain variant of k_trace_pool_f64, in the GENERATED CODE of the fast
flavour (CPU test: hipcc cross-compiles gfx950 without a GPU).

One or two lanes of 64 leave the scene in almost every iteration, and a wave instruction costs the same for two lanes as
for 64.  So with a black solid background (TraceArgs.bg_black) the arm is a scalar load, a compare and a branch to the
additions of the other ended lanes: no vector instruction.  With any other solid background it is three v_mul_f64 that
take the colour as a scalar operand and write the throughput's own registers; the sky arm does the same with the colour
it forms.  Before, the two kinds formed their products in temporaries and three v_mov_b64 copied them into the throughput
where the arms joined, in every iteration, products with a black background's zeros included.

The arm is found by the flag's own load (its offset comes from tests/background_flag_driver.cpp) and ends at the
additions into the pixel's sum.  This counts only what that change removed."""
import os
import re
import shutil
import subprocess

import pytest

import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def flag_offset(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("miss_arm") / "background_flag_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "racer-tracer_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "background_flag_driver.cpp")], check=True)
    return int(subprocess.run([exe, "layout"], check=True, capture_output=True, text=True).stdout.split()[0])


@pytest.fixture(scope="module")
def miss_arm(flag_offset):
    """The instructions from the load of TraceArgs.bg_black to the first addition into a pixel's sum behind it, and the
    registers of the three terms added there (the throughput's)."""
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    text = kernel_asm.asm_text("pool", "fast")
    start = text.index("\n_ZN10rtdev_fast16k_trace_pool_f64ILi0ELb0ELb0ELb0E")
    body = text[start:text.index(".Lfunc_end", start)]
    ops = [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    loads = [i for i, o in enumerate(ops) if re.match(r"s_load_dword s\d+, s\[\d+:\d+\], 0x%x$" % flag_offset, o)]
    assert len(loads) == 1, loads       # the path loop reads the flag in one place, and nothing else does
    end = next(i for i in range(loads[0], len(ops)) if ops[i].startswith("ds_add_f64"))
    assert all(o.startswith("ds_add_f64") for o in ops[end:end + 3])
    return ops[loads[0]:end], [re.match(r"ds_add_f64 v\d+, (v\[\d+:\d+\])", o).group(1) for o in ops[end:end + 3]]


def test_the_arm_copies_nothing(miss_arm):
    miss_arm, _ = miss_arm
    assert not any(o.startswith("v_mov_b64") for o in miss_arm), miss_arm


def test_a_solid_colour_is_three_products_with_scalar_operands_in_place(miss_arm):
    miss_arm, throughput = miss_arm
    assert len(set(throughput)) == 3
    for reg in throughput:
        assert any(re.match(r"v_mul_f64 %s, %s, s\[\d+:\d+\]$" % (re.escape(reg), re.escape(reg)), o) for o in miss_arm), (reg, miss_arm)


def test_a_black_background_reaches_the_additions_without_a_vector_instruction(miss_arm):
    """From the flag's load to the scalar branch that tests it: scalar instructions, and at most the ballot of `best < 0`,
    which the compiler schedules among them (the lanes that miss still end).  The flag is tested before anything is
    multiplied."""
    miss_arm, _ = miss_arm
    branch = next(i for i, o in enumerate(miss_arm) if o.startswith("s_cbranch_scc"))
    assert any(o.startswith("s_cmp_") for o in miss_arm[:branch])
    vector = [o for o in miss_arm[:branch] if o.startswith(("v_", "ds_", "global_", "buffer_", "flat_"))]
    assert all(o.startswith("v_cmp_") for o in vector) and len(vector) <= 1, vector
