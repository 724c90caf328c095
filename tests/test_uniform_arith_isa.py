"""Wave-uniform integer arithmetic of the pooled trace kernel stays in the scalar unit, and there is less of it: pinned
in the GENERATED CODE (CPU test: hipcc cross-compiles gfx950 without a GPU; tests/kernel_asm.py).

  * No 64-bit integer compare whose sources are all scalar registers or constants sits in the vector stream.  The
    cooperative samplers' request count comes from a 64-bit bit count; compared as the 64-bit value the compiler makes of
    it, every `n > 32`, `n > 16`, ... is a `v_cmp_gt_u64 sN, s[..], imm` (the scalar unit has no ordered 64-bit compare)
    with an `s_and_b64 vcc, exec, ..` and a branch behind it: 13 of them in `<0,0,0,0>` before rt_pool_groups.h, about four
    executed per path-loop iteration.  Checked in both flavours of `<0,0,0,0>`, `<1,0,0,0>` and `<1,1,1,0>`.
  * The static count of scalar instructions of the fast `<0,0,0,0>` (every `s_*` but branches, `s_waitcnt` and `s_nop`) is
    strictly below the parent commit's 863, counted by the same rule with the same compiler (the tree: 824)."""
import re

import pytest

import kernel_asm

VARIANTS = ["Li0ELb0ELb0ELb0E", "Li1ELb0ELb0ELb0E", "Li1ELb1ELb1ELb0E"]
PARENT_SCALAR_C3 = 863


def kernel_instructions(text, flavour, variant):
    start = text.index("\n_ZN%drtdev_%s16k_trace_pool_f64I%s" % (len("rtdev_" + flavour), flavour, variant))
    body = text[start:text.index(".Lfunc_end", start)]
    ops = [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith(".")]
    return [o for o in ops if not o.startswith(";")]


def uniform_u64_compares(ops):
    """64-bit integer vector compares none of whose sources is a vector register."""
    found = []
    for o in ops:
        m = re.match(r"v_cmpx?_\w+_[ui]64(?:_e32|_e64)?\s+(.*)$", o)
        if m:
            sources = [s.strip() for s in m.group(1).split(",")][1:]  # (the first operand is the destination mask)
            if not any(re.match(r"v\d+$|v\[\d+:\d+\]$", s) for s in sources):
                found.append(o)
    return found


def scalar_instructions(ops):
    return [o for o in ops if o.startswith("s_") and not o.startswith(("s_branch", "s_cbranch", "s_waitcnt", "s_nop"))]


@pytest.fixture(scope="module", params=sorted(kernel_asm.FLAVOURS))
def flavour_text(request):
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    return request.param, kernel_asm.asm_text("pool", request.param)


def test_the_rule_finds_the_compare_it_is_about():
    ops = ["v_cmp_gt_u64_e64 s[2:3], s[0:1], 32", "v_cmp_lt_u64_e32 vcc, s[4:5], v[2:3]", "v_cmp_ne_u64_e32 vcc, 0, v[8:9]",
           "v_cmp_gt_u32_e32 vcc, s20, v4", "v_cmp_lt_u64_e64 vcc, s[6:7], 8"]
    assert uniform_u64_compares(ops) == [ops[0], ops[4]]
    assert len(scalar_instructions(["s_add_i32 s0, s0, 1", "s_cbranch_scc1 .LBB0_1", "s_waitcnt lgkmcnt(0)", "s_nop 0",
                                    "s_load_dwordx2 s[0:1], s[2:3], 0x0", "v_mov_b32_e32 v0, s0", "s_branch .LBB0_2"])) == 2


@pytest.mark.parametrize("variant", VARIANTS)
def test_no_vector_compare_of_scalar_u64(flavour_text, variant):
    flavour, text = flavour_text
    found = uniform_u64_compares(kernel_instructions(text, flavour, variant))
    print(flavour, variant, found)
    assert found == []


def test_the_group_size_is_a_count_of_leading_zeros(flavour_text):
    flavour, text = flavour_text
    for variant in VARIANTS:
        assert any(o.startswith("s_flbit_i32_b32") for o in kernel_instructions(text, flavour, variant)), (flavour, variant)


def test_fewer_scalar_instructions_than_the_parent():
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    got = len(scalar_instructions(kernel_instructions(kernel_asm.asm_text("pool", "fast"), "fast", VARIANTS[0])))
    print("scalar instructions of the fast <0,0,0,0>:", got, "parent:", PARENT_SCALAR_C3)
    assert got < PARENT_SCALAR_C3, got
