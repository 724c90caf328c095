"""The hand-out of the rects-only plain variant of k_trace_pool_f64 loads the point of the primary hit and computes
nothing, pinned in the GENERATED CODE of both arithmetic flavours (CPU test: hipcc cross-compiles gfx950 without a GPU).

A camera batch forms the point of every entry that lives on, with the expression the path loop uses behind its own
closest-hit loop (rt_trace_common.h: ray_at), and stores it in the ring; the lane that takes an entry reads it back with
the pool index and the `best` word.  The source brackets the taking branch and the two uses of ray_at with assembly
comments (`; hand_out_begin` / `; hand_out_end`, `; hit_point_begin` / `; hit_point_end`), as `; near_zero` marks its
branch; the brackets are tied to the values they enclose, so the instructions between them are the ones meant."""
import re

import pytest

import kernel_asm

PARENT_STATIC_LDS = 20096      # what the block had before the ring carried points: 64 bytes more cost the profile build a block per CU
F64_ARITHMETIC = re.compile(r"v_(fma|fmac|mul|add)_f64")


def _body(flavour):
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    text = kernel_asm.asm_text("pool", flavour)
    ns = "_ZN10rtdev_fast" if flavour == "fast" else "_ZN11rtdev_exact"
    start = text.index("\n%s16k_trace_pool_f64ILi0ELb0ELb0ELb0E" % ns)
    return text[start:text.index(".Lfunc_end", start)]


def _instructions(text):
    ops = [l.strip() for l in text.split("\n") if l.startswith("\t") and not l.strip().startswith(".")]
    return [o for o in ops if not o.startswith(";")]


def _between(body, begin, end):
    """The instructions of every `; begin` ... `; end` bracket of the kernel, and where each bracket starts."""
    found = [(m.start(), _instructions(m.group(1))) for m in re.finditer(r"; %s\n(.*?); %s\n" % (begin, end), body, re.S)]
    assert all("; %s" % begin not in "\n".join(ops) for _, ops in found)
    return found


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_static_lds_is_not_above_the_parents(flavour):
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    lds = kernel_asm.inventory("pool", flavour)[(0, 0, 0, 0)]
    print(flavour, "static LDS", lds)
    assert lds <= PARENT_STATIC_LDS


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_the_hand_out_loads_and_does_not_compute(flavour):
    brackets = _between(_body(flavour), "hand_out_begin", "hand_out_end")
    assert len(brackets) == 1
    ops = brackets[0][1]
    print(flavour, len(ops), "instructions in the taking branch:", ops)
    assert not [o for o in ops if F64_ARITHMETIC.match(o)]       # no camera ray, no o + t * d
    assert not [o for o in ops if o.startswith("s_load")]        # no camera vector, no lens flag: nothing of the kernel arguments
    assert not [o for o in ops if o.startswith("s_cbranch")]     # (no branch on an aperture either)
    reads = [o for o in ops if o.startswith("ds_read")]
    assert 0 < len(reads) <= 4                                   # the point's three doubles and the `best` word (the pool index is read by every lane, in front)


def test_the_point_is_formed_behind_the_last_rect_test_and_in_the_batch():
    """Fast flavour: ray_at is three fma.  Once behind the path loop's last rect test (the loop's nine written-out tests
    follow the batches' three in the kernel's text), once in the camera batch, behind the batches' last."""
    body = _body("fast")
    brackets = _between(body, "hit_point_begin", "hit_point_end")
    assert len(brackets) == 2
    for _, ops in brackets:
        fma = [o for o in ops if re.match(r"v_fmac?_f64", o)]
        print(ops)
        assert len(fma) == 3
        assert not [o for o in ops if F64_ARITHMETIC.match(o) and o not in fma]
    rect_tests = [m.end() for m in re.finditer(r";;#ASMSTART\n(.*?);;#ASMEND", body, re.S) if "v_cmpx_ngt_f64" in m.group(1)]
    assert len(rect_tests) == 12
    (in_batch, _), (in_loop, _) = brackets
    assert rect_tests[2] < in_batch < rect_tests[3]      # behind the batch's three tests, in front of the loop's first
    assert in_loop > rect_tests[11]                      # behind the loop's last
    # ... and directly behind it: nothing but the segment counter and scalar bookkeeping in between
    gap = _instructions(body[rect_tests[11]:in_loop])
    assert not [o for o in gap if F64_ARITHMETIC.match(o) or o.startswith("ds_") or o.startswith("s_cbranch")], gap


def test_the_reference_flavour_keeps_the_product_and_the_sum():
    """RT_ARITH_REFERENCE: no contraction — three multiplications and three additions, in both places."""
    brackets = _between(_body("exact"), "hit_point_begin", "hit_point_end")
    assert len(brackets) == 2
    for _, ops in brackets:
        assert sum(1 for o in ops if o.startswith("v_mul_f64")) == 3 and sum(1 for o in ops if o.startswith("v_add_f64")) == 3
        assert not [o for o in ops if re.match(r"v_fmac?_f64", o)]
