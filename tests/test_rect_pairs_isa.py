"""The pair loop of the rects-only plain variant steps over a facing pair's second rect test (rt_pool_coop.h:
closest_hit_rects<true>, rt_rect_pairs.h), pinned in the GENERATED CODE (CPU test: hipcc cross-compiles gfx950 without a GPU).

Fast flavour, `<0,0,0,0>`: the written-out rect tests are still twelve (three in the camera batches, nine in the path loop:
a pair's two and the odd record's, per plane); between a pair's first and second test lies a scalar conditional branch
whose target lies behind the second; the first test of a pair takes k and the index from vector registers, every other
test from scalar ones; and the selection in front of it is the handful of instructions rt_rect_pairs.h counts on — no
64-bit comparison of scalars, no select between scalars (v_cndmask_b32), no integer multiply.

The reference flavour (RT_EXACT_DIV) has no pair form: nothing of it in its kernel's text (its instruction stream is the
parent commit's, shown once in profiles/r21_pool_kernel_asm_compare.txt)."""
import re

import pytest

import kernel_asm


def _body(flavour):
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    text = kernel_asm.asm_text("pool", flavour)
    ns = "_ZN10rtdev_fast" if flavour == "fast" else "_ZN11rtdev_exact"
    start = text.index("\n%s16k_trace_pool_f64ILi0ELb0ELb0ELb0E" % ns)
    return text[start:text.index(".Lfunc_end", start)]


def _rect_tests(body):
    return [m for m in re.finditer(r";;#ASMSTART\n(.*?);;#ASMEND", body, re.S) if "v_cmpx_ngt_f64" in m.group(1)]


def test_twelve_rect_tests_and_a_branch_over_each_pairs_second():
    body = _body("fast")
    tests = _rect_tests(body)
    assert len(tests) == 12
    for plane in range(3):
        first, second = tests[3 + 3 * plane], tests[4 + 3 * plane]
        between = body[first.end():second.start()]
        branches = re.findall(r"\ts_cbranch_(?:scc[01]|vccn?z)\s+(\.LBB\d+_\d+)", between)
        print("plane", plane, "branches between the pair's tests:", branches)
        assert branches
        targets = [body.index("\n%s:" % label) for label in branches]
        assert any(t >= second.end() for t in targets)      # ... and forward, past the second test (its label may follow at once)


def test_only_a_pairs_first_test_takes_k_and_the_index_per_lane():
    tests = _rect_tests(_body("fast"))
    per_lane = []
    for n, m in enumerate(tests):
        ops = [l.strip() for l in m.group(1).split("\n") if l.strip()]
        k_vector = re.match(r"v_add_f64 v\[\d+:\d+\], v\[\d+:\d+\], -v\[\d+:\d+\]", ops[0]) is not None
        i_vector = re.match(r"v_mov_b32 v\d+, v\d+", [o for o in ops if o.startswith("v_mov_b32")][0]) is not None
        assert k_vector == i_vector, ops
        if k_vector:
            per_lane.append(n)
    assert per_lane == [3, 6, 9]


def test_the_selection_is_a_handful_of_instructions():
    """From the request of the pair's scalars to the pair's first test: one shift (written out), an AND, an add and a
    subtract on addresses, three LDS reads, the two operations of t_other and one comparison."""
    body = _body("fast")
    spans = re.findall(r"; pair requested\n(.*?);;#ASMSTART\n\tv_add_f64", body, re.S)
    assert len(spans) == 3
    for span in spans:
        ops = [l.strip().split()[0] for l in span.split("\n") if l.startswith("\t") and l.strip() and not l.strip().startswith((";", "."))]
        vector = [o for o in ops if o.startswith("v_")]
        print(vector, [o for o in ops if o.startswith("ds_")])
        assert not [o for o in vector if o.startswith(("v_cndmask", "v_mul_lo", "v_mul_hi", "v_mad_u64")) or re.match(r"v_cmp_\w+_[ui]64", o)]
        assert sum(o.startswith("ds_read") for o in ops) == 3
        assert sum(o.startswith("v_cmp") for o in vector) == 1
        # the plain case's moves of k and the index into vector registers come on top, once or twice (a copy per arm)
        assert len([o for o in vector if not o.startswith("v_mov")]) <= 8, vector


def test_the_reference_flavour_has_no_pair_form():
    body = _body("exact")
    assert "; pair requested" not in body and "; facing pair" not in body and "; both records" not in body
    assert not _rect_tests(body)
