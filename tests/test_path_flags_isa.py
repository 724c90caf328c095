"""The path loop's lane flags in the plain variants of k_trace_pool_f64, pinned in the GENERATED CODE (CPU test: hipcc
cross-compiles gfx950 without a GPU).

`alive`, `waiting` and the per-iteration `ended`, `scattered`, `finish` are wave-uniform 64-bit masks that live in SGPR
pairs (LABNOTES R9): they are combined in the scalar unit, branches run under `inverse_ballot(mask)`, and where a branch
decides one of them it leaves per-lane data behind (`best`, the material's kind) whose comparison is balloted after the
lanes have joined.  As per-lane bools every test of one of them was `v_cndmask_b32 v, 0, 1, mask` + `v_cmp_ne_u32 mask',
0, v`, and every assignment at a join another `v_cndmask_b32 0/1`, each as dear as an f64 fma.

Static counts of the whole kernel, the parent commit's against this tree's (same compiler, the flags of kernel_asm.py):

                                                   <0,0,0,0>          <1,0,0,0>
                                                parent   tree      parent   tree
  A  bool_to_mask_pairs                            8       4          8       4
  B  v_cndmask_b32 v, 0, +-1, mask                15      11         15      11
     v_readlane_b32                               29      29         32      31
     v_writelane_b32                              19      19         22      21

(The issue that asked for this quotes 7 pairs for the parent's <0,0,0,0>; this compiler gives 8.  The bounds below are
the tree's counts, under either figure.)  The lane reads and writes all sit in item code, outside the path loop: no mask
of the path loop was parked in a VGPR lane.  What is left of A and B: the item code's and the camera batches' ballots,
the sampler's `base` increments (a 0/1 select in each form of a round, ONE add behind their join), and the masked
direction write."""
import re

import pytest

import kernel_asm

# variant -> (A, B, v_readlane_b32, v_writelane_b32) of this tree, and the parent's for the strict comparisons
TREE = {"Li0ELb0ELb0ELb0E": (4, 11, 29, 19), "Li1ELb0ELb0ELb0E": (4, 11, 31, 21)}
PARENT = {"Li0ELb0ELb0ELb0E": (8, 15, 29, 19), "Li1ELb0ELb0ELb0E": (8, 15, 32, 22)}
ISSUE_PARENT_C3 = (7, 15, 29, 19)  # the figures the issue quotes for <0,0,0,0>


@pytest.fixture(scope="module")
def pool_fast_text():
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    return kernel_asm.asm_text("pool", "fast")


def kernel_instructions(text, variant):
    start = text.index("\n_ZN10rtdev_fast16k_trace_pool_f64I" + variant)
    body = text[start:text.index(".Lfunc_end", start)]
    ops = [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith(".")]
    return [o for o in ops if not o.startswith(";")]


def bool_to_mask_pairs(ops):
    """`v_cndmask_b32 vN, 0, 1, <mask>` followed within three instructions by `v_cmp_ne_u32 <mask'>, 0, vN`."""
    n = 0
    for i, l in enumerate(ops):
        m = re.match(r"v_cndmask_b32_e64 (v\d+), 0, 1, ", l)
        if m and any(re.match(r"v_cmp_ne_u32_e(32|64) \S+, 0, " + m.group(1) + "$", x) for x in ops[i + 1:i + 4]):
            n += 1
    return n


def mask_to_integer_selects(ops):
    """`v_cndmask_b32 vN, 0, 1, <mask>` and `v_cndmask_b32 vN, 0, -1, <mask>`: a lane mask turned into a per-lane integer."""
    return sum(1 for o in ops if re.match(r"v_cndmask_b32_e(32|64) v\d+, 0, -?1, ", o))


def test_bounds_are_below_the_parent():
    for variant, (a, b, rl, wl) in TREE.items():
        pa, pb, prl, pwl = PARENT[variant]
        assert a < pa and b < pb and rl <= prl and wl <= pwl, variant
    a, b, rl, wl = TREE["Li0ELb0ELb0ELb0E"]
    ia, ib, irl, iwl = ISSUE_PARENT_C3
    assert a < ia and b < ib and rl <= irl and wl <= iwl


@pytest.mark.parametrize("variant", sorted(TREE))
def test_count_a_bools_turned_into_masks(pool_fast_text, variant):
    got = bool_to_mask_pairs(kernel_instructions(pool_fast_text, variant))
    print("bool_to_mask_pairs", variant, got)
    assert got <= TREE[variant][0], got


@pytest.mark.parametrize("variant", sorted(TREE))
def test_count_b_masks_turned_into_integers(pool_fast_text, variant):
    got = mask_to_integer_selects(kernel_instructions(pool_fast_text, variant))
    print("v_cndmask_b32 0, +-1", variant, got)
    assert got <= TREE[variant][1], got


@pytest.mark.parametrize("variant", sorted(TREE))
def test_lane_traffic(pool_fast_text, variant):
    ops = kernel_instructions(pool_fast_text, variant)
    reads = sum(1 for o in ops if o.startswith("v_readlane_b32"))
    writes = sum(1 for o in ops if o.startswith("v_writelane_b32"))
    print("v_readlane_b32 / v_writelane_b32", variant, reads, writes)
    assert reads <= TREE[variant][2] and writes <= TREE[variant][3], (reads, writes)
