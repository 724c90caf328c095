"""The glue of the path loop in the plain variants of k_trace_pool_f64, pinned in the GENERATED CODE (CPU test: hipcc
cross-compiles gfx950 without a GPU).  C3 (`<0,0,0,0>`) is bound by vector issue, and the forms below are what took
vector instructions out of every iteration without changing a value (LABNOTES R6):
  * a ballot of a `bool` that is not a comparison of the same block costs `v_cndmask_b32 v, 0, 1, mask` +
    `v_cmp_ne_u32 mask', 0, v`; the sampler's accepted / pending masks and the near-zero test ballot comparisons and
    AND the masks in the scalar unit instead,
  * the sampler's request is posted as four 32-bit LDS stores, so pixel, sample, segment and candidate need not sit in
    four consecutive VGPRs (which cost copies in every iteration),
  * the Lambertian direction is formed in the registers of `d` itself (the rects-only variant recovers the normal in the
    1e-23 case that needs it), so no copy of the new direction is made at the join."""
import re

import pytest

import kernel_asm

PLAIN = ("Li0ELb0ELb0ELb0E", "Li1ELb0ELb0ELb0E")  # rects-only (C3), spheres-only


@pytest.fixture(scope="module")
def pool_fast_text():
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    return kernel_asm.asm_text("pool", "fast")


def kernel_ops(text, variant):
    start = text.index("\n_ZN10rtdev_fast16k_trace_pool_f64I" + variant)
    body = text[start:text.index(".Lfunc_end", start)]
    return [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith(".")]


def instructions(ops):
    return [o for o in ops if not o.startswith(";")]


def bool_to_mask_pairs(ops):
    """`v_cndmask_b32 vN, 0, 1, <mask>` followed within three instructions by `v_cmp_ne_u32 <mask'>, 0, vN`."""
    n = 0
    for i, l in enumerate(ops):
        m = re.match(r"v_cndmask_b32_e64 (v\d+), 0, 1, ", l)
        if m and any(re.match(r"v_cmp_ne_u32_e(32|64) \S+, 0, " + m.group(1) + "$", x) for x in ops[i + 1:i + 4]):
            n += 1
    return n


@pytest.mark.parametrize("variant", PLAIN)
def test_few_bools_turned_into_masks(pool_fast_text, variant):
    ops = instructions(kernel_ops(pool_fast_text, variant))
    # 13 before the sampler's and the near-zero ballots took comparisons; what is left are ballots of the loop-carried
    # path flags and the item code's
    assert bool_to_mask_pairs(ops) <= 8, bool_to_mask_pairs(ops)


def test_rects_only_variant_copies(pool_fast_text):
    """64-bit register copies in the whole rects-only kernel (static count; the rect tests' `best_t` updates included):
    64 before the request stores and the in-place Lambertian direction."""
    ops = instructions(kernel_ops(pool_fast_text, "Li0ELb0ELb0ELb0E"))
    assert sum(1 for o in ops if o.startswith("v_mov_b64")) <= 57


@pytest.mark.parametrize("variant", PLAIN)
def test_sampler_request_is_four_32_bit_stores(pool_fast_text, variant):
    ops = instructions(kernel_ops(pool_fast_text, variant))
    groups = 0
    for i in range(len(ops) - 3):
        quad = [re.match(r"ds_write_b32 (v\d+), v\d+(?: offset:(\d+))?$", o) for o in ops[i:i + 4]]
        if all(quad) and len({m.group(1) for m in quad}) == 1:
            offs = [int(m.group(2) or 0) for m in quad]
            groups += offs == [offs[0] + 4 * k for k in range(4)]
    assert groups >= 2, groups  # the sphere sampler's one store site in each of its two unrolled rounds


@pytest.mark.parametrize("variant", PLAIN)
def test_near_zero_test_is_three_compares_and_no_select(pool_fast_text, variant):
    ops = kernel_ops(pool_fast_text, variant)
    at = next(i for i, o in enumerate(ops) if "near_zero" in o)
    before = instructions(ops[max(0, at - 16):at])
    assert sum(1 for o in before if o.startswith("v_cmp_lt_f64") and "|" in o) == 3, before
    assert not any(o.startswith("v_cndmask_b32") for o in before), before
    # the three masks are ANDed and tested in the scalar unit: one branch around the rare arm, none between the compares
    first = next(i for i, o in enumerate(before) if o.startswith("v_cmp_lt_f64"))
    assert sum(1 for o in before[first:] if o.startswith("s_cbranch")) <= 1, before
