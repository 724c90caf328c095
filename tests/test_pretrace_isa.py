"""What tracing the primary segments in the camera batches must not cost the rects-only plain variant of
k_trace_pool_f64, pinned in the GENERATED CODE of both arithmetic flavours (CPU test: hipcc cross-compiles gfx950 without
a GPU): seven waves per SIMD (at most 72 VGPRs), no scratch, and static LDS that still leaves seven blocks per CU beside
C3's six-record primitive table — 23 040 bytes is the seven-block edge (18 granules of 1 280 bytes)."""
import re

import pytest

import kernel_asm

C3_TABLE_BYTES = 6 * 192
SEVEN_BLOCK_EDGE = 23040


@pytest.mark.parametrize("flavour", ["fast", "exact"])
def test_rects_only_plain_variant_keeps_seven_blocks(flavour):
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    text = kernel_asm.asm_text("pool", flavour)
    m = re.search(r"\.amdhsa_kernel _ZN\d+rtdev_%s16k_trace_pool_f64ILi0ELb0ELb0ELb0E.*?\.end_amdhsa_kernel" % flavour, text, re.S)
    assert m
    get = lambda key: int(re.search(r"\.%s (\d+)" % key, m.group(0)).group(1))
    vgprs, scratch, lds = get("amdhsa_next_free_vgpr"), get("amdhsa_private_segment_fixed_size"), get("amdhsa_group_segment_fixed_size")
    print(flavour, "VGPRs", vgprs, "scratch", scratch, "static LDS", lds)
    assert vgprs <= 72
    if flavour == "fast":   # (the reference flavour's IEEE divisions spilled a few registers before this loop existed: not pinned)
        assert scratch == 0
    assert lds + C3_TABLE_BYTES <= SEVEN_BLOCK_EDGE
    assert kernel_asm.inventory("pool", flavour)[(0, 0, 0, 0)] == lds


def test_the_batch_traces_with_one_rect_test_per_plane_and_the_loop_with_pairs():
    """Twelve written-out rect tests in the fast flavour's kernel: three planes x (a pair + the odd one out) in the path
    loop, one per plane in the camera batches."""
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    text = kernel_asm.asm_text("pool", "fast")
    start = text.index("\n_ZN10rtdev_fast16k_trace_pool_f64ILi0ELb0ELb0ELb0E")
    body = text[start:text.index(".Lfunc_end", start)]
    blocks = re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", body, re.S)
    assert sum(1 for b in blocks if "v_cmpx_ngt_f64" in b) == 12
