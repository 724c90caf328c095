"""The random_in_unit_sphere candidate's bit assembly (rt_trace_common.h: sphere_candidate / sym42_bits), pinned twice
(CPU tests: numpy, and hipcc cross-compiling gfx950 without a GPU):
  * a numpy model of the v_alignbit_b32 form gives, over edge and random words, the very bits of rt_rng.h's formula
    u42(w, t) = (w << 10 | t & 0x3FF) * 2^-42, coordinate -1 + 2 u42 — so the frame cannot change;
  * the compiled trace kernels place the high words with v_alignbit_b32 (0x400:w >> 12), not with a shift and an OR of
    0x40000000 (the inline constant 2.0): one vector instruction per coordinate, three per candidate."""
import re

import numpy as np
import pytest

import kernel_asm

M32 = np.uint64(0xFFFFFFFF)


def alignbit(hi, lo, s):
    """v_alignbit_b32: the low 32 bits of (hi:lo) >> s."""
    return ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(s) & M32


def new_bits(a, b, c, d):
    """sphere_candidate's three 64-bit patterns, as rt_trace_common.h assembles them."""
    u = lambda x: x.astype(np.uint64)
    hi = lambda w: alignbit(np.full_like(w, 0x400), w, 12)
    lo = [alignbit(a, (u(d) << np.uint64(22)) & M32, 12),
          ((u(b) << np.uint64(20)) & M32) | (u(d) & np.uint64(0x000FFC00)),
          ((u(c) << np.uint64(20)) & M32) | ((u(d) >> np.uint64(10)) & np.uint64(0x000FFC00))]
    return [(hi(w) << np.uint64(32)) | l for w, l in zip((a, b, c), lo)]


def spec_u42(a, b, c, d):
    """rt_rng.h: U_j = out[j] << 10 | (out[3] >> 10 j) & 0x3FF, j = 0, 1, 2."""
    u = lambda x: x.astype(np.uint64)
    return [(u(w) << np.uint64(10)) | ((u(d) >> np.uint64(10 * j)) & np.uint64(0x3FF)) for j, w in enumerate((a, b, c))]


def words():
    edge = np.array([0, 1, 0x3FF, 0x400, 0xFFF, 0x1000, 0x000FFC00, 0x3FF00000, 0x7FFFFFFF, 0x80000000, 0xFFFFF000,
                     0xFFFFFFFE, 0xFFFFFFFF, 0x55555555, 0xAAAAAAAA], dtype=np.uint32)
    grid = np.stack(np.meshgrid(edge, edge, indexing="ij"), -1).reshape(-1, 2)
    rng = np.random.default_rng(20261015)
    rand = rng.integers(0, 2**32, size=(200000, 4), dtype=np.uint64).astype(np.uint32)
    # every pair of edge words in (a, d), (b, d), (c, d), plus random blocks
    cols = [np.concatenate([grid[:, 0], grid[:, 1], grid[:, 1], rand[:, 0]]),
            np.concatenate([grid[:, 1], grid[:, 0], grid[:, 1], rand[:, 1]]),
            np.concatenate([grid[:, 1], grid[:, 1], grid[:, 0], rand[:, 2]]),
            np.concatenate([grid[:, 1], grid[:, 1], grid[:, 1], rand[:, 3]])]
    return cols


def test_alignbit_assembly_gives_the_rt_rng_bits():
    a, b, c, d = words()
    for bits, big_u in zip(new_bits(a, b, c, d), spec_u42(a, b, c, d)):
        # D = 2 (1 + U 2^-42): exponent 1, mantissa U << 10
        assert np.array_equal(bits, np.uint64(0x4000000000000000) | (big_u << np.uint64(10)))
        coord = bits.view(np.float64) - 3.0
        # -1 + 2 u42 (both sides exact in f64: multiples of 2^-41 below 1 in magnitude)
        assert np.array_equal(coord, -1.0 + 2.0 * (big_u.astype(np.float64) * 2.0**-42))
        assert coord.min() >= -1.0 and coord.max() < 1.0


@pytest.fixture(scope="module")
def pool_fast_asm():
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    return kernel_asm.asm_text("pool", "fast")


@pytest.mark.parametrize("variant", ["Li0ELb0ELb0ELb0E", "Li1ELb0ELb0ELb0E", "Li1ELb1ELb1ELb0E", "Li2ELb0ELb0ELb0E"])
def test_candidate_high_words_are_one_alignbit(pool_fast_asm, variant):
    start = pool_fast_asm.index("\n_ZN10rtdev_fast16k_trace_pool_f64I" + variant)
    body = pool_fast_asm[start:pool_fast_asm.index(".Lfunc_end", start)]
    assert not re.search(r"v_or_b32\w*\s+v\d+, 2\.0,", body), variant   # the old 0x40000000 | (w >> 12)
    # four per candidate (three high words and out[0]'s low word), in each of the sampler's candidate sites
    assert len(re.findall(r"v_alignbit_b32\s+[^\n]*, 12\n", body)) >= 8, variant
