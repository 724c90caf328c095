"""The sphere sampler's candidates drawn from a per-request Philox prefix (rt_trace_common.h: scatter_prefix /
philox_from_prefix) and its answers returned through the request slots (rt_trace_pool_kernel.hip:
coop_random_in_unit_sphere), pinned twice (CPU tests):
  * a numpy model of the two functions, written the way the device code is, gives the oracle's plain Philox4x32-7 block
    for every counter, key and block tried — so the frame cannot change; the same for the scalar per-group lowest bit
    that picks the lane answering each request;
  * the compiled rects-only kernel (`<0,0,0,0>`, hipcc cross-compiling gfx950 without a GPU) has 4 multiplies per
    request and 10 per candidate instead of 14, and no lane shuffles left in the sampler's grouped rounds."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import kernel_asm

sys.path.insert(0, kernel_asm.ROOT)
from oracle import oracle_ctypes as orc  # noqa: E402

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
ROUNDS = 7
SCATTER = 3
U32 = np.uint64(0xFFFFFFFF)


def rng_h_constants():
    text = open(os.path.join(kernel_asm.ROOT, "include", "rt_rng.h")).read()
    get = lambda name: int(re.search(r"#define %s (\w+?)u?\b" % name, text).group(1), 0)
    return (get("RT_PHILOX_ROUNDS"), get("RT_PHILOX_M0"), get("RT_PHILOX_M1"), get("RT_PHILOX_W0"), get("RT_PHILOX_W1"),
            get("RT_RNG_SCATTER"))


def test_model_constants_are_rt_rng_h():
    assert rng_h_constants() == (ROUNDS, M0, M1, W0, W1, SCATTER)


def mul(m, x):
    """(hi, lo) of the 64-bit product of a 32-bit constant and 32-bit words."""
    p = np.uint64(m) * x
    return p >> np.uint64(32), p & U32


def add(k, r, w):
    return (k + np.uint64(r) * np.uint64(w)) & U32


def rounds_from(first, c0, c1, c2, c3, k0, k1):
    """Rounds first .. ROUNDS - 1 (rt_trace_common.h: philox_rounds), k0 / k1 being round `first`'s keys."""
    for _ in range(first, ROUNDS):
        h0, l0 = mul(M0, c0)
        h1, l1 = mul(M1, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = add(k0, 1, W0), add(k1, 1, W1)
    return c0, c1, c2, c3


def scatter_prefix(pixel, sample, seg, k0, k1):
    """rt_trace_common.h: scatter_prefix, step for step: (b, y, x, w, z)."""
    h0, l0 = mul(M0, pixel)                                  # round 1
    h1, l1 = mul(M1, ((seg << np.uint64(8)) | np.uint64(SCATTER)) & U32)
    a = h1 ^ sample ^ k0
    qh, ql = mul(M0, a)                                      # round 2's M0 multiply
    c2 = qh ^ l0 ^ add(k1, 1, W1)
    rh, rl = mul(M1, c2)                                     # round 3's M1 multiply
    return h0 ^ k1, l1 ^ add(k0, 1, W0), rh ^ add(k0, 2, W0), rl, ql ^ add(k1, 2, W1)


def philox_from_prefix(prefix, block, k0, k1):
    """rt_trace_common.h: philox_from_prefix, step for step."""
    b, y, x, w, z = prefix
    sh, sl = mul(M1, b ^ block)                              # round 2's M1 multiply
    th, tl = mul(M0, sh ^ y)                                 # round 3's M0 multiply
    return rounds_from(3, x ^ sl, w, th ^ z, tl, add(k0, 3, W0), add(k1, 3, W1))


def oracle_block(pixel, sample, seg, block, k0, k1):
    out = (C.c_uint32 * 4)()
    orc.lib().orc_philox4x32((C.c_uint32 * 4)(pixel, sample, ((seg << 8) | SCATTER) & 0xFFFFFFFF, block),
                             (C.c_uint32 * 2)(k0, k1), ROUNDS, out)
    return tuple(out)


EDGE = [0, 1, 2, 3, 0xFF, 0x100, 0xFFFF, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
BLOCKS = [0, 1, 2, 3, 7, 15, 31, 63, 255, 0xFFFF, 0x7FFFFFFF, 0xFFFFFFFF]  # 0, 1 and 2^k - 1 up to 2^32 - 1


def cases():
    rng = np.random.default_rng(20261016)
    rows = []
    for e in EDGE:  # every edge word in every position of the counter and the key
        for pos in range(5):
            r = [int(v) for v in rng.integers(0, 2**32, size=5, dtype=np.uint64)]
            r[pos] = e
            rows.append(r)
    rows += [[int(v) for v in rng.integers(0, 2**32, size=5, dtype=np.uint64)] for _ in range(400)]
    rows += [[0, 0, 0, 0, 0], [0xFFFFFFFF] * 5, [1920 * 1080 - 1, 1023, 19, 1, 0]]
    return rows


def test_prefix_model_equals_the_oracles_philox():
    rng = np.random.default_rng(7)
    checked = 0
    for pixel, sample, seg, k0, k1 in cases():
        u = np.uint64
        prefix = scatter_prefix(u(pixel), u(sample), u(seg), u(k0), u(k1))
        for block in BLOCKS + [int(rng.integers(0, 2**32))]:
            got = tuple(int(v) for v in philox_from_prefix(prefix, u(block), u(k0), u(k1)))
            assert got == oracle_block(pixel, sample, seg, block, k0, k1), (pixel, sample, seg, block, k0, k1)
            checked += 1
    assert checked > 5000


def test_prefix_model_vectorised_over_random_counters():
    """20 000 random counters, keys and blocks at once, against the plain rounds of the same model, and every 997th of
    them against the oracle."""
    rng = np.random.default_rng(42)
    pixel, sample, seg, block, k0, k1 = (rng.integers(0, 2**32, size=20000, dtype=np.uint64) for _ in range(6))
    plain = rounds_from(0, pixel, sample, ((seg << np.uint64(8)) | np.uint64(SCATTER)) & U32, block, k0, k1)
    fast = philox_from_prefix(scatter_prefix(pixel, sample, seg, k0, k1), block, k0, k1)
    for a, b in zip(plain, fast):
        assert np.array_equal(a, b)
    for n in range(0, 20000, 997):
        assert tuple(int(v[n]) for v in plain) == oracle_block(*(int(v[n]) for v in (pixel, sample, seg, block, k0, k1)))


def lowest_in_groups(x, lg):
    """rt_trace_pool_kernel.hip: lowest_in_groups, in 64-bit words."""
    m = (1 << 64) - 1
    q = 1 << lg
    low = 1
    for k in range(6):
        low |= (low << ((q << k) & 63)) & m
    top = (low << (q - 1)) & m
    nx = ~x & m
    return x & ((((nx & ~top & m) + low) & m) ^ (nx & top))


def test_lowest_in_groups_picks_the_first_accepted_lane_of_every_group():
    rng = np.random.default_rng(3)
    words = [0, (1 << 64) - 1, 1, 1 << 63, 0x8000000080000000, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA]
    words += [int(v) for v in rng.integers(0, 2**63, size=3000, dtype=np.uint64)]
    words += [int(a) & int(b) & int(c) for a, b, c in rng.integers(0, 2**63, size=(1000, 3), dtype=np.uint64)]
    words += [w << 1 | 1 for w in words[:200]]
    for lg in range(1, 7):
        q = 1 << lg
        for x in words:
            want = 0
            for g in range(0, 64, q):
                field = (x >> g) & ((1 << q) - 1)
                if field:
                    want |= (field & -field) << g
            assert lowest_in_groups(x, lg) == want, (hex(x), lg)


# ---------------------------------------------------------------------------------------------- compiled code
C3 = "Li0ELb0ELb0ELb0E"


@pytest.fixture(scope="module")
def c3_ops():
    if kernel_asm.hipcc() is None:
        pytest.skip("no hipcc")
    text = kernel_asm.asm_text("pool", "fast")
    start = text.index("\n_ZN10rtdev_fast16k_trace_pool_f64I" + C3)
    body = text[start:text.index(".Lfunc_end", start)]
    ops = [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith(".")]
    return [o for o in ops if not o.startswith(";")]


def post_runs(ops):
    """Starts of six consecutive ds_write_b32 from one address at consecutive offsets: the sampler's request posts."""
    starts = []
    for i in range(len(ops) - 5):
        run = [re.match(r"ds_write_b32 (v\d+), v\d+(?: offset:(\d+))?$", o) for o in ops[i:i + 6]]
        if all(run) and len({m.group(1) for m in run}) == 1:
            offs = [int(m.group(2) or 0) for m in run]
            if offs == [offs[0] + 4 * k for k in range(6)]:
                starts.append(i)
    return starts


def test_multiplies_per_request_and_per_candidate(c3_ops):
    """Static v_mad_u64_u32 of the rects-only kernel: 105 before the prefix.  The sampler now holds one 4-multiply prefix
    and four candidate sites (the own-candidate and the grouped form of each of the two unrolled rounds) of 10 each; the
    other 53 are the camera batches' Philox and address arithmetic."""
    muls = [o for o in c3_ops if o.startswith("v_mad_u64_u32")]
    assert len(muls) == 97, len(muls)


def test_grouped_rounds_answer_through_the_slot(c3_ops):
    posts = post_runs(c3_ops)
    assert len(posts) == 2, posts  # one post in each of the two unrolled rounds
    # the later round's result write is ONE in-place masked move (move_masked: inline asm, its three moves printed
    # without _e32 between the exec mask's save and restore)
    moves = [i for i in range(1, len(c3_ops) - 4) if c3_ops[i - 1].startswith("s_and_saveexec_b64")
             and all(re.match(r"v_mov_b64 v\[", o) for o in c3_ops[i:i + 3]) and c3_ops[i + 3].startswith("s_mov_b64 exec,")]
    assert len(moves) == 1 and moves[0] > posts[1], (moves, posts)
    region = c3_ops[posts[0]:moves[0] + 3]
    assert not any(o.startswith("ds_bpermute_b32") for o in region)
    # each grouped round's answer: three doubles written into the slot by the winning lanes
    answers = [o for o in region if re.match(r"ds_write(2)?_b64 ", o)]
    assert len(answers) == 4, answers
    # the whole kernel: the six shuffles of each grouped round are gone (40 before)
    assert sum(1 for o in c3_ops if o.startswith("ds_bpermute_b32")) == 28
