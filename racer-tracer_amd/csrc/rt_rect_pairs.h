// rt_rect_pairs.h — facing pairs of plain rects in the grouped device table: two rects on parallel planes with the same
// in-plane bounds (a box's two side walls, its floor and ceiling).  A ray can reach only the one its direction points at,
// so the pair loop of the rects-only closest-hit loop (rt_pool_coop.h: closest_hit_rects<true>) runs ONE full rect test
// per lane for such a pair, on the record the lane selects, where it ran two.  Plain C++17: the host compiles it too
// (rt_scene_create.hip marks the pairs; tests/rect_pairs_driver.cpp holds the rule to the two-test sequence).
//
// THE RULE, per lane, for a marked pair (records i and i + 1 of the table; c is the axis their planes fix):
//   sel     = the record with the larger k when the sign bit of d_c is clear, else the one with the smaller k
//   other   = its partner
//   t_other = (k_other - o_c) * inv_c        the two operations the rect test starts with: the bits it would have formed
//   settled = t_other < 0.001                the skipped test's first comparison rejects the lane, whatever best_t is
// When every shooting lane of the wave is settled, each runs the rect test of its `sel` and the second test is stepped
// over.  Otherwise the wave runs record i, then record i + 1, in every lane: what it ran before there were pairs.
//
// EXACT, bit for bit:
//   * A settled lane's skipped test would have changed neither `best` nor `best_t`: xy_rect.rs:32 leaves at t < t_min,
//     and t_min is the 0.001 of the comparison above, on the same t.
//   * The test the lane does run has the operands and the instructions the two-test sequence gave that record (the four
//     bounds are bit-identical in both records, k and the index are the record's own), and the `best_t` it starts from is
//     the one the sequence would have handed it: the other record's test, whether it came first or second, changed nothing.
//     So the order of a pair's two tests does not enter at all — no argument about ties is needed.
//   * Which record a lane selects decides how OFTEN the wave is settled, never what it computes.  (With finite, distinct
//     t at most one of a lane's two tests can pass anyway; +-0.0 and NaN directions, where that needs care, select by
//     their sign bit like everything else and are then settled or not by the comparison alone.)
//   * Not settled: d_c == +-0.0 with the origin on the wrong side (t_other = +inf), NaN (o_c == k with d_c == 0, or a NaN
//     ray), an origin outside the slab with the nearer plane ahead of it, and an origin on a plane whose rounding left it
//     0.001 or more behind.  All of them run the old sequence.
#pragma once
#include <stdint.h>
#include <cmath>
#include "rt_primary_bounds.h"

#if defined(__HIPCC__)
#define RT_PAIRS_FN __host__ __device__ inline
#else
#define RT_PAIRS_FN inline
#endif

namespace rt_pairs {

RT_PAIRS_FN uint64_t bits_of(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}

// Records a and b (consecutive in their group, a at an even distance from the group's first) are a facing pair: plain
// rects of one kind, bit-identical in-plane bounds, finite and different k.
inline bool facing_pair(const rtdev::RectGeo &a, const rtdev::RectGeo &b) {
    return a.axis == b.axis && bits_of(a.a0) == bits_of(b.a0) && bits_of(a.a1) == bits_of(b.a1) && bits_of(a.b0) == bits_of(b.b0) &&
           bits_of(a.b1) == bits_of(b.b1) && std::isfinite(a.k) && std::isfinite(b.k) && a.k != b.k;
}

// What the two records of a facing pair carry in the device table, in a field the rect tests do not read (Prim.p[5]: the
// eight bytes behind k).  A lane reads its record's k and table index from the table's copy in LDS, at a byte offset it
// forms from two wave-uniform words with three integer instructions; nothing is selected between scalars (which costs
// two moves and a select per 32-bit word on this target) and no index is multiplied.
//   low word, both records   : the record's own table index (what a lane reads behind the k it selected)
//   high word, first record  : the byte offset, from the table's start, of the k of the record with the LARGER k — a
//                              direction without a sign bit selects it.  Never 0 (k is not a record's first field):
//                              0 says "no pair" (every other plain rect of the groups, whatever its host record held).
//   high word, second record : the step from there to its partner's k, + or - one record.
enum : uint32_t { kRecordBytes = 192, kOffsetOfK = 32 }; // sizeof(rtdev::Prim), offsetof(rtdev::Prim, p[4]): asserted where Prim is known
struct Fields {
    uint64_t first, second; // the bits of p[5] of the pair's two records
};
// (i: the table index of the pair's first record, a)
inline Fields mark_facing(int i, double k_a, double k_b) {
    const uint32_t larger = (uint32_t)(k_a > k_b ? i : i + 1) * kRecordBytes + kOffsetOfK;
    const uint32_t step = k_a > k_b ? (uint32_t)kRecordBytes : 0u - (uint32_t)kRecordBytes;
    return Fields{(uint64_t)(uint32_t)i | (uint64_t)larger << 32, (uint64_t)(uint32_t)(i + 1) | (uint64_t)step << 32};
}
inline uint64_t mark_single(int i) { return (uint64_t)(uint32_t)i; }
// The field of every record of the three rect groups (XY, XZ, YZ: records [0, rect_end[0]), [rect_end[0], rect_end[1]),
// [rect_end[1], rect_end[2])), `geo` in table order.  Only records first + 2j, first + 2j + 1 of a group can be a pair:
// the pairing the closest-hit loop makes.
inline void mark_table(const rtdev::RectGeo *geo, const int32_t rect_end[3], uint64_t *field) {
    for (int j = 0; j < rect_end[2]; ++j) field[j] = mark_single(j);
    for (int g = 0, first = 0; g < 3; first = rect_end[g++])
        for (int j = first; j + 1 < rect_end[g]; j += 2)
            if (facing_pair(geo[j], geo[j + 1])) {
                const Fields f = mark_facing(j, geo[j].k, geo[j + 1].k);
                field[j] = f.first;
                field[j + 1] = f.second;
            }
}
RT_PAIRS_FN uint32_t larger_of(uint64_t first_bits) { return (uint32_t)(first_bits >> 32); } // 0: not a pair
RT_PAIRS_FN uint32_t step_of(uint64_t second_bits) { return (uint32_t)(second_bits >> 32); }

// ---- the rule (offsets of k in the table's bytes; the caller reads k, and the index behind it, there)
// (`larger` may be counted from anywhere — the table's first byte, address 0 of the memory the table lies in — as long
// as the caller reads where it counted from: the rule adds and subtracts.)
RT_PAIRS_FN uint32_t sign_mask(double d_c) { // 0, or all ones under a sign bit
    const uint32_t hi = (uint32_t)(bits_of(d_c) >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
    // (the shift below as the one instruction it is: left to the optimiser, the shift and the AND behind it become a
    // comparison with 0, a move of `step` into a vector register and a select)
    uint32_t mask;
    asm("v_ashrrev_i32 %0, 31, %1" : "=v"(mask) : "v"(hi));
    return mask;
#else
    return (uint32_t)((int32_t)hi >> 31);
#endif
}
RT_PAIRS_FN uint32_t selected(uint32_t larger, uint32_t step, uint32_t sign) { return larger + (sign & step); }
RT_PAIRS_FN uint32_t partner(uint32_t larger, uint32_t step, uint32_t sel) { return (2u * larger + step) - sel; }
RT_PAIRS_FN double t_of_plane(double k, double o_c, double inv_c) { return (k - o_c) * inv_c; }
RT_PAIRS_FN bool settled(double t_other) { return t_other < 0.001; }

} // namespace rt_pairs
