// rt_pool_groups.h — the group arithmetic of the wave-cooperative samplers (rt_pool_coop.h): n open requests share the
// 64 lanes of a wave in groups of q = 2^lg lanes, one group per request.  Everything here is integer arithmetic on
// values that are the same in all 64 lanes; on the device it belongs to the scalar unit, which every wave of a CU
// queues for, so each piece is stated in the shortest form the unit has: the group size by one count of leading
// zeros, the masks by one table read.  Plain C++17: the host compiles it too (tests/group_math_driver.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_GROUPS_FN __host__ __device__ inline
#else
#define RT_GROUPS_FN inline
#endif

namespace rt_groups {

// lg of the group size for n open requests, 1 <= n <= 64: the largest lg with n << lg <= 64, which is
// 6 - ceil(log2 n) = (n <= 1 ? 6 : clz(n - 1) - 26).  2n - 1 has one significant bit more than n - 1 and is never
// zero, so the same number is clz(2n - 1) - 25 with no case for n == 1.
RT_GROUPS_FN int group_lg(uint32_t n) { return __builtin_clz(2u * n - 1u) - 25; }

// The masks of the groups of q = 2^lg bits of a 64-bit lane mask, 0 <= lg <= 6:
//   low   : bit 0 of every group      (0xffff…, 0x5555…, 0x1111…, 0x0101…, 0x00010001…, 0x0000000100000001, 1)
//   top   : bit q - 1 of every group  (low << (q - 1))
//   width : the q low bits            (one group's worth of lanes, shifted down to bit 0)
struct GroupMasks {
    uint64_t low, top, width;
    uint64_t pad; // 32 bytes: an entry's byte offset is lg << 5
};

// (computed, not written out: the table below is this function at lg = 0 .. 6, and the host test holds both to the
// shift ladder that lowest_in_groups used to run in every round)
constexpr GroupMasks group_masks_of(int lg) {
    const int q = 1 << lg;
    uint64_t low = 0;
    for (int b = 0; b < 64; b += q) low |= 1ull << b;
    return GroupMasks{low, low << (q - 1), q == 64 ? ~0ull : (1ull << q) - 1ull, 0};
}

RT_GROUPS_FN GroupMasks group_masks(uint32_t lg) {
    constexpr GroupMasks table[7] = {group_masks_of(0), group_masks_of(1), group_masks_of(2), group_masks_of(3),
                                     group_masks_of(4), group_masks_of(5), group_masks_of(6)};
    return table[lg];
}

// The lowest set bit of every group of x: x & -x within each group, the negation done per group as (~x without the
// groups' top bits) + 1 in every group, whose carry stops at the group's top bit, XOR the top bits of ~x.
RT_GROUPS_FN uint64_t lowest_in_groups(uint64_t x, const GroupMasks &m) {
    return x & (((~x & ~m.top) + m.low) ^ (~x & m.top));
}

} // namespace rt_groups
