// The group arithmetic of the wave-cooperative samplers (racer-tracer_amd/csrc/rt_pool_groups.h) on the CPU, for
// tests/test_group_math_cpu.py, which also builds and runs it under AddressSanitizer and UBSan.
// Standard input, one command per line; standard output, one answer per line:
//   lg <n>            -> group_lg(n)
//   masks <lg>        -> low top width of group_masks(lg), hexadecimal
//   lowest <x> <lg>   -> lowest_in_groups(x, group_masks(lg)), hexadecimal (x hexadecimal)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "rt_pool_groups.h"

int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (std::strcmp(what, "lg") == 0) {
            unsigned n;
            if (std::scanf("%u", &n) != 1) return 2;
            std::printf("%d\n", rt_groups::group_lg(n));
        } else if (std::strcmp(what, "masks") == 0) {
            unsigned lg;
            if (std::scanf("%u", &lg) != 1 || lg > 6) return 2;
            const rt_groups::GroupMasks m = rt_groups::group_masks(lg);
            std::printf("%" PRIx64 " %" PRIx64 " %" PRIx64 "\n", m.low, m.top, m.width);
        } else if (std::strcmp(what, "lowest") == 0) {
            uint64_t x;
            unsigned lg;
            if (std::scanf("%" SCNx64 " %u", &x, &lg) != 2 || lg > 6) return 2;
            std::printf("%" PRIx64 "\n", rt_groups::lowest_in_groups(x, rt_groups::group_masks(lg)));
        } else {
            return 2;
        }
    }
    return 0;
}
