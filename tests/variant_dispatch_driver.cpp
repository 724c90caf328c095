// Prints what rtdev::dispatch_variant (racer-tracer_amd/csrc/rt_variant_dispatch.h) picks for every combination of
// prims_class in {-1, 0, 1, 2, 7}, textured, specular and bvh, one line each:
//   <prims_class> <textured> <specular> <bvh> -> <P> <T> <S> <B>
// Host code only: the header needs no HIP (tests/test_variant_dispatch.py compiles this with g++).
#include <cstdio>
#include "rt_variant_dispatch.h"

namespace {
// a variant that reports its own template arguments
template <int P, bool T, bool S, bool B> struct Echo {
    static int key() { return P * 1000 + T * 100 + S * 10 + B; }
};
} // namespace

int main() {
    const int classes[] = {-1, 0, 1, 2, 7};
    for (int c : classes)
        for (int t = 0; t < 2; ++t)
            for (int s = 0; s < 2; ++s)
                for (int b = 0; b < 2; ++b) {
                    const int key = rtdev::dispatch_variant<Echo>(c, t != 0, s != 0, b != 0, [](auto v) { return decltype(v)::key(); });
                    printf("%d %d %d %d -> %d %d %d %d\n", c, t, s, b, key / 1000, key / 100 % 10, key / 10 % 10, key % 10);
                }
    // a callable without a result is dispatched too (the launchers' form)
    int calls = 0;
    rtdev::dispatch_variant<Echo>(rtdev::PRIMS_RECTS, true, false, false, [&](auto) { ++calls; });
    return calls == 1 ? 0 : 1;
}
