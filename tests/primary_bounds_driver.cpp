// Prints rtdev::primary_bounds (racer-tracer_amd/csrc/rt_primary_bounds.h) for every case on standard input, one line each.
// A case is 21 numbers: origin[3] ulc[3] horizontal[3] vertical[3] lens_radius width height mn[3] mx[3] (strtod's forms:
// hexadecimal floats, nan, inf); the answer is "px0 px1 py0 py1".
// Host code only: the header needs no HIP (tests/test_primary_bounds_cpu.py compiles this with g++).
#include <cstdio>
#include "rt_primary_bounds.h"

int main() {
    for (;;) {
        double x[21];
        for (int i = 0; i < 21; ++i)
            if (scanf("%lf", &x[i]) != 1) return i == 0 ? 0 : 1; // (a case cut short is an error)
        const rtdev::PixelRect r = rtdev::primary_bounds(x, x + 3, x + 6, x + 9, x[12], (int)x[13], (int)x[14], x + 15, x + 18);
        printf("%d %d %d %d\n", r.px0, r.px1, r.py0, r.py1);
    }
}
