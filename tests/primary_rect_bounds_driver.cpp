// Prints rtdev::primary_rects (racer-tracer_amd/csrc/rt_primary_bounds.h) — the kernel argument rt_api.hip's launch_pool
// forms on every launch — for every case on standard input, one line each.
// A case is 23 numbers and its rects: origin[3] ulc[3] horizontal[3] vertical[3] lens_radius width height mn[3] mx[3]
// force n_rects, then n_rects times "axis a0 a1 b0 b1 k" (strtod's forms: hexadecimal floats, nan, inf).  The scene's
// rectangle is primary_bounds of the box [mn, mx] as in fill_args — or, with force != 0, the frame without its outermost
// pixels: a rectangle that is not the whole frame, so that a rect's OWN doubts can be told from the scene's.
// The answer is "n  sx0 sx1 sy0 sy1" and the RT_PRIMARY_RECTS rectangles, four integers each.
// Host code only: the header needs no HIP (tests/test_primary_rect_bounds_cpu.py compiles this with g++).
#include <cstdio>
#include <vector>
#include "rt_primary_bounds.h"

int main() {
    for (;;) {
        double x[23];
        for (int i = 0; i < 23; ++i)
            if (scanf("%lf", &x[i]) != 1) return i == 0 ? 0 : 1; // (a case cut short is an error)
        const int width = (int)x[13], height = (int)x[14], n_rects = (int)x[22];
        std::vector<rtdev::RectGeo> rects;
        for (int j = 0; j < n_rects; ++j) {
            double g[6];
            for (int i = 0; i < 6; ++i)
                if (scanf("%lf", &g[i]) != 1) return 1;
            rects.push_back(rtdev::RectGeo{(int32_t)g[0], g[1], g[2], g[3], g[4], g[5]});
        }
        rtdev::PixelRect scene = rtdev::primary_bounds(x, x + 3, x + 6, x + 9, x[12], width, height, x + 15, x + 18);
        if (x[21] != 0.0) scene = rtdev::PixelRect{1, width - 2, 1, height - 2};
        const rtdev::PrimaryRects r = rtdev::primary_rects(x, x + 3, x + 6, x + 9, width, height, scene, rects.data(), n_rects);
        printf("%d %d %d %d %d", r.n, scene.px0, scene.px1, scene.py0, scene.py1);
        for (int i = 0; i < rtdev::RT_PRIMARY_RECTS; ++i) printf(" %d %d %d %d", r.r[i].px0, r.r[i].px1, r.r[i].py0, r.r[i].py1);
        printf("\n");
    }
}
