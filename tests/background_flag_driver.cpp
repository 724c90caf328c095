// Prints rtdev::background_is_black (racer-tracer_amd/csrc/rt_device_types.h) — what rt_api.hip's fill_args writes into
// TraceArgs.bg_black on every render — for every case on standard input, one line each.
// A case is four numbers: kind top[3] (strtod's forms: -0.0, 1e-300, hexadecimal floats, nan, inf); the answer is 0 or 1.
// With the argument `layout` it prints instead "offsetof(TraceArgs, bg_black) sizeof(TraceArgs) offsetof(TraceArgs, cull_py1)":
// where the kernels find the flag, and that it is the last member, behind what was the last one.
// Host code only: the header needs no HIP (tests/test_background_flag_cpu.py compiles this with g++).
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "rt_device_types.h"

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "layout") == 0) {
        printf("%zu %zu %zu\n", offsetof(rtdev::TraceArgs, bg_black), sizeof(rtdev::TraceArgs), offsetof(rtdev::TraceArgs, cull_py1));
        return 0;
    }
    for (;;) {
        double x[4];
        for (int i = 0; i < 4; ++i)
            if (scanf("%lf", &x[i]) != 1) return i == 0 ? 0 : 1; // (a case cut short is an error)
        rtdev::Background bg;
        memset(&bg, 0, sizeof bg);
        bg.kind = (int32_t)x[0];
        for (int k = 0; k < 3; ++k) {
            bg.top[k] = x[1 + k];
            bg.bottom[k] = 0.25; // (the flag does not read it)
        }
        printf("%d\n", (int)rtdev::background_is_black(bg));
    }
}
