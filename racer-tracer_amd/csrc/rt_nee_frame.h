// rt_nee_frame.h — the body of the whole-frame NEE kernels: k_nee_f64 (rt_nee_kernel.hip) with the light code of
// rt_render_frame_nee's first day, k_nee_lights_f64 (rt_nee_lights_kernel.hip) with rt_scene_set_lights' list.  One
// statement, inlined into both; LIGHTS is the policy of rt_nee_common.h's nee_samples and X its argument block.
#pragma once
#include "rt_nee_common.h"

namespace RT_KNS {

template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH, class LIGHTS>
__device__ __forceinline__ void nee_frame(const TraceArgs &A, const NeeArgs &N, const typename LIGHTS::Args &X) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tiles_x = (A.width + 15) >> 4;
    const int bx = blockIdx.x % tiles_x;
    const int by = blockIdx.x / tiles_x;
    const int px = bx * 16 + (wave & 1) * 8 + (lane & 7);
    const int vrow = by * 16 + (wave >> 1) * 8 + (lane >> 3); // a row of the launch's owned-row grid
    // owned row -> image row, once: the draws and the sums below are the IMAGE pixel's.  The strip fields are read through
    // kernargs_here(), next to their one use, so that a launch without strips keeps no register for them.
    const int py = image_row(kernargs_here(), vrow);
    // (an owned row at or beyond owned_rows lies in a strip that starts below the image: its image row is >= height)
    const bool in_image = px < A.width && py < A.height;

    PathRng rng;
    rng.pixel = (uint32_t)py * (uint32_t)A.width + (uint32_t)px;
    rng.k0 = A.seed_lo;
    rng.k1 = A.seed_hi;

    const double u = pixel_jitter(rng, px, A.width);

    d3 sum = mk(0.0, 0.0, 0.0); // the pixel's sum
    unsigned int n_segments = 0, n_started = 0;
    nee_samples<PRIMS, TEXTURED, SPECULAR, BVH, LIGHTS>(A, N, rng, px, py, u, in_image ? A.sample_begin : A.sample_end, A.sample_end, sum,
                                                        n_segments, n_started, X);

    if (in_image) {
        double *px_out = A.accum + 3 * (size_t)rng.pixel;
        px_out[0] = sum.x;
        px_out[1] = sum.y;
        px_out[2] = sum.z;
    }
    wave_stat_add(A, lane, RT_STAT_SEGMENTS, n_segments); // path segments (shadow rays excluded)
    wave_stat_add(A, lane, RT_STAT_SAMPLES, n_started);   // primary rays
}

} // namespace RT_KNS
