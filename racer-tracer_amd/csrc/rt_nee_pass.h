// rt_nee_pass.h — the body of the NEE kernels that trace one chunk of listed tiles on top of the running sums:
// k_nee_pass_f64 (rt_nee_pass_kernel.hip, which says what a pass is) and k_nee_lights_pass_f64
// (rt_nee_lights_pass_kernel.hip) with rt_scene_set_lights' list.  LIGHTS / X as in rt_nee_frame.h.
#pragma once
#include "rt_nee_common.h"

namespace RT_KNS {

template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH, class LIGHTS>
__device__ __forceinline__ void nee_pass(const TraceArgs &A, const NeeArgs &N, const typename LIGHTS::Args &X) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t item = 4u * blockIdx.x + (uint32_t)wave; // wave-uniform
    // (a wave without work — beyond the list, or cancelled — runs through with no pixel in the image rather than return
    // early: with the early exits the compiler gave the twelve linear-loop variants a 68- or 132-byte stack frame that
    // no instruction touches, and a private segment has to be set up for every wave of a launch)
    unsigned int up = item >= A.n_items;
    if (A.cancel_flag != nullptr && lane == 0) up |= __hip_atomic_load(A.cancel_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    up = __builtin_amdgcn_readfirstlane(up);
    uint32_t tile = item;
    if (A.tile_list != nullptr) tile = __builtin_amdgcn_readfirstlane(A.tile_list[up ? 0u : item]);
    const bool idle = up != 0u || tile >= (uint32_t)A.n_tiles; // (a list holds tiles of the grid only)
    const int px = (int)(tile % (uint32_t)A.tiles_x) * 8 + (lane & 7);
    const int py = (int)(tile / (uint32_t)A.tiles_x) * 8 + (lane >> 3);
    const bool in_image = !idle && px < A.width && py < A.height;

    PathRng rng;
    rng.pixel = (uint32_t)py * (uint32_t)A.width + (uint32_t)px;
    rng.k0 = A.seed_lo;
    rng.k1 = A.seed_hi;

    // cpu.rs:35-36: one horizontal jitter per pixel.  rt_path_steps.h's pixel_jitter, written out: as a call it changes nothing
    // but the numbering of scalar registers, and rt_render_progressive_nee's kernel time rose by 0.4 to 0.5 % on the Cornell
    // scenes with it, in every run (LABNOTES 16)
    rng.sample = RT_RNG_SAMPLE_PIXEL;
    const u4 bj = rng.block(0, RT_RNG_PIXEL, 0);
    const double u = ((double)px + u53(bj.a, bj.b)) / (double)(A.width - 1);

    d3 sum = mk(0.0, 0.0, 0.0); // the pixel's running sum (+0.0 before the first chunk: the host cleared accum)
    if (in_image) {
        const double *px_sum = A.accum + 3 * (size_t)rng.pixel;
        sum = mk(px_sum[0], px_sum[1], px_sum[2]);
    }
    unsigned int n_segments = 0, n_started = 0;
    nee_samples<PRIMS, TEXTURED, SPECULAR, BVH, LIGHTS>(A, N, rng, px, py, u, in_image ? A.sample_begin : A.sample_end, A.sample_end, sum,
                                                        n_segments, n_started, X);
    if (in_image) {
        double *px_sum = A.accum + 3 * (size_t)rng.pixel;
        px_sum[0] = sum.x;
        px_sum[1] = sum.y;
        px_sum[2] = sum.z;
    }
    wave_stat_add(A, lane, RT_STAT_SEGMENTS, n_segments); // path segments (shadow rays excluded)
    wave_stat_add(A, lane, RT_STAT_SAMPLES, n_started);   // primary rays
}

} // namespace RT_KNS
