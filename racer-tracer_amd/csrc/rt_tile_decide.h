// rt_tile_decide.h — the decision step of an adaptive pass (rtdev::TileDecision), stated once for the two kernels that
// run it: k_fold_adaptive_f64 (rt_frame_kernels.hip, behind the pooled kernel's slices) and k_nee_decide_f64
// (rt_nee_pass_kernel.hip, behind the NEE passes).  One wave per 8x8 tile of the WHOLE frame, one lane per pixel, 16
// tiles to a block.  Every tile writes its pixels into the pass's frame slot, sqrt(scale * S) with the pass's scale
// while it runs and with its own once it has stopped (the very bits of its stop: its sums are no longer touched), so the
// slot is whole without a copy between slots.  A running tile's error (include/rt_abi.h: rt_render_adaptive) is the
// largest of tile_pixel_error over its pixels and channels; it stops (eligible, error <= threshold) or is appended to
// the next pass's list.
#pragma once
#include <math.h>
#include "rt_device_types.h"

#ifdef __HIPCC__
#define RT_TILE_FN __host__ __device__ __forceinline__
#else
#define RT_TILE_FN inline // (the host tests compile the error alone: tests/tile_error_driver.cpp)
#endif

namespace rtdev {

// e = sigma / (sqrt(m + sigma) + sqrt(m)) of one pixel and channel: m = S / s, V = max(0, Q - S m) / (k - 1) over the k
// chunks taken for batch means, sigma = sqrt(V / s); e = 0 where sigma = 0, so a black pixel needs no floor.
// scale = 1 / s and inv_batches = 1 / (k - 1) come from the host: the error is compared to a threshold, not bit for bit.
RT_TILE_FN double tile_pixel_error(double S, double Q, double scale, double inv_batches) {
    const double m = S * scale;
    const double var = fmax(0.0, Q - S * m) * inv_batches;
    const double sigma = sqrt(var * scale);
    return sigma > 0.0 ? sigma / (sqrt(m + sigma) + sqrt(m)) : 0.0;
}

} // namespace rtdev

#ifdef __HIPCC__
#include "rt_trace_common.h"

namespace RT_KNS {

// Tile t (wave-uniform, < D.n_tiles), by its whole wave: the stopped tile rewrites its pixels; the running one takes
// `fold(i, S, Q)` in its valid lanes — what the pass adds to the pixel's sums S and Q (at element i of the frame), if
// the kernel has anything to add — then writes its pixels, takes its error and stops or runs on.
// Returns, in lane 0, 1 when the tile runs on.
template <class Fold> __device__ __forceinline__ uint32_t decide_tile(const TileDecision &D, int t, int lane, Fold fold) {
    const int tx = t % D.tiles_x, ty = t / D.tiles_x;
    const int px = tx * 8 + (lane & 7), py = ty * 8 + (lane >> 3);
    const bool valid = px < D.width && py < D.height;
    const size_t i = valid ? ((size_t)py * (size_t)D.width + (size_t)px) * 3 : 0;
    double S[3] = {0.0, 0.0, 0.0}, Q[3] = {0.0, 0.0, 0.0};
    if (valid)
        for (int ch = 0; ch < 3; ++ch) S[ch] = D.running[i + ch];
    const int stop = __builtin_amdgcn_readfirstlane(D.tile_stop[t]);
    if (stop != 0) {
        const double scale = D.tile_scale[t];
        if (valid)
            for (int ch = 0; ch < 3; ++ch) D.out[i + ch] = sqrt(scale * S[ch]);
        if (lane == 0) D.err[t] = D.err_prev[t];
        return 0u;
    }
    double e_max = 0.0;
    if (valid) {
        for (int ch = 0; ch < 3; ++ch) Q[ch] = D.squares[i + ch];
        fold(i, S, Q);
        for (int ch = 0; ch < 3; ++ch) {
            D.out[i + ch] = sqrt(D.scale * S[ch]);
            if (D.chunks_done >= 2) {
                const double e = tile_pixel_error(S[ch], Q[ch], D.scale, D.inv_batches);
                e_max = e > e_max ? e : e_max;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(e_max, off, 64);
        e_max = o > e_max ? o : e_max;
    }
    uint32_t keep = 0u;
    if (lane == 0) {
        const double err = D.chunks_done >= 2 ? e_max : -1.0;
        D.err[t] = err;
        if (D.eligible && err <= D.threshold) {
            D.tile_stop[t] = D.samples_done;
            D.tile_scale[t] = D.scale;
        } else {
            keep = 1u;
        }
    }
    return keep;
}

// The tiles that run on (`keep` in lane 0 of the wave of tile t; every thread of the block calls this) are appended to
// the next list with ONE atomic per block of 16 tiles: one per tile, all on the one counter, serialised at L2 and
// cost 0.38 ms a pass on a 1080p frame.
__device__ __forceinline__ void append_running_tiles(const TileDecision &D, int t, int lane, int wave, uint32_t keep) {
    __shared__ uint32_t keep_of[16];
    __shared__ uint32_t list_base;
    if (lane == 0) keep_of[wave] = keep;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < 16; ++w) total += keep_of[w];
        list_base = total ? atomicAdd(D.next_count, total) : 0u;
    }
    __syncthreads();
    if (lane == 0 && keep) {
        uint32_t at = list_base;
        for (int w = 0; w < wave; ++w) at += keep_of[w];
        D.next_list[at] = (uint32_t)t;
    }
}

} // namespace RT_KNS
#endif
