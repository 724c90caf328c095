// rt_nee_stream.h — the body of the NEE tile-stream kernels and what it stands on: k_nee_stream_f64
// (rt_nee_stream_kernel.hip, which describes the launch) and k_nee_lights_stream_f64 (rt_nee_lights_stream_kernel.hip) with
// rt_scene_set_lights' list.  LIGHTS is the policy of rt_nee_common.h's nee_samples and X its argument block.
#pragma once
#include "rt_nee_common.h"

// Samples a wave traces between two looks at the host's cancel word.  A tuning constant: the sum is carried from chunk to
// chunk in registers, in sample order, so no pixel depends on it.  Small = a cancel lands sooner (a wave runs out its
// chunk, not its tile); the price per chunk is one read of pinned host memory by lane 0 and the lanes of the wave meeting
// at the boundary (a lane whose paths were short waits for the wave's longest).  Measured: 16 costs
// the Cornell scenes +32 to +45 % over the one-shot frame and a cancel returns in 1.6-3.6 ms; 64 costs them +9 to +16 %
// (nothing on emissive) and a cancel returns in 5-12.5 ms.
#ifndef RT_NEE_STREAM_CHUNK
#define RT_NEE_STREAM_CHUNK 64
#endif

namespace RT_KNS {

constexpr int kNeeStreamChunk = RT_NEE_STREAM_CHUNK;
#ifdef RT_EXACT_DIV
constexpr bool kStreamExact = true;
#else
constexpr bool kStreamExact = false;
#endif
// Waves per SIMD the register allocator is held to (__launch_bounds__' second argument with blocks of 256 threads):
// k_nee_f64's own occupancy step of the same key and flavour wherever that costs no scratch memory.  Left alone, the
// tile loop around the path loop takes 2 to 12 VGPRs more than k_nee_f64 and the plain-colour rect variants (126 / 127
// VGPRs there) fall from 4 waves to 3; held to 128 they fit without a spill.  The exception is the exact rect variant with
// Metal / Dielectric, which spills 12 to 80 bytes at 128 in every shape tried and is left at 3 waves (DESIGN.md 4.10 has
// the table).
// This table and kStreamShape below are fitted to ONE compiler's register allocation (the ROCm release the register table
// of DESIGN.md 4.10 was taken with).  After a compiler change, sweep both again: tests/test_nee_stream_isa.py fails where
// a variant gains a private segment or leaves k_nee_f64's occupancy step, and says which.
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
constexpr int kStreamWaves = TEXTURED ? 1
                             : BVH    ? 3
                             : (PRIMS == PRIMS_RECTS && !(kStreamExact && SPECULAR)) || (kStreamExact && PRIMS == PRIMS_SPHERES && !SPECULAR) ? 4
                                                                                                                                               : 3;
// Where a tile's prologue and the chunk loop read the launch's arguments from.  By default the prologue re-reads them
// through kernargs_here() (nothing of it is hoisted in front of the loops: 4-5 VGPRs) and the chunk loop uses the kernel's
// own copy.  Three variants are compiled the other way round: in the default shape their kernels carry a 32- or 64-byte
// stack frame that no instruction touches (slots of scalar spills that ended up in VGPR lanes), and a private segment has
// to be set up for every wave of such a launch; in this shape they have none and stay in k_nee_f64's occupancy step
// (tests/test_nee_stream_isa.py holds both).  Same arithmetic either way.  The price: fast (0,1,1,0) takes 250 VGPRs in
// this shape (k_nee_f64: 235) — the same step, 1 wave, but with little room left under 256.
enum : unsigned { STREAM_PROLOGUE_FROM_COPY = 1u, STREAM_LOOP_FROM_KERNARGS = 2u };
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
constexpr unsigned kStreamShape =
    !kStreamExact && PRIMS == PRIMS_RECTS && TEXTURED && !BVH ? (SPECULAR ? STREAM_PROLOGUE_FROM_COPY | STREAM_LOOP_FROM_KERNARGS : STREAM_PROLOGUE_FROM_COPY)
    : kStreamExact && PRIMS == PRIMS_ANY && !TEXTURED && !SPECULAR && !BVH ? STREAM_PROLOGUE_FROM_COPY
                                                                           : 0u;
static_assert(kNeeStreamChunk >= 1, "a chunk holds at least one sample");

// Item -> tile: the items are the tiles of the launch's regions in queue order, row-major inside a region
// (rt_device_types.h: Region with ONE chunk per tile; rt_api.hip: setup_delivery fills item_begin).  All wave-uniform.
__device__ __forceinline__ void stream_tile_of(const RT_CONSTANT TraceArgs *K, uint32_t item, int &region, int &tx, int &ty,
                                               uint32_t &reg_tiles) {
    region = 0;
    while (region + 1 < K->n_regions && item >= K->regions[region + 1].item_begin) ++region;
    const uint32_t local = item - K->regions[region].item_begin;
    const uint32_t ntx = (uint32_t)K->regions[region].ntx;
    tx = K->regions[region].tx0 + (int)(local % ntx);
    ty = K->regions[region].ty0 + (int)(local / ntx);
    reg_tiles = ntx * (uint32_t)K->regions[region].nty;
}

// Tile row -> image row of the lane's pixel.  A region's tile rows are rows of the launch's OWNED-row grid (rt_device_types.h:
// Region), so with strips (strip_count > 1: a share of rt_render_frame_nee_multi / rt_render_nee_multi) the lane's owned row
// ty * 8 + lane / 8 maps to the image row every other kernel forms.  Strips of whole tile rows (strip_rows % 8 == 0) keep
// every strip quantity wave-uniform: the tile's first image row is scalar and the lane adds its offset; only a strip that
// cuts a tile takes the per-lane division, as k_trace_pool_f64 does around rows_aligned.  An owned row at or beyond
// owned_rows (a last tile row that hangs over) lies in a strip that starts below the image: its image row is >= height.
__device__ __forceinline__ int stream_image_row(const RT_CONSTANT TraceArgs *K, int ty, int lane) {
    const int sub = lane >> 3;
    const int strip_count = K->strip_count;
    if (strip_count <= 1) return ty * 8 + sub;
    const int strip_rows = K->strip_rows, strip_index = K->strip_index;
    if ((strip_rows & 7) == 0) {
        const int q = (ty * 8) / strip_rows; // wave-uniform
        return (q * strip_count + strip_index) * strip_rows + (ty * 8 - q * strip_rows) + sub;
    }
    const int vrow = ty * 8 + sub;
    return ((vrow / strip_rows) * strip_count + strip_index) * strip_rows + vrow % strip_rows;
}

// ... as a call, for the tile prologue of the kernel: the strip road's registers are the callee's, live for the length of
// the call and not beside the path loop's (the kernel has almost none to spare: DESIGN.md 4.10).  Only called with strips.
__device__ __noinline__ int stream_image_row_strips(const RT_CONSTANT TraceArgs *K_in, int ty) {
    const uint64_t bits = (uint64_t)K_in; // (arguments travel in VGPRs: readfirstlane makes them scalar again)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bits);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bits >> 32));
    const RT_CONSTANT TraceArgs *K = (const RT_CONSTANT TraceArgs *)(((uint64_t)hi << 32) | lo);
    return stream_image_row(K, __builtin_amdgcn_readfirstlane(ty), (int)(threadIdx.x & 63));
}

// The end of a tile: its pixels into TraceArgs.deliver_out (tile-column layout, rt_device_types.h), then the region's
// counter and — by the wave that finishes the region — its flag: k_trace_pool_f64's deliver_item from the release fence
// on, the hand-off that has been soaked on hardware.  Out of line, and fed the item number alone: the tile's coordinates
// are formed again here rather than kept in scalar registers across the path loop, which has none to spare.
__device__ __noinline__ void stream_deliver_tile(const RT_CONSTANT TraceArgs *K_in, uint32_t item, double sum0, double sum1, double sum2,
                                                 double scale) {
    const int lane = threadIdx.x & 63;
    const RT_CONSTANT TraceArgs *K;
    { // function arguments travel in VGPRs; readfirstlane tells the backend that these are wave-uniform (scalar loads)
        const uint64_t bits = (uint64_t)K_in;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bits);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bits >> 32));
        K = (const RT_CONSTANT TraceArgs *)(((uint64_t)hi << 32) | lo);
    }
    item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
    int region, tx, ty;
    uint32_t reg_tiles;
    stream_tile_of(K, item, region, tx, ty, reg_tiles);
    const int px = tx * 8 + (lane & 7), py = stream_image_row(K, ty, lane); // the IMAGE row: deliver_out is the whole frame's
    if (px < K->width && py < K->height) {
        // column `col` starts at pixel column col * step and is stored as [height][its width][3] behind the columns before it
        int col = px / K->deliver_col_step;
        if (col > K->deliver_cols - 1) col = K->deliver_cols - 1;
        const int col_x = col * K->deliver_col_step;
        const int col_w = col == K->deliver_cols - 1 ? K->width - col_x : K->deliver_col_step;
        double *out = K->deliver_out + ((size_t)K->height * (size_t)col_x + (size_t)py * (size_t)col_w + (size_t)(px - col_x)) * 3;
        out[0] = sqrt(scale * sum0); // k_resolve_f64's arithmetic with the host's reciprocal: rt_render_frame_nee's pixel
        out[1] = sqrt(scale * sum1);
        out[2] = sqrt(scale * sum2);
    }
    // The pixels sit in HOST memory: release them at system scope before this tile is counted, and publish the region
    // behind an acquire of the other waves' releases.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    uint32_t tiles_before = 0;
    if (lane == 0) tiles_before = __hip_atomic_fetch_add(K->region_done + region, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tiles_before = (uint32_t)__builtin_amdgcn_readfirstlane((int)tiles_before);
    if (tiles_before == reg_tiles - 1u) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (lane == 0) {
            __hip_atomic_store(K->region_done + region, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // re-armed for the next launch
            __hip_atomic_store(K->deliver_flags + region, K->deliver_serial, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH, class LIGHTS>
__device__ __forceinline__ void nee_stream(const TraceArgs &A, const NeeArgs &N, const typename LIGHTS::Args &X) {
    constexpr unsigned SHAPE = kStreamShape<PRIMS, TEXTURED, SPECULAR, BVH>;
    const int lane = threadIdx.x & 63;
    unsigned int n_segments = 0, n_started = 0;
    for (;;) {
        uint32_t item = 0x80000000u;
        if (lane == 0) {
            const unsigned int *cf = kernargs_here()->cancel_flag;
            unsigned int up = 0u;
            if (cf != nullptr) up = __hip_atomic_load(cf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (up == 0u) item = atomicAdd(A.queue, 1u);
        }
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= A.n_items) break; // the queue is dry, poisoned, or the word is up
        int region, tx, ty;
        uint32_t reg_tiles;
        stream_tile_of(kernargs_here(), item, region, tx, ty, reg_tiles);
        const int px = tx * 8 + (lane & 7);
        int py = ty * 8 + (lane >> 3);
        if (kernargs_here()->strip_count > 1) py = stream_image_row_strips(kernargs_here(), ty); // owned row -> image row, once per tile
        const RT_CONSTANT TraceArgs *K = kernargs_here();
        const bool from_copy = (SHAPE & STREAM_PROLOGUE_FROM_COPY) != 0u;
        // (the width through kernargs_here() in both shapes: with the row map above, a copy-shaped prologue that also takes the
        // width from the copy brings the unused stack frame back to fast (0,1,1,0); height and seeds stay the shape's)
        const int width = K->width;
        const bool in_image = px < width && py < (from_copy ? A.height : K->height);

        PathRng rng;
        rng.pixel = (uint32_t)py * (uint32_t)width + (uint32_t)px;
        rng.k0 = from_copy ? A.seed_lo : K->seed_lo;
        rng.k1 = from_copy ? A.seed_hi : K->seed_hi;

        const double u = pixel_jitter(rng, px, width);

        d3 sum = mk(0.0, 0.0, 0.0); // the pixel's sum, carried from chunk to chunk
        unsigned int up = 0u;
        for (int s0 = 0; s0 < ((SHAPE & STREAM_LOOP_FROM_KERNARGS) ? kernargs_here()->samples : A.samples); s0 += kNeeStreamChunk) {
            { // (asked only while it is down: 4 000 cancelled waves asking again at every chunk they idle through is what the link serves slowest)
                const unsigned int *cf = kernargs_here()->cancel_flag;
                if (cf != nullptr && lane == 0 && up == 0u) up = __hip_atomic_load(cf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                up = (unsigned int)__builtin_amdgcn_readfirstlane((int)up);
            }
            const int s1 = s0 + kNeeStreamChunk < A.samples ? s0 + kNeeStreamChunk : A.samples;
            nee_samples<PRIMS, TEXTURED, SPECULAR, BVH, LIGHTS>(A, N, rng, px, py, u, in_image && up == 0u ? s0 : s1, s1, sum, n_segments, n_started, X);
        }
        if (up == 0u) stream_deliver_tile(kernargs_here(), item, sum.x, sum.y, sum.z, N.inv_samples);
    }
    wave_stat_add(A, lane, RT_STAT_SEGMENTS, n_segments); // path segments (shadow rays excluded)
    wave_stat_add(A, lane, RT_STAT_SAMPLES, n_started);   // primary rays
}

} // namespace RT_KNS
