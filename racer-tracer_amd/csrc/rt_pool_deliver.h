// rt_pool_deliver.h — the in-launch hand-off of finished tiles to the host (TraceArgs.deliver_out): deliver_item of the
// pooled trace kernel (rt_trace_pool_kernel.hip).
#pragma once
#include "rt_trace_common.h"

namespace RT_KNS {

// DELIVERY: what a delivering launch does at the end of an item (rt_device_types.h: TraceArgs.deliver_out).  Out of
// line on purpose: inlined, its address arithmetic and loads raised the register count of the whole path loop
// (80 -> 89 VGPRs in the plain variants, i.e. five blocks per CU instead of six).
__device__ __noinline__ void deliver_item(const RT_CONSTANT TraceArgs *K_in, double sum0, double sum1, double sum2, bool my_valid, int chunk,
                                          int tx, int ty, int tile_py0, bool rows_aligned, int region, uint32_t reg_tiles) {
    const int lane = threadIdx.x & 63;
    const RT_CONSTANT TraceArgs *K;
    // K: the launch's own argument block in the kernarg segment, handed in by the kernel (a by-reference copy of `A` would
    // live in scratch, and llvm.amdgcn.kernarg.segment.ptr is NULL outside a kernel).  Function arguments travel in
    // VGPRs; readfirstlane tells the backend that this one is wave-uniform, so its fields come by scalar loads.
    {
        const uint64_t bits = (uint64_t)K_in;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bits);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bits >> 32));
        K = (const RT_CONSTANT TraceArgs *)(((uint64_t)hi << 32) | lo);
    }
    chunk = __builtin_amdgcn_readfirstlane(chunk);
    tx = __builtin_amdgcn_readfirstlane(tx);
    ty = __builtin_amdgcn_readfirstlane(ty);
    tile_py0 = __builtin_amdgcn_readfirstlane(tile_py0);
    region = __builtin_amdgcn_readfirstlane(region);
    reg_tiles = (uint32_t)__builtin_amdgcn_readfirstlane((int)reg_tiles);
    {
        const size_t slice = (size_t)K->slice_rows * (size_t)K->width * 3; // a slice holds the launch's owned rows only
        // (pixel coordinates are formed again here rather than kept in registers across the path loop)
        const int out_px = (tx * 8 + (lane & 7)) * K->step_x;
        int out_py = tile_py0 + (lane >> 3) * K->step_y;
        if (!rows_aligned) {
            const int vrow = ty * 8 + (lane >> 3);
            out_py = ((vrow / K->strip_rows) * K->strip_count + K->strip_index) * K->strip_rows + vrow % K->strip_rows;
        }
        const size_t in_slice = ((size_t)(ty * 8 + (lane >> 3)) * (size_t)K->width + (size_t)out_px) * 3;
        double *dst = K->partial + (size_t)(K->chunk_base + chunk) * slice + in_slice;
        // ---- DELIVERY: the launch finishes its own pixels (rt_device_types.h: TraceArgs.deliver_out).
        // The slices cross waves inside ONE launch here, and an XCD's L2 is not coherent with its seven neighbours':
        // a device-scope release fence per item (L2 write-back + invalidate) was measured first and costs C2 12 %
        // (profiles/r03_fence_probe.txt).  Instead the slice stores and loads are device-scope relaxed atomics —
        // plain stores / loads with the sc1 bit, which write through to / read from the level all XCDs share — and
        // s_waitcnt orders this wave's stores before its bump of the tile's counter: no cache maintenance at all.
        if (my_valid) {
            __hip_atomic_store(dst + 0, sum0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(dst + 1, sum1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(dst + 2, sum2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the stores have been acknowledged at device scope
        const int tile_id = ty * K->tiles_x + tx;
        uint32_t chunks_before = 0;
        if (lane == 0) chunks_before = __hip_atomic_fetch_add(K->tile_done + tile_id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        chunks_before = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunks_before);
        if ((int)chunks_before != K->total_chunks - 1) return;
        // Every chunk of this tile has landed: vec3.rs:119-125 scale_sqrt over the slices in chunk order —
        // exactly k_resolve_chunks_f64's sum, so the pixels are bit-identical to the two-pass path.
        if (my_valid) {
            const double *src = K->partial + in_slice;
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
#pragma unroll 1
            for (int c = 0; c < K->total_chunks; ++c) {
                acc0 += __hip_atomic_load(src + (size_t)c * slice + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                acc1 += __hip_atomic_load(src + (size_t)c * slice + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                acc2 += __hip_atomic_load(src + (size_t)c * slice + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const double scale = 1.0 / (double)K->samples; // what rtdev_launch_resolve_chunks passes
            // tile-column layout of the output (one column = the plain frame): column `col` starts at pixel column
            // col * step and is stored as [height][its width][3] behind the columns before it
            int col = out_px / K->deliver_col_step;
            if (col > K->deliver_cols - 1) col = K->deliver_cols - 1;
            const int col_x = col * K->deliver_col_step;
            const int col_w = col == K->deliver_cols - 1 ? K->width - col_x : K->deliver_col_step;
            double *out = K->deliver_out + ((size_t)K->height * (size_t)col_x + (size_t)out_py * (size_t)col_w + (size_t)(out_px - col_x)) * 3;
            out[0] = sqrt(scale * acc0);
            out[1] = sqrt(scale * acc1);
            out[2] = sqrt(scale * acc2);
        }
        if (lane == 0) __hip_atomic_store(K->tile_done + tile_id, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // re-armed for the next launch on this scene (written through, like the slices)
        // The pixels may sit in HOST memory: release them at system scope before this tile is counted (once per
        // tile, 1/19 of the items on C3), and publish the region behind an acquire of the other waves' releases.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        uint32_t tiles_before = 0;
        if (lane == 0) tiles_before = __hip_atomic_fetch_add(K->region_done + region, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tiles_before = (uint32_t)__builtin_amdgcn_readfirstlane((int)tiles_before);
        if (tiles_before == reg_tiles - 1u) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if (lane == 0) {
                __hip_atomic_store(K->region_done + region, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(K->deliver_flags + region, K->deliver_serial, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

} // namespace RT_KNS
