// rt_trace_pool_kernel.hip — the default trace kernel (f64): persistent waves
// over a queue of (8x8 pixel tile, sample chunk) items, lanes drawing paths
// from the item's pool, wave-cooperative rejection sampling.
//
// Replaces CpuRenderer::raytrace's pixel x sample loop
// (racer-tracer/src/renderer/cpu.rs:26-71) and the recursive ray_color
// (renderer.rs:41-90).  The ideas, all measured against the v1 kernel
// (rt_trace_kernel.hip) on cornell_box 1080p:
//
// 1. PERSISTENT WAVES + ITEM QUEUE.  The grid is sized to what is resident
//    (CUs x blocks per CU); every wave pulls items from one atomic counter
//    until the queue is dry.  An item is a tile x a chunk of its samples; the
//    chunk plan (rt_plan.cpp: chunk_plan, a function of spp only) has long chunks
//    first and a taper of short ones last, so a launch ends on small items.
//
// 2. LANES ARE NOT PIXELS.  Inside an item the 64 lanes share a pool of
//    64 x chunk (pixel, sample) paths: whenever lanes have no path in flight a
//    ballot + prefix count hands them the next pool entries.  No lane waits for
//    the slowest pixel of its tile; ray state (origin, direction, throughput)
//    lives in VGPRs and never touches HBM.  Finished samples are added to the
//    tile's 64 pixel sums in LDS (ds_add_f64); the item's sums go to its own
//    slice partial[chunk][pixel], and k_resolve adds slices in index order, so
//    the frame is deterministic and independent of scheduling.
//
// 3. COOPERATIVE REJECTION SAMPLING.  random_in_unit_sphere (vec3.rs:424-430)
//    loops until a candidate falls inside the sphere; per lane that is 1.9
//    iterations on average but a wave pays for its slowest lane (~6.4).
//    Because every draw is ADDRESSED (include/rt_rng.h) — candidate i of a
//    path is a pure function of (pixel, sample, segment, i): ONE Philox block,
//    three 42-bit coordinates — any lane can evaluate any lane's candidate.  Each round the lanes that still need a
//    sample post a request in LDS, the 64 lanes split into groups that test
//    consecutive candidates of one request each, and a ballot picks the first
//    accepted candidate in stream order.  ~3 rounds instead of ~6.4, identical
//    values (the accepted candidate is exactly the one the sequential loop
//    would have stopped at).
//
// 4. REGENERATION BATCHES.  Pool entries leave in index order, so the camera samples
//    (vertical jitter, ray time, lens disk) of 64 consecutive entries are drawn by the
//    whole wave into LDS ahead of the hand-out instead of by the ~16 lanes that start a
//    path in a given iteration.
//
// 5. UNIFORMS ARE RE-READ WHERE THEY ARE USED (kernargs_here): camera and background would
//    otherwise sit in SGPRs across the path loop and be spilled to VGPR lanes.
//
// 6. NO SCALAR SWITCH IN THE CLOSEST-HIT LOOP.  The device table is grouped by kind (plain XY / XZ / YZ
//    rects, plain spheres, the rest); each group gets one straight-line test with the plane a compile-time
//    constant.  With a wave-uniform index the `match` on a record's kind was scalar control flow, ~25 SALU
//    instructions and half a dozen branches around 12 vector instructions per rect.  In the rects-only plain variant a
//    FACING PAIR of rects (two walls on parallel planes with the same bounds: rt_rect_pairs.h) costs a lane ONE rect test,
//    on the record its direction points at, whenever the other plane lies behind t_min in every lane of the wave.
//
// 7. THE ONE EXPENSIVE TEXTURE IS EVALUATED BY THE WHOLE WAVE (coop_noise_turbulence): lanes only note
//    their Noise lookup while shading; eight lookups per round take eight lanes each, one octave per lane.
//
// 8. A PATH CARRIES ORIGIN, DIRECTION, THROUGHPUT AND NOTHING ELSE WHILE IT WAITS.  A hit's point overwrites the ray
//    origin, its attenuation is multiplied into the throughput at once, a Lambertian hit's normal overwrites the ray
//    direction (the incoming one is dead), and a finished path's contribution is formed in the throughput.  Every
//    value kept beside those cost registers and, where the material arms meet, a copy per arm.
//
// 9. TWO ITEMS IN FLIGHT (the variants with any primitive kind or a BVH).  The lanes an item's last paths no longer need
//    start the NEXT item's paths; per-pixel sums are 64-bit fixed-point integers, so the order in which samples arrive —
//    which now depends on what else the wave traces — cannot change a bit of the frame (SUMS AND OVERLAPPED ITEMS below).
//
// 10. PRIMARY SEGMENTS ARE TRACED IN THE CAMERA BATCHES (the rects-only plain variant, C3's, in both arithmetic flavours).
//    The batch of idea 4 forms the rays of its 64 entries and runs the closest-hit loop on them, all lanes busy and the
//    rays coherent; an entry whose path ends on that segment (a miss, a light, max_depth <= 1) adds its contribution there
//    and never takes a lane, the others wait in a ring of 67 slots in LDS with the POINT of their hit, their primitive and
//    the signs of their ray (30 bytes each).  The path loop of that variant is ROTATED: hand-out from the ring, shade the
//    pending hits, sampler, new direction, trace, ends — so a lane that takes an entry loads a point and traces the path's
//    SECOND segment in the same iteration; it forms no camera ray (LABNOTES R19.1).  Every sample keeps its bits; the
//    order in which an item's samples reach its sums changes (spp 1 and 2 frames are bit-identical to the old loop's).
//    C3 59.6 -> 56.4 ms (LABNOTES R10.1).  The other variants keep the loop of ideas 1 - 9.
//    An item none of whose pixels can see the scene takes no batch at all, and a batch tests only the rects — and forms
//    the ray's reciprocal only on the planes — that some pixel of its item can see (rt_primary_bounds.h; start_item).
//
// The launch is VALU-throughput bound with the CU's one scalar ALU close behind (scalar_busy 0.60 on C3: count scalar
// instructions before vector ones; DESIGN.md 4.2 / 6 and LABNOTES.md have the counters, the per-region cycle profile of the
// -DRT_PROFILE_REGIONS build — which adds 1.8 KB of LDS per block and can cost a variant at a granule edge a block per CU —
// and the variants that were measured and dropped).
#include <cstddef>
#include <type_traits>
#include "rt_trace_common.h"
#include "rt_primary_bounds.h"
#include "rt_variant_dispatch.h"
#include "rt_pool_profile.h"
#include "rt_pool_lds.h"
#include "rt_pool_coop.h"
#include "rt_ring_level.h"
#include "rt_pool_deliver.h"

#ifndef RT_OCC_TEX
#define RT_OCC_TEX 4 // textured spheres-only / rects-only variants: 40 KB of LDS per block still fits four (C4 +3 %)
#endif
#ifndef RT_OCC_TEX_BVH
#define RT_OCC_TEX_BVH 4 // textured BVH variants: 32-byte nodes and no Perlin table in static LDS leave room for four blocks (random scene +20 %)
#endif
#ifndef RT_OCC_TEX_ANY
#define RT_OCC_TEX_ANY 4 // textured linear-loop variants with any primitive kind (emissive.yml 24.5 -> 22.8 ms against three)
#endif
#ifndef RT_OCC_SPEC
#define RT_OCC_SPEC 5
#endif
#ifndef RT_OCC_ANY
#define RT_OCC_ANY 5 // untextured linear-loop variants with any primitive kind (cornell_box_boxes: 4 -> 5 waves per SIMD 20.7 -> 19.3 ms)
#endif
#ifndef RT_OCC_PLAIN
#define RT_OCC_PLAIN 7 // rects-only / spheres-only, no textures, no specular materials: 72 VGPRs, seven blocks per CU when LDS allows (C3 73.4 ->
                       // 72.0 ms against six).  Six needed 80 of the 79 the allocator wanted until the path state was re-set between
                       // items (its live ranges then end at the path loop's exit: 73); the bound keeps the allocator there.
#endif
namespace RT_KNS {

// BVH: closest hit through the skip-link hierarchy instead of the linear loop
// (instantiated for PRIMS_ANY only; chosen for scenes with many primitives).
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
__global__ __launch_bounds__(256, TEXTURED ? (PRIMS == PRIMS_ANY ? (BVH ? RT_OCC_TEX_BVH : RT_OCC_TEX_ANY) : RT_OCC_TEX) : (BVH ? 4 : (PRIMS == PRIMS_ANY ? RT_OCC_ANY : (SPECULAR ? RT_OCC_SPEC : RT_OCC_PLAIN)))) void k_trace_pool_f64(const TraceArgs A, const rtdev::PrimaryRects) {
    // (the second argument, the rect records' pixel rectangles, is read by the PRETRACE variant alone, through the kernel
    // argument segment where it is used: primary_rects_here)
    // Two batches of camera samples stay ahead of the hand-out, so that it may straddle a batch
    // boundary; the BVH variants keep one (their node array wants the LDS: three resident blocks
    // instead of two on the `random` scene) and a hand-out stops at the end of its batch.
    constexpr int NBUF = BVH ? 1 : 2;
    // Two items in flight where it pays: the variants whose iterations are long (any primitive kind, BVH).  The rects-only
    // and spheres-only variants gain under 1 % from it (their tail iterations are cheap: no hand-out, no batches, one sampler
    // round) and lose 2 % to the bookkeeping, so they keep one item at a time and f64 sums.
#if defined(RT_EXACT_DIV) || defined(RT_NO_OVERLAP)
    constexpr bool OVERLAP = false;
#else
    constexpr bool OVERLAP = BVH || PRIMS == PRIMS_ANY;
#endif
    // PRIMARY SEGMENTS IN THE BATCHES (the rects-only plain variant, both arithmetic flavours): see the path loop below.
#ifdef RT_NO_PRETRACE
    constexpr bool PRETRACE = false;
#else
    constexpr bool PRETRACE = PRIMS == PRIMS_RECTS && !TEXTURED && !SPECULAR && !BVH;
#endif
    using Lds = std::conditional_t<PRETRACE, PretraceLds, WaveLds<TEXTURED, NBUF, OVERLAP>>;
    __shared__ Lds lds_all[4];
    // Dynamic LDS of a block: [BVH nodes | primitive table + texture table][Perlin gradients][lens samples][ray times];
    // the host sizes it (rt_device_types.h: pool_lds_layout, whose order the offsets below follow) and says what is in it.
    extern __shared__ __align__(16) unsigned char dyn_lds[];
    // The gradients of the first Perlin table (6 KB) are staged in LDS once per block when the
    // permutation tables are the identity (always, in the reference: noise.rs:121-130): the 56
    // random gradient fetches of a marble lookup then hit LDS instead of the vector memory
    // path, and the lattice hash needs no table.  Scenes without a Noise texture do not pay the 6 KB.
    struct PerlinGradients {
        double ranvec[256][3];
    };
    static_assert(offsetof(Perlin, ranvec) == 0, "the gradients lead the Perlin record");
    const Perlin *lds_perlin = nullptr;
    if (TEXTURED) {
        if (A.perlin_in_lds) {
            const size_t at = BVH ? (size_t)A.bvh_lds_nodes * sizeof(BvhNode)
                                  : (size_t)A.n_prims * sizeof(Prim) + (size_t)A.n_textures * sizeof(Texture);
            const uint64_t *src = reinterpret_cast<const uint64_t *>(A.perlins);
            uint64_t *dst = reinterpret_cast<uint64_t *>(dyn_lds + at);
            for (int i = threadIdx.x; i < (int)(sizeof(PerlinGradients) / 8); i += 256) dst[i] = src[i];
            lds_perlin = reinterpret_cast<const Perlin *>(dyn_lds + at); // only .ranvec is read (IDENTITY path)
        }
        __syncthreads();
    }
    // the lens-disk samples of this wave's batches: [NBUF][64][2] doubles per wave behind the tables above (see WaveLds)
    double (*lens)[64][2] = nullptr;
    if (A.lens_lds) {
        size_t at = BVH ? (size_t)A.bvh_lds_nodes * sizeof(BvhNode)
                        : (size_t)A.n_prims * sizeof(Prim) + (TEXTURED ? (size_t)A.n_textures * sizeof(Texture) : 0);
        if (TEXTURED && A.perlin_in_lds) at += sizeof(PerlinGradients);
        lens = reinterpret_cast<double (*)[64][2]>(dyn_lds + at) + (threadIdx.x >> 6) * NBUF;
    }
    // ... and the ray times of the batches, [NBUF][64] doubles per wave behind those: only a scene with a MovingSphere reads a
    // ray's time (ray.rs:26-28), and without their 1 KB per wave more blocks fit a CU
    double (*ray_times)[64] = nullptr;
    if (PRIMS == PRIMS_ANY && A.time_lds) {
        size_t at = BVH ? (size_t)A.bvh_lds_nodes * sizeof(BvhNode)
                        : (size_t)A.n_prims * sizeof(Prim) + (TEXTURED ? (size_t)A.n_textures * sizeof(Texture) : 0);
        if (TEXTURED && A.perlin_in_lds) at += sizeof(PerlinGradients);
        if (A.lens_lds) at += (size_t)4 * NBUF * 64 * 2 * sizeof(double); // rt_device_types.h: pool_lens_lds_bytes
        ray_times = reinterpret_cast<double (*)[64]>(dyn_lds + at) + (threadIdx.x >> 6) * NBUF;
    }
    // BVH nodes are staged in dynamic LDS when they fit (the host sets bvh_lds_nodes):
    // a traversal step is a dependent load, and ~100 steps at
    // L2 latency with 3-4 waves per SIMD is what bounds the big-scene variants.
    const BvhNode *lds_nodes = nullptr;
    if (BVH && A.bvh_lds_nodes > 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(A.bvh_nodes);
        uint4 *dst = reinterpret_cast<uint4 *>(dyn_lds);
        for (int i = threadIdx.x; i < A.bvh_lds_nodes * (int)(sizeof(BvhNode) / 16); i += 256) dst[i] = src[i];
        lds_nodes = reinterpret_cast<const BvhNode *>(dyn_lds);
        __syncthreads();
    }
    // The linear-loop variants stage the whole primitive table (192 B each, materials included)
    // in dynamic LDS instead: the closest-hit loop keeps reading it through the scalar cache, but
    // the per-lane fetch of the WINNING primitive for shading is then an LDS read, not a trip
    // through the vector memory path in the middle of every iteration.
    const Prim *lds_prims = nullptr;
    if (!BVH) {
        const uint4 *src = reinterpret_cast<const uint4 *>(A.prims);
        uint4 *dst = reinterpret_cast<uint4 *>(dyn_lds);
        for (int i = threadIdx.x; i < A.n_prims * (int)(sizeof(Prim) / 16); i += 256) dst[i] = src[i];
        lds_prims = reinterpret_cast<const Prim *>(dyn_lds);
        __syncthreads();
    }
    // ... and the texture table (64 B each) behind it: a Checkered lookup is a dependent chain
    // texture -> sub-texture
    const Texture *lds_textures = nullptr;
    if (!BVH && TEXTURED) {
        const uint4 *src = reinterpret_cast<const uint4 *>(A.textures);
        uint4 *dst = reinterpret_cast<uint4 *>(dyn_lds + (size_t)A.n_prims * sizeof(Prim));
        for (int i = threadIdx.x; i < A.n_textures * (int)(sizeof(Texture) / 16); i += 256) dst[i] = src[i];
        lds_textures = reinterpret_cast<const Texture *>(dyn_lds + (size_t)A.n_prims * sizeof(Prim));
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int lane_of_wave = lane;
    Lds &L = lds_all[threadIdx.x >> 6];
    unsigned int n_segments = 0, n_started = 0;
    if ((OVERLAP || PRETRACE) && lane < 3) L.ulc[lane] = A.cam.ulc[lane];
    if constexpr (PRETRACE) {
        if (lane < 3) {
            L.cam_origin[lane] = A.cam.origin[lane];
            L.bg_top[lane] = A.bg.top[lane];
        }
        L.n_started = 0u; // (every lane: a `lane == 0` here is kept, as a lane mask, for the kernel's last lines)
    }

    // SUMS AND OVERLAPPED ITEMS.  When the pool of an item is dry its last paths still take a dozen iterations to end, with
    // ever fewer lanes tracing (`random`: 14 % of a wave's iterations ran at 14 lanes, cornell_box_boxes 13 % at 19, C4
    // 6 % at 19; profiles/r04_region_cycles.txt).  With per-pixel sums kept as doubles the wave has to sit that tail out: the
    // order in which an item's samples reach its sums — hence their rounding — must not depend on what else the wave is
    // doing, or the frame would depend on which wave drew which item.  The OVERLAP variants keep the sums as INTEGERS
    // instead (TraceArgs.sum_scale: the scene's radiance is bounded, so a sample fits a 52-bit fixed-point number) — exact,
    // so their order does not matter — and draw the next item the moment the pool runs dry: two items are in flight, the
    // lanes the old one frees start the new one's paths (cornell_box_boxes -5 %, `random` -2.5 % of the frame time; the
    // frame is then also the same for strips that cut the item tiles: tests/test_gpu_overlap.py).  The other variants,
    // and every RT_ARITH_REFERENCE kernel, add doubles and start the next item after the last path.  (A scene without a
    // radiance bound — a colour above 1 on a scattering material — is given to the RT_ARITH_REFERENCE copy by the host.)
    //
    // The wave-uniform flags of this bookkeeping are bits of ONE integer and the tests on them integer compares: as `bool`s
    // they lived in 64-bit lane masks, which the path loop's scalar register pressure sent to VGPR lanes — a dozen v_readlane
    // per iteration.  They are also made opaque where the path loop tests them: a loop-invariant test is hoisted out of the
    // loop AS A LANE MASK, with the same fate.
    constexpr bool FIXED_SUMS = OVERLAP;
#ifdef RT_EXACT_DIV
    const uint32_t sum_scale_hi = 0u;
#else
    const uint32_t sum_scale_hi = (uint32_t)((unsigned long long)__double_as_longlong(A.sum_scale) >> 32); // 2^k: the lower half is 0
#endif
    // ---- the item entries are handed out of (slot `cur` of L.sum / L.info); the other slot may hold an item whose
    // pool is dry and whose last paths are still in flight (`draining`)
    // HAVE: slot `cur` holds an item (its pool may be dry); CUR: cur << 6, the slot bit as it sits in a lane's `spix`
    // POOL_DRY (two-item variants): the hand-out has just taken the pool's last entries
    enum : uint32_t { HAVE = 1u, DRAINING = 2u, QUEUE_DRY = 4u, POOL_DRY = 8u, CUR = 64u };
    uint32_t state = 0u;
    int smp0 = 0, n_valid = 0;
    int tile_py0 = 0; // image row of the current tile's first row; -1: strips that cut tiles (the batches then take the long road)
    uint32_t total = 0, next = 0, n_batches = 0, batches_done = 0;
    // `next` at which the next batch of camera samples is due (batch b when next >= (b - (NBUF - 1)) * 64: NBUF batches stay
    // ahead of the hand-out), or ~0 when the item's batches are all drawn: ONE scalar compare per iteration decides
    uint32_t batch_due = ~0u;
    uint32_t ring_head = 0; // PRETRACE: slot of the ring's oldest entry
    // PRETRACE: the entries that wait in the ring, kept as a counter, and the level below which a camera batch is due
    // (rt_ring_level.h; 0 once the item's batches are all drawn).  `next` is not kept up inside that variant's path loop:
    // it is the pool's index in front of the loop (0) and behind it (total).
    uint32_t ring_level = 0, batch_below = 0;
    uint32_t my_pixel = 0; // image index of this lane's pixel of the current item's tile

    RT_REGION_DECL
    // Draws the wave's next item and sets slot `cur` up for it; false when the queue is dry.  (All 64 lanes.)
    auto start_item = [&]() -> bool {
        // (an opaque copy of the lane index: whatever of the code below depends on the lane alone would otherwise be computed
        // once, in front of the loops, and parked in scratch memory across them — the plain variants have none)
        int lane = lane_of_wave;
        asm volatile("" : "+v"(lane));
        uint32_t item = 0;
        if (lane == 0) {
            item = atomicAdd(A.queue, 1u);
            // The host's cancel word (rt_device_types.h: cancel_flag).  Reads of pinned host memory are a scarce resource —
            // every item of every wave asking cost rt_render 30 % on C3 (615 000 items, ~28 M such reads per second is
            // what the link gives) — so only the wave that draws an item whose number is a multiple of 32 asks, and when
            // the word is up it poisons the launch's item counter ITSELF: every other wave's next atomicAdd then returns
            // "queue dry".  On C3 an item is drawn every 0.12 us, so somebody asks every 4 us.
            const unsigned int *cf = kernargs_here()->cancel_flag;
            if (cf != nullptr && (item & 31u) == 0u && item < A.n_items &&
                __hip_atomic_load(cf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) {
                atomicOr(A.queue, 0x80000000u);
                item = 0x80000000u;
            }
        }
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= A.n_items) return false;
        // item -> (region, chunk, tile): regions in queue order, chunk-major inside a region (rt_device_types.h: Region)
        int region = 0, reg_tx0 = 0, reg_ty0 = 0, reg_ntx = A.tiles_x;
        uint32_t reg_tiles = (uint32_t)A.n_tiles, local = item;
        if constexpr (PRETRACE) {
            // (the region count opaque, where the path loop leaves no scalar register to spare: n_regions - 1 would be formed
            // in front of the loops and parked in a VGPR lane across them)
            int n_regions = A.n_regions;
            asm volatile("" : "+s"(n_regions));
            if (n_regions > 1) {
                const RT_CONSTANT TraceArgs *K = kernargs_here();
                while (region + 1 < n_regions && item >= K->regions[region + 1].item_begin) ++region;
                local = item - K->regions[region].item_begin;
                reg_tx0 = K->regions[region].tx0;
                reg_ntx = K->regions[region].ntx;
                reg_ty0 = K->regions[region].ty0;
                reg_tiles = (uint32_t)reg_ntx * (uint32_t)K->regions[region].nty;
            }
        } else if (A.n_regions > 1) {
            const RT_CONSTANT TraceArgs *K = kernargs_here();
            while (region + 1 < A.n_regions && item >= K->regions[region + 1].item_begin) ++region;
            local = item - K->regions[region].item_begin;
            reg_tx0 = K->regions[region].tx0;
            reg_ntx = K->regions[region].ntx;
            reg_ty0 = K->regions[region].ty0;
            reg_tiles = (uint32_t)reg_ntx * (uint32_t)K->regions[region].nty;
        }
        // the adaptive passes (one region): the launch's tiles are a list, one wave-uniform load per item
        const uint32_t *tile_list = kernargs_here()->tile_list;
        if (tile_list != nullptr) reg_tiles = kernargs_here()->n_list;
        const uint32_t chunk = local / reg_tiles;
        uint32_t tile = local - chunk * reg_tiles;
        if (tile_list != nullptr) tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_list[tile]);
        const int ty = reg_ty0 + (int)(tile / (uint32_t)reg_ntx);
        const int tx = reg_tx0 + (int)(tile % (uint32_t)reg_ntx);
        const int cur = (int)(state >> 6) & 1;
        int n_smp; // the chunk's samples (chunk = index within this launch)
        {
            const RT_CONSTANT TraceArgs *K = kernargs_here();
            smp0 = K->chunk_start[A.chunk_base + (int)chunk];
            n_smp = K->chunk_start[A.chunk_base + (int)chunk + 1] - smp0;
        }

        // ---- this lane's pixel of the tile (used for the pool table and the hand-out's pixel index)
        // (step_x/step_y > 1: the preview renderer, cpu_scaled.rs — the grid cell is the
        // top-left pixel of a block, the resolve pass fills the block)
        // Image row of the tile's first row.  With strips of a multiple of 8 rows (what every multi-GPU host here
        // uses) a tile lies inside ONE strip, so the owned-row -> image-row map is one scalar division per item;
        // other strip heights take the per-lane division.
        const bool rows_aligned = A.strip_count <= 1 || (A.strip_rows & 7) == 0;
        tile_py0 = ty * 8 * A.step_y;
        if (A.strip_count > 1 && rows_aligned) {
            const int q = (ty * 8) / A.strip_rows; // wave-uniform
            tile_py0 = (q * A.strip_count + A.strip_index) * A.strip_rows + (ty * 8 - q * A.strip_rows);
        }
        const int my_px = (tx * 8 + (lane & 7)) * A.step_x;
        const int my_vrow = ty * 8 + (lane >> 3);
        int my_py = tile_py0 + (lane >> 3) * A.step_y;
        if (!rows_aligned)
            my_py = ((my_vrow / A.strip_rows) * A.strip_count + A.strip_index) * A.strip_rows + my_vrow % A.strip_rows;
        const bool my_valid = my_px < A.cover_w && my_vrow < A.owned_rows && my_py < A.height;
        my_pixel = (uint32_t)my_py * (uint32_t)A.width + (uint32_t)my_px;
        const uint64_t valid_mask = ballot(my_valid);
        n_valid = __popcll(valid_mask);
        // ITEMS NO CAMERA RAY CAN HIT (PRETRACE).  The host bounds the pixels whose camera rays can reach a primitive
        // (TraceArgs.cull_px0..; rt_primary_bounds.h).  In an item without such a pixel every path is one segment that misses:
        // with a solid background each of its n_smp samples adds `top` to its pixel, which is all the item's batches would
        // do — a Philox block, a ray, six rect tests and three LDS adds per sample.  So the item takes none of them: its sums
        // are formed below by the batches' own LDS additions (n_smp equal terms onto +0.0: no order to keep; NOT a
        // multiplication, which rounds once), the counters grow as the batches count, and its pool is empty, like that of an
        // item without a pixel: the outer loop goes from here to finish_item.
        // A sky background depends on the ray, and max_depth <= 0 ends every path white without a segment: the batches.
        bool culled = false;
        if constexpr (PRETRACE) {
            const RT_CONSTANT TraceArgs *K = kernargs_here();
            // (four comparisons ANDed in the scalar unit: written with && they are four nested branches)
            const int x0 = K->cull_px0, x1 = K->cull_px1, y0 = K->cull_py0, y1 = K->cull_py1;
            const uint64_t seen = valid_mask & ballot(my_px >= x0) & ballot(my_px <= x1) & ballot(my_py >= y0) & ballot(my_py <= y1);
            culled = seen == 0ull && K->bg.kind != RT_BG_SKY && K->max_depth >= 1;
            // RECTS NO CAMERA RAY OF THE ITEM CAN HIT.  The host also bounds the pixels that can see each of the table's first
            // records (PrimaryRects, the kernel's second argument): bit i of the item's mask says that some valid pixel of the
            // item lies inside record i's rectangle, and the item's batches step over the records whose bit is clear
            // (closest_hit_rects<false>) — such a record's test would change neither `best` nor `best_t` of any of their rays.
            // Per PIXEL, as above, not per tile box: strips that cut the tiles scatter an item's rows over the image.  The
            // bits of the records without a rectangle stay set.  The mask waits in LDS: a scalar register kept across the path
            // loop is one the loop has not got.
            uint32_t rect_mask = ~0u;
            if (!culled) {
                const RT_CONSTANT rtdev::PrimaryRects *R = primary_rects_here();
                const int n_rects = R->n;
                for (int i = 0; i < n_rects; ++i) {
                    const int rx0 = R->r[i].px0, rx1 = R->r[i].px1, ry0 = R->r[i].py0, ry1 = R->r[i].py1;
                    const uint64_t sees = valid_mask & ballot(my_px >= rx0) & ballot(my_px <= rx1) & ballot(my_py >= ry0) & ballot(my_py <= ry1);
                    if (sees == 0ull) rect_mask &= ~(1u << i);
                }
            }
            if (lane == 0) L.rect_mask = rect_mask;
        }
        {
            if (!culled) { // (a culled item forms no ray)
                uint32_t pixel_stream = RT_RNG_SAMPLE_PIXEL;
                // (opaque where the path loop leaves no register to spare: the products of the block's constant words would
                // otherwise be formed in front of the loops and parked in scratch memory across them)
                if constexpr (PRETRACE) asm volatile("" : "+s"(pixel_stream));
                PathRng prng{my_pixel, pixel_stream, A.seed_lo, A.seed_hi};
                u4 bj = prng.block(0, RT_RNG_PIXEL, 0);
                const RT_CONSTANT TraceArgs *K = kernargs_here();
                const double u = div_by((double)my_px + u53(bj.a, bj.b), (double)(A.width - 1), K->inv_width_m1); // cpu.rs:35-36
                if constexpr (OVERLAP || PRETRACE) {
                    L.u[lane] = u;
                } else {
                    const d3 base = ld3(K->cam.ulc) + u * ld3(K->cam.horizontal); // camera.rs:331, first two terms
                    L.base[lane][0] = base.x;
                    L.base[lane][1] = base.y;
                    L.base[lane][2] = base.z;
                }
            }
            // fixed-point sums: a sample arrives as the bit pattern of (T * scale + 2^52), i.e. 0x433 << 52 plus the
            // integer; the n_smp patterns' exponent fields are taken off here, once, instead of masked off every sample
            unsigned long long zero = FIXED_SUMS ? 0ull - (unsigned long long)n_smp * 0x4330000000000000ull : 0ull;
            if constexpr (PRETRACE) asm volatile("" : "+v"(zero)); // (as above)
            unsigned long long *sum = reinterpret_cast<unsigned long long *>(L.sum[cur * 64 + lane]);
            sum[0] = zero;
            sum[1] = zero;
            sum[2] = zero;
            if (my_valid) L.pix_of[lane_rank(valid_mask)] = lane;
            if (lane == 0) L.info[cur] = ItemInfo{(int)chunk, tx, ty, tile_py0, region, (int)reg_tiles, rows_aligned ? 1 : 0, 0};
        }
        if constexpr (PRETRACE) {
            if (culled) {
                const d3 bg = ld3(L.bg_top);
                if (bg.x != 0.0 || bg.y != 0.0 || bg.z != 0.0) // (wave-uniform; a black background leaves the sums at +0.0)
                    // (addressed by the kernel's own lane index: by the opaque copy, the zero stores above got a 64-bit address)
                    for (int k = 0; k < n_smp; ++k) { // vec3.rs:38-42 Color::add, once per sample
                        atomicAdd(&L.sum[lane_of_wave][0], bg.x);
                        atomicAdd(&L.sum[lane_of_wave][1], bg.y);
                        atomicAdd(&L.sum[lane_of_wave][2], bg.z);
                    }
                if (__builtin_amdgcn_inverse_ballot_w64(valid_mask)) n_segments += (unsigned int)n_smp; // one primary segment per path
                if (lane == 0) L.n_started += (uint32_t)n_valid * (uint32_t)n_smp;
            }
        }
        if (!rows_aligned) tile_py0 = -1;
        total = culled ? 0u : (uint32_t)n_valid * (uint32_t)n_smp; // paths in this item's pool
        next = 0;
        n_batches = (total + 63u) >> 6;
        batches_done = 0;
        batch_due = n_batches > 0u ? 0u : ~0u;
        ring_head = 0;
        ring_level = 0;
        batch_below = rt_ring::batch_below_of(0u, total, RING_SLOTS);
        return true;
    };
    // The item of slot `s` has no path left: its sums go to its own slice of `partial` (or the launch finishes the tile's
    // pixels itself: deliver_item).  (All 64 lanes.)
    auto finish_item = [&](int s) {
        int lane = lane_of_wave;
        asm volatile("" : "+v"(lane));
        const ItemInfo I = L.info[s];
        const int chunk = __builtin_amdgcn_readfirstlane(I.chunk), f_tx = __builtin_amdgcn_readfirstlane(I.tx),
                  f_ty = __builtin_amdgcn_readfirstlane(I.ty), f_py0 = __builtin_amdgcn_readfirstlane(I.tile_py0);
        const bool f_aligned = __builtin_amdgcn_readfirstlane(I.rows_aligned) != 0;
        const int f_px = (f_tx * 8 + (lane & 7)) * A.step_x;
        const int f_vrow = f_ty * 8 + (lane >> 3);
        int f_py = f_py0 + (lane >> 3) * A.step_y;
        if (!f_aligned) f_py = ((f_vrow / A.strip_rows) * A.strip_count + A.strip_index) * A.strip_rows + f_vrow % A.strip_rows;
        const bool f_valid = f_px < A.cover_w && f_vrow < A.owned_rows && f_py < A.height;
        double s0 = L.sum[s * 64 + lane][0], s1 = L.sum[s * 64 + lane][1], s2 = L.sum[s * 64 + lane][2];
        if (FIXED_SUMS) { // the integers, rounded ONCE to the nearest double; the scale is a power of two
            const double unscale = kernargs_here()->sum_unscale;
            s0 = (double)(unsigned long long)__double_as_longlong(s0) * unscale;
            s1 = (double)(unsigned long long)__double_as_longlong(s1) * unscale;
            s2 = (double)(unsigned long long)__double_as_longlong(s2) * unscale;
        }
        if (A.deliver_out == nullptr) {
            if (f_valid) {
                // slice row = row of the launch's owned-row grid (a share's slices hold its own rows only)
                const size_t in_slice = (size_t)f_vrow * (size_t)A.width + (size_t)f_px;
                double *dst = A.partial + ((size_t)(A.chunk_base + chunk) * (size_t)A.slice_rows * (size_t)A.width + in_slice) * 3;
                dst[0] = s0;
                dst[1] = s1;
                dst[2] = s2;
            }
        } else {
            deliver_item(kernargs_here(), s0, s1, s2, f_valid, chunk, f_tx, f_ty, f_py0, f_aligned, __builtin_amdgcn_readfirstlane(I.region),
                         (uint32_t)__builtin_amdgcn_readfirstlane(I.reg_tiles));
        }
    };
    // Pool entry w of the current item = (pixel w % n_valid of the tile, sample smp0 + w / n_valid).
    auto entry_of = [&](uint32_t w, int &py_out, uint32_t &pixel_out, uint32_t &sample_out, int &pix) { // (all 64 lanes: a lane shuffle)
        int s_off;
        if (n_valid == 64) {
            pix = (int)(w & 63u);
            s_off = (int)(w >> 6);
        } else {
            s_off = (int)(w / (uint32_t)n_valid);
            pix = L.pix_of[w - (uint32_t)s_off * (uint32_t)n_valid];
        }
        // lane p of the wave holds the image index of pixel p of the tile (my_pixel); the image row follows from the
        // tile's first row — or, with strips that cut tiles (tile_py0 < 0), from the parked tile row
        pixel_out = (uint32_t)shfl_i((int)my_pixel, pix);
        py_out = tile_py0 + (pix >> 3) * A.step_y;
        if (tile_py0 < 0) {
            const int vrow = __builtin_amdgcn_readfirstlane(L.info[(state >> 6) & 1u].ty) * 8 + (pix >> 3);
            py_out = ((vrow / A.strip_rows) * A.strip_count + A.strip_index) * A.strip_rows + vrow % A.strip_rows;
        }
        sample_out = (uint32_t)(smp0 + s_off);
    };
    // REGENERATION BATCHES.  A lane that starts a new path needs the path's camera
    // sample: the vertical jitter and ray time (one Philox block) and the lens disk (a
    // rejection loop).  Only ~16 of 64 lanes start a path in a given iteration, so doing
    // this at the hand-out runs ~120 instructions at 25 % lane use.  Entries leave the pool
    // in index order, so the wave instead draws the samples of 64 consecutive entries at
    // once — every lane busy — into LDS, two batches ahead of `next`.  (The buffers belong to the current item: an item
    // that still has paths in flight when the next one starts has handed out all its entries.)
    auto prepare_batch = [&](uint32_t b) {
        if constexpr (!PRETRACE) {
        int lane = lane_of_wave; // (opaque, like start_item's)
        asm volatile("" : "+v"(lane));
        const RT_CONSTANT TraceArgs *K = kernargs_here();
        const uint32_t w = b * 64u + (uint32_t)lane;
        const bool in_pool = w < total;
        int py_b = 0;
        uint32_t pixel_b = 0, sample_b = 0;
        int pix_b = 0;
        entry_of(w, py_b, pixel_b, sample_b, pix_b); // (entries behind the pool's end: values nobody reads)
        const u4 bc = philox4x32(pixel_b, sample_b, RT_RNG_CAMERA, 0u, A.seed_lo, A.seed_hi);
        const int buf = (int)(b & (uint32_t)(NBUF - 1));
        L.v[buf][lane] = div_by((double)py_b + u53(bc.a, bc.b), (double)(A.height - 1), K->inv_height_m1); // cpu.rs:39-40
        // camera.rs:335: the ray's time, second double of the same block (MovingSphere reads it)
        if (PRIMS == PRIMS_ANY && ray_times != nullptr) ray_times[buf][lane] = K->cam.time_a + (K->cam.time_b - K->cam.time_a) * u53(bc.c, bc.d);
        // camera.rs:327: aperture 0 multiplies the disk by 0, so its draws are dead and skipped
        if (K->cam.lens_radius != 0.0) {
            double lx = 0.0, ly = 0.0;
            coop_random_in_unit_disk(in_pool, pixel_b, sample_b, A.seed_lo, A.seed_hi, lane, L.scratch.req, lx, ly);
            lens[buf][lane][0] = lx * K->cam.lens_radius; // camera.rs:327 `lens_radius * random_in_unit_disk()`: formed here, by all
            lens[buf][lane][1] = ly * K->cam.lens_radius; // 64 lanes, not at the hand-out by the quarter of them that start a path
        }
        }
    };

    // PRIMARY SEGMENTS IN THE BATCHES (PRETRACE).  A path's first segment needs nothing a lane carries: its ray is a
    // function of the pool entry.  So the batch that draws the camera samples of 64 consecutive entries — all lanes busy,
    // rays of neighbouring pixels from one origin, so the rect tests' early outs fire — also forms their rays and runs
    // the closest-hit loop on them, with the expressions and the order of the path loop (a value never depends on where
    // it was computed).  An entry whose path ENDS on that segment (a miss, a light, or a depth limit of 0 or 1) adds its
    // contribution to the tile's sums right here and never takes a lane: on C3, whose camera looks at the box from
    // outside, that is half the paths.  The others go to a ring in LDS (PretraceLds) with the POINT of their hit, and the
    // hand-out gives lanes ring entries instead of pool entries: the camera ray is formed here and nowhere else.
    // The camera ray of pixel `pix` of the tile (camera.rs:326-337) (upper_left_corner + u * horizontal, the vector the
    // other variants keep per pixel, is formed here as the two-item variants do).
    // (TraceArgs.lens_lds is set exactly when the camera has an aperture: an integer the scalar unit can test)
    auto camera_ray = [&](int pix, double v, double lens_x, double lens_y, d3 &ro, d3 &rd) {
        if constexpr (PRETRACE) {
        const RT_CONSTANT TraceArgs *K = kernargs_here();
        ro = ld3(L.cam_origin);
        rd = (ld3(L.ulc) + L.u[pix] * ld3(K->cam.horizontal)) - v * ld3(K->cam.vertical) - ld3(K->cam.origin); // camera.rs:331
        if (kernargs_here()->lens_lds != 0) { // (lens_x, lens_y mean something only here; both rays are updated in place)
            const d3 offset = ld3(K->cam.right) * lens_x + ld3(K->cam.up) * lens_y;
            ro = ro + offset;
            rd = rd - offset;
        }
        }
    };
    // (Returns the count of the entries it queued.  The caller adds it to the level: with the level updated in here, on
    // one of the two ways out, the path loop carried a copy of it and a vector move more per iteration, C3 +0.09 ms.)
    auto pretrace_batch = [&](uint32_t b) -> uint32_t {
        if constexpr (PRETRACE) {
        int lane = lane_of_wave; // (opaque, like start_item's)
        asm volatile("" : "+v"(lane));
        const RT_CONSTANT TraceArgs *K = kernargs_here();
        const uint32_t w = b * 64u + (uint32_t)lane;
        const uint64_t in_pool = ballot(w < total);
        int py_b = 0, pix_b = 0;
        uint32_t pixel_b = 0, sample_b = 0;
        entry_of(w, py_b, pixel_b, sample_b, pix_b); // (entries behind the pool's end: values nobody reads)
        const int max_depth = K->max_depth;
        if (max_depth <= 0) { // renderer.rs:48-55: no segment at all, every path of the batch is white and ends here
            double one = 1.0;
            asm volatile("" : "+v"(one));
            if (__builtin_amdgcn_inverse_ballot_w64(in_pool)) {
                atomicAdd(&L.sum[pix_b][0], one);
                atomicAdd(&L.sum[pix_b][1], one);
                atomicAdd(&L.sum[pix_b][2], one);
            }
            if (lane == 0) L.n_started += (uint32_t)__popcll(in_pool);
            return 0u; // (nothing queues up: the level stays 0)
        }
        const u4 bc = philox4x32(pixel_b, sample_b, RT_RNG_CAMERA, 0u, A.seed_lo, A.seed_hi);
        // (the 64 slots behind the ring's entries are free — the path loop sees to that: at most RING_SLOTS - 64 entries
        // wait when a batch runs)
        const uint32_t in_ring = ring_level;
        d3 bo, bd;
        {
            const double v = div_by((double)py_b + u53(bc.a, bc.b), (double)(A.height - 1), K->inv_height_m1); // cpu.rs:39-40
            double lx, ly; // (set and read with an aperture only; the empty asm "defines" them without a move)
            asm volatile("" : "=v"(lx), "=v"(ly));
            if (kernargs_here()->lens_lds != 0) { // camera.rs:327
                lx = ly = 0.0;
                uint32_t w_here = w;
                asm volatile("" : "+v"(w_here)); // (the comparison anew: kept from above it is a bool turned back into a mask)
                coop_random_in_unit_disk(w_here < total, pixel_b, sample_b, A.seed_lo, A.seed_hi, lane, L.scratch.req, lx, ly);
                lx = lx * K->cam.lens_radius;
                ly = ly * K->cam.lens_radius;
            }
            camera_ray(pix_b, v, lx, ly, bo, bd); // (the camera sample is consumed here: a ring entry carries none of it)
        }
        // ---- the primary segment (renderer.rs:56-58)
        double best_t = __builtin_inf();
        int best = -1;
        increment_masked(n_segments, in_pool);
        // (the records no pixel of this item can see are stepped over: start_item)
        const uint32_t rect_mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.rect_mask);
        closest_hit_rects<false>(A.prims, bo, bd, rcp3(bd), best_t, best, rect_mask);
        // what the path adds to its pixel if it ends here (its throughput is 1): the background
        // (background_color.rs:27-33 / :45-48), or what it hit
        d3 C = ld3(L.bg_top);
        if (kernargs_here()->bg.kind == RT_BG_SKY) {
            const double t = 0.5 * (unit_fast(bd).y + 1.0);
            C = (1.0 - t) * C + t * ld3(kernargs_here()->bg.bottom);
        }
        const uint64_t hit = in_pool & ballot(best >= 0);
        int kind; // (set and read under `hit`)
        asm volatile("" : "=v"(kind));
        if (__builtin_amdgcn_inverse_ballot_w64(hit)) { // a light's emission, or a Lambertian's attenuation (which is all a path of depth 1 adds)
            const Material &M = lds_prims[best].mat;
            kind = M.kind;
            C = ld3(M.color);
        }
        asm volatile("" : "+v"(kind));
        // ends here: a miss, a light, or no depth left for a second segment (the scattered ray would come back white)
        const uint64_t light = hit & ballot(kind == RT_MAT_DIFFUSE_LIGHT);
        const uint64_t ends = kernargs_here()->max_depth <= 1 ? in_pool : (in_pool & ~hit) | light;
        const uint64_t lives = in_pool & ~ends;
        if (__builtin_amdgcn_inverse_ballot_w64(ends)) { // vec3.rs:38-42 Color::add into the pixel's sum
            // (the pixel's sum by a 32-bit product, one v_mad_u32_u24: written &L.sum[pix_b][k] the address is a 64-bit
            // v_mad_u64_u32 wherever the compiler has not kept L.u's address of the same pixel to add to)
            double *const sum = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(&L.sum[0][0]) + (uint32_t)pix_b * (uint32_t)sizeof(L.sum[0]));
            atomicAdd(sum + 0, C.x);
            atomicAdd(sum + 1, C.y);
            atomicAdd(sum + 2, C.z);
        }
        if (lane == 0) L.n_started += (uint32_t)__popcll(in_pool);
        // ---- the others queue up behind the ring's entries, in pool order (head < RING_SLOTS, in_ring + rank < RING_SLOTS),
        // with the point of their hit — the expression and the operands the path loop's trace block gives ray_at — and the
        // signs of the ray's direction, of which the normal takes the one on the rect's axis
        uint32_t slot = ring_head + in_ring + (uint32_t)lane_rank(lives);
        if (slot >= RING_SLOTS) slot -= RING_SLOTS;
        if (__builtin_amdgcn_inverse_ballot_w64(lives)) {
            asm volatile("; hit_point_begin" : "+v"(best_t));
            d3 p = ray_at(bo, best_t, bd);
            asm volatile("; hit_point_end" : "+v"(p.x), "+v"(p.y), "+v"(p.z));
            auto sign_of = [](double dk) { return (uint32_t)((unsigned long long)__double_as_longlong(dk) >> 63); };
            L.ring_p[0][slot] = p.x;
            L.ring_p[1][slot] = p.y;
            L.ring_p[2][slot] = p.z;
            L.ring_w[slot] = w;
            L.ring_best[slot] = (uint16_t)((uint32_t)best | sign_of(bd.x) << RING_BEST_BITS | sign_of(bd.y) << (RING_BEST_BITS + 1u) |
                                           sign_of(bd.z) << (RING_BEST_BITS + 2u));
        }
        return (uint32_t)__popcll(lives); // (the entries that ended here have left the pool)
        }
        return 0u;
    };

    // ---- path state of this lane (it outlives the items: a lane's path may belong to either slot)
    uint64_t alive_m = 0;
    int spix = 0;         // slot of the item the current path belongs to << 6 | its pixel of that item's tile (lane order)
    PathRng rng{0, 0, A.seed_lo, A.seed_hi};
    d3 o = mk(0, 0, 0), d = o, T = o;
    uint32_t seg = 0;
    double ray_time = 0.0; // ray.rs:26-28; scattered rays inherit it (e.g. lambertian.rs:35)
    // A lane whose hit needs a random_in_unit_sphere sample that the wave has not
    // found yet stays `waiting` (it keeps its hit below and skips tracing) until a
    // later iteration's sampler rounds reach its accepted candidate.
    uint64_t waiting_m = 0;
    uint32_t cand_base = 0;   // first untested candidate of the open request
    uint64_t lambert_m = 0;   // material of the open hit (else Metal)
    // the open hit: its point takes the ray origin's place (`o` is dead once the hit record exists) and its
    // attenuation goes into T at once, so neither is carried as extra state while the lane waits
    d3 hit_normal = o;
    double fuzz = 0.0;

    for (;;) {
        // ---- the items in flight (wave-uniform; out here, not in the path loop below: with this code inside it the path
        // state was copied from register to register around it in every iteration — C3 5.78 -> 6.84 vector instructions
        // per segment)
        if ((state & (HAVE | DRAINING)) == HAVE && next >= total) { // the pool is dry: what is in flight of it drains in the other slot
            state ^= HAVE | DRAINING | (OVERLAP ? CUR : 0u);
            state &= ~POOL_DRY;
            total = next = n_batches = batches_done = 0; // (no pool: the hand-out below finds nothing to do)
            batch_due = ~0u;
        }
        // (without OVERLAP there is one slot, and whatever is in flight belongs to the draining item)
        if ((state & DRAINING) != 0u && (OVERLAP ? alive_m & ballot((((uint32_t)spix ^ state) & CUR) != 0u) : alive_m) == 0) { // the last path of the draining item has ended
            finish_item(OVERLAP ? (int)((state ^ CUR) >> 6) & 1 : 0);
            state &= ~DRAINING;
        }
        if ((state & (HAVE | QUEUE_DRY)) == 0u && (FIXED_SUMS || (state & DRAINING) == 0u)) {
            state |= start_item() ? HAVE : QUEUE_DRY;
            if (OVERLAP && (state & HAVE) != 0u && total == 0u) state |= POOL_DRY; // (an item without a pixel: nothing to hand out)
        }
        if ((state & (HAVE | DRAINING)) == 0u) break; // the queue is dry and nothing is in flight
        RT_REGION(0); // item setup / end
        if (!OVERLAP) {
            // one item at a time: no path is in flight here.  Saying so — every lane's path state is set anew — ends the
            // state's live ranges at the loop's exit: across the item code above they would otherwise hold their registers
            // (the plain variants: 77 -> 80 VGPRs and 64 bytes of scratch).
            alive_m = waiting_m = lambert_m = 0;
            spix = 0;
            rng.pixel = rng.sample = 0;
            o = d = T = hit_normal = mk(0, 0, 0);
            seg = cand_base = 0;
            ray_time = fuzz = 0.0;
        }
        // ---- the path loop of the PRETRACE variant, ROTATED: hand-out, shade the pending hits, sampler, new direction,
        // trace, ends.  A lane leaves the trace block with its hit — `best`, and the hit's POINT in `o`, formed right behind
        // the closest-hit loop (ray_at); `d` still holds the incoming direction, whose sign on the rect's axis makes the
        // normal — or ended; the back edge sits between the trace block and the shading.  A lane that takes a ring entry
        // LOADS the same: the point its batch formed with the same expression, `best`, and a direction of +-1.0s with the
        // camera ray's signs.  So it is shaded with the others, gets its sample and traces its SECOND segment in the
        // iteration that hands it out: the loop traces no primary segment and forms no camera ray.  Across the sampler a
        // lane holds what it holds in the other variants (`waiting`: o = the hit's point, d = its normal).
        if constexpr (PRETRACE) {
            int best = -1; // the pending hit of a lane with a path that is not `waiting`
            for (;;) {
                // ---- camera batches: keep more than RING_SLOTS - 64 entries in the ring while the pool has any (a batch
                // needs 64 free slots, and nothing else does; the hand-out goes short only where more lanes are idle than
                // entries wait — at an item's start, and in the iteration that follows a batch most of whose entries ended)
                // ("a batch is left" and "64 slots are free" as one comparison: the last batch puts batch_below out of reach)
                while (rt_ring::batch_is_due(ring_level, batch_below)) {
                    ring_level = rt_ring::after_batch(ring_level, pretrace_batch(batches_done++));
                    batch_below = rt_ring::batch_below_of(batches_done << 6, total, RING_SLOTS);
                }
                RT_REGION(1); // batches
                // ---- hand ring entries to the lanes without a path (ballot + prefix count)
                const uint32_t in_ring = ring_level;
                if (in_ring != 0u) {
                    const uint64_t idle = ~alive_m;
                    const uint32_t r = (uint32_t)lane_rank(idle);
                    uint32_t slot = ring_head + r; // (every lane reads a slot: the pixel comes by a lane shuffle)
                    if (slot >= RING_SLOTS) slot -= RING_SLOTS;
                    const uint32_t w = L.ring_w[slot];
                    int s_off, pix_new;
                    if (n_valid == 64) {
                        pix_new = (int)(w & 63u);
                        s_off = (int)(w >> 6);
                    } else {
                        s_off = (int)(w / (uint32_t)n_valid);
                        pix_new = L.pix_of[(w - (uint32_t)s_off * (uint32_t)n_valid) & 63u];
                    }
                    const uint32_t pixel_new = (uint32_t)shfl_i((int)my_pixel, pix_new);
                    const uint64_t taking = idle & ballot(r < in_ring);
                    const uint32_t n_take = rt_ring::taken((uint32_t)__popcll(idle), in_ring);
                    ring_level = rt_ring::after_hand_out(in_ring, n_take);
                    ring_head = rt_ring::slot_at(ring_head, n_take, RING_SLOTS);
                    if (__builtin_amdgcn_inverse_ballot_w64(taking)) { // the hit the batch found: loads, and no arithmetic on doubles
                        asm volatile("; hand_out_begin");
                        spix = pix_new;
                        rng.pixel = pixel_new;
                        rng.sample = (uint32_t)(smp0 + s_off);
                        o = mk(L.ring_p[0][slot], L.ring_p[1][slot], L.ring_p[2][slot]);
                        uint32_t word = L.ring_best[slot];
                        asm volatile("" : "+v"(word)); // (a 32-bit value to shift: as a 16-bit one every shift count takes a register)
                        best = (int)(word & RING_BEST_MASK);
                        // What the shading below reads of the incoming direction is its sign on the rect's axis, so the lane
                        // gets a direction with the camera ray's three signs.  The fast flavour's against() reads the sign bit
                        // of the high word and nothing else: a shift that brings the entry's bit there is the whole
                        // component (what it leaves below the sign bit is never read as a number).  The reference flavour's
                        // set_face_normal takes a dot product with the axis: +-1.0.  The low words are whatever their
                        // registers hold (the empty asm "defines" them without a move): mantissa bits of a finite number.
                        auto signed_like = [word](uint32_t k) {
                            uint32_t lo;
                            asm volatile("" : "=v"(lo));
                            uint32_t hi = word << (31u - RING_BEST_BITS - k);
#ifdef RT_EXACT_DIV
                            hi = 0x3FF00000u | (hi & 0x80000000u);
#endif
                            return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
                        };
                        d = mk(signed_like(0u), signed_like(1u), signed_like(2u));
                        T = mk(1.0, 1.0, 1.0);
                        seg = 0;
                        asm volatile("; hand_out_end");
                    }
                    alive_m |= taking;
                }
                RT_REGION(2); // hand-out + primary ray
                // (the loop ends when nothing is in flight: the ring is then empty and every batch drawn, so the pool is dry)
                if (alive_m == 0) break;
                uint64_t ended_m = 0;
                // ---- shade the pending hits.  (The masks are ballots of per-lane data taken where the lanes are together: a
                // mask assigned inside a divergent branch would live in a VGPR pair.)
                const uint64_t hit_m = alive_m & ~waiting_m;
                int kind; // material of the hit: set and read under hit_m
                asm volatile("" : "=v"(kind));
                if (__builtin_amdgcn_inverse_ballot_w64(hit_m)) {
                    const Prim &P = lds_prims[best];
                    const Material &M = P.mat;
                    // (the hit record: its point is in `o` since the segment was traced — or the entry handed out — and the
                    // normal is formed below, from the sign of `d` on the rect's axis)
                    kind = M.kind;
                    RT_REGION(8); // hit record
                    T = T * ld3(M.color); // emission (the path ends) or attenuation: solid_color.rs:24-28
                    RT_REGION(9); // texture, step 1
                    // a light (diffuse_light.rs:25-37) ends the path, anything else is a Lambertian (lambertian.rs:26-38,
                    // direction below); what a Lambertian hit sets is dead in a path that has ended
                    cand_base = 0;
                    // the incoming direction is dead: lambertian.rs:27 starts from the normal
#ifndef RT_EXACT_DIV
                    // h.normal (set_face_normal_axis: +-1.0 against the ray on the rect's axis, +0.0 on the others), formed IN
                    // d's registers.  Its three low words are zeros, and given one zero the compiler keeps it in a register of
                    // its own across the loop and pairs it with each high word somewhere else: two v_mov_b64 per iteration to
                    // bring the pairs to d.  Three opaque zeros are three v_mov_b32 into d's own low words.
                    {
                        const int axis = P.kind == RT_PRIM_XY_RECT ? 2 : (P.kind == RT_PRIM_XZ_RECT ? 1 : 0); // (prim_hit_record's)
                        auto against = [](double dk, bool on_axis) { // on the axis +1.0 for dk < 0, -1.0 for dk > 0; else +0.0
                            uint32_t lo = 0u;
                            asm volatile("" : "+v"(lo));
                            const uint32_t hi = on_axis ? 0xBFF00000u ^ ((uint32_t)((unsigned long long)__double_as_longlong(dk) >> 32) & 0x80000000u) : 0u;
                            return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
                        };
                        // (two comparisons: a rect that is neither XY nor XZ is YZ, which the scalar unit works out of the two masks)
                        const uint64_t xy_m = ballot(axis == 2), xz_m = ballot(axis == 1);
                        d = mk(against(d.x, __builtin_amdgcn_inverse_ballot_w64(~(xy_m | xz_m))), against(d.y, __builtin_amdgcn_inverse_ballot_w64(xz_m)),
                               against(d.z, __builtin_amdgcn_inverse_ballot_w64(xy_m)));
                    }
#else
                    {
                        Hit h; // (prim_hit_record's normal of a plain rect: xy_rect.rs:43-45 and its siblings)
                        set_face_normal_axis(h, d, P.kind == RT_PRIM_XY_RECT ? 2 : (P.kind == RT_PRIM_XZ_RECT ? 1 : 0));
                        d = h.normal;
                    }
#endif
                }
                asm volatile("" : "+v"(kind));
                const uint64_t light_m = hit_m & ballot(kind == RT_MAT_DIFFUSE_LIGHT);
                ended_m |= light_m;
                waiting_m |= hit_m & ~light_m;
                RT_REGION(4); // material
                // ---- the wave evaluates the open rejection loops together (all 64 lanes arrive here)
                d3 sph = mk(0.0, 0.0, 0.0);
                const uint64_t finish_m = coop_random_in_unit_sphere<2>(waiting_m, rng.pixel, rng.sample, seg, cand_base, A.seed_lo, A.seed_hi, lane,
                                                                        L.scratch.sphere, sph);
                waiting_m &= ~finish_m;
                RT_REGION(5); // sampler
                if (__builtin_amdgcn_inverse_ballot_w64(finish_m)) { // lambertian.rs:27-33
                    const d3 dir = d + unit_fast(sph); // d holds the normal since the hit
                    // vec3.rs:127-130 near_zero keeps the normal: once in 10^23 samples, so the wave branches around it
                    const uint64_t near_zero = ballot(fabs(dir.x) < 1e-8) & ballot(fabs(dir.y) < 1e-8) & ballot(fabs(dir.z) < 1e-8);
#ifndef RT_EXACT_DIV
                    // (a rect's normal is +-1 on its axis and +0 on the others: rounding the negated unit sample to integers
                    // gives it back exactly, so d takes the new direction in place — see the other variants' loop)
                    d = dir;
                    if (near_zero != 0) {
                        asm volatile("; near_zero (keeps the compiler from turning the branch back into selects)");
                        if ((near_zero >> lane) & 1ull) {
                            const d3 u = unit_fast(sph);
                            d = mk(rint(-u.x) + 0.0, rint(-u.y) + 0.0, rint(-u.z) + 0.0);
                        }
                    }
#else
                    const d3 normal = d;
                    d = dir;
                    if (near_zero != 0) {
                        asm volatile("; near_zero (keeps the compiler from turning the branch back into selects)");
                        if ((near_zero >> lane) & 1ull) d = normal;
                    }
#endif
                }
                // renderer.rs:48-55: the recursion's next level has depth 0 -> white
                increment_masked(seg, finish_m);
                const uint64_t deep_m = finish_m & ballot((int)seg >= A.max_depth);
                ended_m |= deep_m;
                // ---- the next segment of every lane that has its new ray
                const uint64_t shooting = finish_m & ~deep_m;
                RT_LANES(__popcll(shooting), rt_ring::pool_is_dry(ring_level, batch_below)); // (what `next >= total` says)
                // (the pending hit is dead here — a lane that does not shoot is `waiting`, ended or idle, and none of those reads
                // it before it is set again — and saying so costs no instruction: set to "no hit" out here, for every lane,
                // the move was issued twice, here and again in front of the closest-hit loop)
                asm volatile("" : "=v"(best));
                if (__builtin_amdgcn_inverse_ballot_w64(shooting)) {
                    double best_t = __builtin_inf(); // closest hit, t in [0.001, inf) (renderer.rs:58): dead behind this block
                    best = -1;
                    ++n_segments;
                    closest_hit_rects<true>(A.prims, o, d, rcp3(d), best_t, best, ~0u, lds_prims);
                    // the hit's point takes the ray origin's place where the segment is traced: the shading block of the next
                    // iteration forms none, and a ring entry can hand one out.  (A lane that missed gets o + inf * d, which
                    // nothing reads: it ends below.)
                    asm volatile("; hit_point_begin" : "+v"(best_t));
                    o = ray_at(o, best_t, d);
                    asm volatile("; hit_point_end" : "+v"(o.x), "+v"(o.y), "+v"(o.z));
                    RT_REGION(3); // closest hit
                }
                const uint64_t miss_m = shooting & ballot(best < 0);
                // A BLACK BACKGROUND (TraceArgs.bg_black: solid, every component == 0.0) costs the loop nothing: a lane that
                // leaves the scene ends, and its segment is counted, but it forms no product and takes no part in the
                // additions below.  Exact: its terms would be T * (+-0.0) = +-0.0 (T is finite: a product of colours), a sum
                // starts at +0.0, and round-to-nearest never makes -0.0 of +0.0 plus anything — so a sum is never -0.0, and
                // x + (+-0.0) is x for every x a sum can hold.
                uint64_t adding_m = ended_m; // the ended lanes that have something to add
                ended_m |= miss_m;
                if (kernargs_here()->bg_black == 0) {
                    adding_m = ended_m;
                    const RT_CONSTANT TraceArgs *K = kernargs_here();
                    // (the two kinds as two lane masks, one of them empty: as the arms of a wave-uniform if / else they meet in
                    // temporaries, with copies in front of either arm and behind both)
                    const uint64_t sky_m = K->bg.kind == RT_BG_SKY ? miss_m : 0ull;
                    if (__builtin_amdgcn_inverse_ballot_w64(miss_m & ~sky_m)) { // background_color.rs:45-48
                        T.x = T.x * K->bg.top[0]; // (the colour as the scalar operand of each product: no copy of it is made)
                        T.y = T.y * K->bg.top[1];
                        T.z = T.z * K->bg.top[2];
                    }
                    if (__builtin_amdgcn_inverse_ballot_w64(sky_m)) { // background_color.rs:27-33
                        const double t = 0.5 * (unit_fast(d).y + 1.0);
                        T = T * ((1.0 - t) * ld3(K->bg.top) + t * ld3(K->bg.bottom));
                    }
                }
                if (__builtin_amdgcn_inverse_ballot_w64(adding_m)) { // vec3.rs:38-42 Color::add into the pixel's sum
                    atomicAdd(&L.sum[spix][0], T.x);
                    atomicAdd(&L.sum[spix][1], T.y);
                    atomicAdd(&L.sum[spix][2], T.z);
                }
                alive_m &= ~ended_m;
                RT_REGION(6); // scatter + accumulate
            }
            next = total; // every batch is drawn and the ring is empty: the pool's index, for the item code above
        } else
        // ---- the path loop: until the pool runs dry or the draining item's last path ends
        for (;;) {
        // ---- camera samples for the entries about to leave the pool (whole wave, see above)
        while (next >= batch_due) {
            prepare_batch(batches_done++);
            batch_due = batches_done >= n_batches ? ~0u : (batches_done < (uint32_t)NBUF ? 0u : (batches_done - (uint32_t)(NBUF - 1)) << 6);
        }
        RT_REGION(1); // batches
        // ---- hand pool entries to the lanes without a path (ballot + prefix count)
        if (next < total) {
            const uint64_t idle = ~alive_m;
            const uint32_t w = next + (uint32_t)lane_rank(idle);
            // entries whose camera samples are in LDS: all of them with two buffers, the current batch with one
            const uint32_t ready = NBUF == 2 ? total : min(total, batches_done << 6);
            next = min(next + (uint32_t)__popcll(idle), ready);
            if (OVERLAP && next >= total) state |= POOL_DRY;
            // entry_of(w) without the pixel arithmetic: lane p of the wave holds pixel p's index in the image
            // (my_pixel), so the entry's comes by a lane shuffle — which every lane has to take part in, hence
            // out here (the lanes that have a path compute an entry nobody reads)
            int s_off, pix_new;
            if (n_valid == 64) {
                pix_new = (int)(w & 63u);
                s_off = (int)(w >> 6);
            } else {
                s_off = (int)(w / (uint32_t)n_valid);
                pix_new = L.pix_of[w - (uint32_t)s_off * (uint32_t)n_valid];
            }
            const uint32_t pixel_new = (uint32_t)shfl_i((int)my_pixel, pix_new);
            const uint64_t taking = idle & ballot(w < ready);
            if (__builtin_amdgcn_inverse_ballot_w64(taking)) { // cpu.rs:39-40 + camera.rs:326-337
                spix = (int)(state & CUR) | pix_new;
                rng.pixel = pixel_new;
                rng.sample = (uint32_t)(smp0 + s_off);
                const RT_CONSTANT TraceArgs *K = kernargs_here();
                const int buf = (int)((w >> 6) & (uint32_t)(NBUF - 1)), slot = (int)(w & 63u);
                const double v = L.v[buf][slot];
                const d3 co = ld3(K->cam.origin);
                o = co;
                if (OVERLAP) d = (ld3(L.ulc) + L.u[pix_new] * ld3(K->cam.horizontal)) - v * ld3(K->cam.vertical) - co; // camera.rs:331
                else d = ld3(L.base[pix_new]) - v * ld3(K->cam.vertical) - co;
                const double lr = K->cam.lens_radius;
                if (lr != 0.0) {
                    const d3 offset = ld3(K->cam.right) * lens[buf][slot][0] + ld3(K->cam.up) * lens[buf][slot][1];
                    o = co + offset;
                    d = d - offset;
                }
                if (PRIMS == PRIMS_ANY && ray_times != nullptr) ray_time = ray_times[buf][slot];
                T = mk(1.0, 1.0, 1.0);
                seg = 0;
                ++n_started;
            }
            alive_m |= taking;
        }
        RT_REGION(2); // hand-out + primary ray
        // (one item at a time: the loop ends when the pool is dry and nothing is in flight — a scalar test on a ballot.
        // The OVERLAP variants leave at the bottom instead.)
        if (!OVERLAP && alive_m == 0) break;
        // ---- one ray_color level for every lane with a path
        // A path that ends here adds its throughput T (times what it ran into) to its pixel: T is dead
        // afterwards, so the product is formed in place.
        uint64_t ended_m = 0;
        uint64_t scattered_m = 0;  // the path got a new ray this iteration (depth check below)
        uint64_t finish_m = 0;     // Lambertian / Metal hit whose direction can be completed now
        const uint64_t tracing = alive_m & ~waiting_m;
        int noise_tex = -1;      // Noise texture this lane's hit wants (evaluated by the whole wave below)
        RT_LANES(__popcll(tracing), next >= total);
        // A scalar mask assigned inside a divergent branch meets its old value in a phi that the compiler takes for
        // divergent (a VGPR pair).  So the branches below leave per-lane DATA behind them (`best`, `kind`, `fuzz`), and the
        // masks are ballots of comparisons of that data, taken where all 64 lanes are back together.
        int max_depth = A.max_depth;
        asm volatile("" : "+s"(max_depth)); // (opaque: hoisted out of the loop the test lives in a lane mask that is spilled)
        const uint64_t shooting = max_depth <= 0 ? 0ull : tracing; // renderer.rs:48-55 with max_depth 0: the path ends
        ended_m = tracing & ~shooting;
        double best_t = __builtin_inf(); // closest hit, t in [0.001, inf) (renderer.rs:58)
        int best = -1, best_aux = 0;
        // material of the hit: set by the lanes that hit and read under their mask, so it starts as whatever its register
        // holds (an empty asm "defines" it: no move).  Opaque after the branch that sets it, or the comparison moves back
        // into the branch and comes out as a bool.
        int kind;
        asm volatile("" : "=v"(kind));
        {
            if (__builtin_amdgcn_inverse_ballot_w64(shooting)) {
                ++n_segments;
                const d3 inv_d = rcp3(d);
                const double inv_a = PRIMS == PRIMS_RECTS ? 0.0 : rcp_f64(len2(d));
                if (BVH) {
#ifdef RT_PROFILE_REGIONS
                    unsigned walk[2] = {0, 0};
                    unsigned *walk_stats = walk;
#else
                    unsigned *walk_stats = nullptr;
#endif
#ifdef RT_PROFILE_REGIONS
                    auto walk_mark = [&](int k) { RT_REGION(k); };
#else
                    const NoMark walk_mark;
#endif
                    if (lds_nodes != nullptr)
                        closest_hit_bvh<PRIMS>(A, lds_nodes, o, d, inv_d, inv_a, ray_time, 0.001, best_t, best, best_aux, walk_stats, walk_mark);
                    else
                        closest_hit_bvh<PRIMS>(A, bvh_nodes_for(A, d), o, d, inv_d, inv_a, ray_time, 0.001, best_t, best, best_aux, walk_stats, walk_mark);
#ifdef RT_PROFILE_REGIONS
                    atomicAdd(&rt_t_[37], (unsigned long long)walk[0]); // per-lane totals (LDS atomics)
                    atomicAdd(&rt_t_[38], (unsigned long long)walk[1]);
#endif
                } else {
                    auto test = [&](const Prim &P, int i) {
                        double t;
                        int aux;
                        if (prim_t<PRIMS>(P, o, d, inv_d, inv_a, ray_time, 0.001, best_t, t, aux)) {
                            best_t = t;
                            best = i;
                            best_aux = aux;
                        }
                    };
                    // two records per scalar-load wait: the table's latency is paid n/2 times, not n
                    // (C3 +2.8 %, C2 +3.8 %; three per wait run out of SGPRs and lose it again)
                    if (PRIMS != PRIMS_SPHERES) {
                        // The table is grouped (rect_end, sphere_end): one straight-line test per group, the plane a
                        // compile-time constant, instead of a scalar switch on the kind of every record.
                        auto test_plane = [&](auto axis, const Prim &P, int i) {
#ifndef RT_EXACT_DIV
                            rect_closest_update<decltype(axis)::value>(P.p[0], P.p[1], P.p[2], P.p[3], P.p[4], o, d, inv_d, 0.001, best_t, best, i);
                            return;
#endif
                            double t;
                            if (rect_t<true>(decltype(axis)::value, P.p[0], P.p[1], P.p[2], P.p[3], P.p[4], o, d, inv_d, 0.001, best_t, t)) {
                                best_t = t;
                                best = i;
                            }
                        };
                        // ONE pointer runs through the groups (they follow each other in the table): an address formed from the
                        // index — a 64-bit multiply-add, four scalar instructions — for every group's first record and every odd
                        // one out was a tenth of the rects-only variant's scalar instructions
                        const Prim *rec = A.prims;
                        int i = 0;
                        auto group = [&](auto axis, int end) {
                            for (; i + 1 < end; i += 2, rec += 2) {
                                const Prim pa = load_prim_uniform(rec, 0), pb = load_prim_uniform(rec, 1);
                                test_plane(axis, pa, i);
                                test_plane(axis, pb, i + 1);
                            }
                            if (i < end) {
                                test_plane(axis, load_prim_uniform(rec, 0), i);
                                ++i;
                                ++rec;
                            }
                        };
                        // the group bounds are re-read from the kernel arguments HERE (kernargs_here): hoisted out of the
                        // path loop their emptiness tests sit in SGPR pairs that the allocator parks in VGPR lanes, and
                        // every iteration pays a v_readlane (4.3 SIMD cycles of the saturated vector pipe) per half of them
                        const RT_CONSTANT TraceArgs *KB = kernargs_here();
                        const int end_xy = KB->rect_end[0], end_xz = KB->rect_end[1], end_yz = KB->rect_end[2];
                        group(std::integral_constant<int, 2>(), end_xy);  // XY
                        group(std::integral_constant<int, 1>(), end_xz);  // XZ
                        group(std::integral_constant<int, 0>(), end_yz);  // YZ
                        if (PRIMS == PRIMS_ANY) {
                            for (; i < A.sphere_end; ++i, ++rec) { // plain spheres: sphere.rs:39-59, no switch, no wrapper
                                double t;
                                int aux;
                                if (prim_t<PRIMS_SPHERES>(load_prim_uniform(rec, 0), o, d, inv_d, inv_a, ray_time, 0.001, best_t, t, aux)) {
                                    best_t = t;
                                    best = i;
                                    best_aux = 0;
                                }
                            }
                            for (; i < KB->box_end; ++i, ++rec) { // boxes, bare or wrapped: box.rs:82-101 as three slabs, no switch
                                double t;
                                int side;
                                if (box_t(load_prim_uniform(rec, 0), o, d, inv_d, 0.001, best_t, t, side)) {
                                    best_t = t;
                                    best = i;
                                    best_aux = side;
                                }
                            }
                            for (; i < A.n_prims; ++i, ++rec) test(load_prim_uniform(rec, 0), i); // moving spheres, wrapped rects and spheres
                        }
                    } else {
                        const Prim *rec = A.prims;
                        int i = 0;
                        for (; i + 1 < A.n_prims; i += 2, rec += 2) {
                            const Prim pa = load_prim_uniform(rec, 0), pb = load_prim_uniform(rec, 1);
                            test(pa, i);
                            test(pb, i + 1);
                        }
                        if (i < A.n_prims) test(load_prim_uniform(rec, 0), i);
                    }
                }
                RT_REGION(3); // closest hit
            }
            const uint64_t miss_m = shooting & ballot(best < 0), hit_m = shooting & ~miss_m;
            ended_m |= miss_m;
            {
                if (__builtin_amdgcn_inverse_ballot_w64(miss_m)) { // background_color.rs:27-33 / :45-48
                    const RT_CONSTANT TraceArgs *K = kernargs_here();
                    d3 bgc = ld3(K->bg.top);
                    if (K->bg.kind == RT_BG_SKY) {
                        const double t = 0.5 * (unit_fast(d).y + 1.0);
                        bgc = (1.0 - t) * bgc + t * ld3(K->bg.bottom);
                    }
                    T = T * bgc;
                }
                if (__builtin_amdgcn_inverse_ballot_w64(hit_m)) {
                    const Prim &P = BVH ? A.prims[best] : lds_prims[best];
                    const Material &M = P.mat;
                    const Hit h = prim_hit_record<PRIMS, TEXTURED, true>(P, o, d, ray_time, best_t, best_aux, M.needs_uv != 0);
                    kind = M.kind;
                    RT_REGION(8); // hit record
#ifdef RT_PROFILE_REGIONS
                    { // how many lanes of an iteration look up a Noise texture together?
                        const int n_noise = __popcll(ballot(TEXTURED && M.tex_kind == RT_TEX_NOISE));
                        if (n_noise > 0 && lane_rank(ballot(1)) == 0) {
                            rt_t_[35] += 1;
                            rt_t_[36] += (unsigned long long)n_noise;
                        }
                    }
#endif
                    // Texture::value once for every material that has one (light, Lambertian, Metal):
                    // one copy of the texture code, shared by the lanes of all three
                    // (variants without SPECULAR hold lights and Lambertians only: the host picks SPECULAR
                    // whenever a Metal or Dialectric exists)
                    if (!SPECULAR || kind != RT_MAT_DIELECTRIC) {
                        d3 tex;
                        if (!TEXTURED || M.tex_kind == RT_TEX_SOLID_COLOR) tex = ld3(M.color); // solid_color.rs:24-28
                        else tex = texture_value_deferred(A, BVH ? A.textures : lds_textures, M.texture, h.u, h.v, h.point, noise_tex, h.uv_approx,
                                                          // sphere.rs:20-27 in f64 from the outward normal (the face normal, un-flipped: exact)
                                                          [&] { return sphere_uv(h.front ? h.normal : -h.normal); });
                        // emission (the path ends) or attenuation, one copy for all three; a Noise colour arrives below
                        if (!TEXTURED || noise_tex < 0) T = T * tex;
                    }
                    RT_REGION(9); // texture, step 1
                    // With four arms, what every material does with the hit goes before the switch: a value
                    // assigned in one arm only costs every arm a copy where they meet (C2 -1.7 %; with the two
                    // arms of the other variants the same hoist costs C3 1 %).  A light ends the path, the point
                    // of a Noise light is read below; hit_normal and fuzz are Metal's, dead for the others.
                    const d3 d_in = d;
                    if (SPECULAR) {
                        o = h.point;
                        cand_base = 0;
                        hit_normal = h.normal;
                        fuzz = M.fuzz;
                    }
                    if (!SPECULAR) {
                        // a light (diffuse_light.rs:25-37) ends the path, anything else is a Lambertian (lambertian.rs:26-38,
                        // direction below); what a Lambertian hit sets is dead in a path that has ended
                        o = h.point;
                        cand_base = 0;
                        d = h.normal; // the incoming direction is dead: lambertian.rs:27 starts from the normal
                    } else if (kind == RT_MAT_DIFFUSE_LIGHT) {
                    } else if (kind == RT_MAT_LAMBERTIAN) {
                        d = h.normal;
                    } else if (kind == RT_MAT_METAL) { // metal.rs:26-43
                        const d3 ud = unit_fast(d_in);
                        d = ud - (2.0 * dot(ud, h.normal)) * h.normal; // metal.rs:30 reflect(); the fuzz term follows below
                    } else { // dialectric.rs:25-55
                        const double ratio = h.front ? M.color[0] : M.ior; // 1 / ior, divided at upload
                        const d3 ud = unit_fast(d_in);
                        const double cos_theta = fmin(dot(-ud, h.normal), 1.0);
                        const double sin_theta = sqrt_fast(1.0 - cos_theta * cos_theta);
                        bool reflect_it = ratio * sin_theta > 1.0;
                        if (!reflect_it) { // the draw happens only when refraction is possible
                            const double r0 = h.front ? M.color[1] : M.color[2]; // ((1 - ratio) / (1 + ratio))^2, at upload
                            const double m = 1.0 - cos_theta;
                            const double m2 = m * m;
                            const double refl = r0 + (1.0 - r0) * (m2 * m2 * m);
                            const u4 b = rng.block(seg, RT_RNG_DIELECTRIC, 0);
                            reflect_it = refl > u53(b.a, b.b);
                        }
                        if (reflect_it) {
                            d = ud - (2.0 * dot(ud, h.normal)) * h.normal;
                        } else { // vec3.rs:416-422
                            const d3 perp = ratio * (ud + cos_theta * h.normal);
                            d = perp + (-sqrt_fast(fabs(1.0 - len2(perp)))) * h.normal;
                        }
                    }
                }
            }
            // what the hit's material decided, from its kind: a light ends the path, a Lambertian and a Metal with fuzz
            // (fuzz 0 multiplies the sample by 0: its draws are dead) wait for a sample, glass has its new ray already
            asm volatile("" : "+v"(kind));
            const uint64_t light_m = hit_m & ballot(kind == RT_MAT_DIFFUSE_LIGHT);
            ended_m |= light_m;
            if (!SPECULAR) {
                waiting_m |= hit_m & ~light_m;
            } else {
                const uint64_t lambertian = hit_m & ballot(kind == RT_MAT_LAMBERTIAN), metal = hit_m & ballot(kind == RT_MAT_METAL);
                const uint64_t fuzzy = metal & ballot(fuzz != 0.0);
                lambert_m = (lambert_m & ~metal) | lambertian;
                waiting_m |= lambertian | fuzzy;
                finish_m = metal & ~fuzzy;
                scattered_m = hit_m & ~(light_m | lambertian | metal);
            }
        }

        // ---- the wave evaluates the open rejection loops together (all 64 lanes arrive
        // here).  A request still open afterwards resumes next iteration, which costs its lane
        // one idle pass.  On cornell-like scenes (many requests, cheap iterations) two rounds
        // settle ~90 % and a third costs more than the idle lanes it saves; where an iteration
        // is expensive (textures, glass) or requests are few, up to four rounds pay: the loop
        // stops as soon as nothing is pending (measured: C2 +1.4 %, C4 +2.7 %, C3 -9 % with 3).
        RT_REGION(4); // miss / material
        if constexpr (TEXTURED) { // the Noise lookups of this iteration, by the whole wave (all 64 lanes arrive here)
            const bool lookup = noise_tex >= 0;
            if (ballot(noise_tex >= 0) != 0) {
                const Texture *tt = BVH ? A.textures : lds_textures;
                const double turb = coop_noise_turbulence(lookup, o, lookup ? tt[noise_tex].depth : 0,
                                                          lookup ? tt[noise_tex].perlin : 0, A, lds_perlin, lane, L.scratch.noise);
                if (lookup) {
                    const d3 tex = noise_colour(tt[noise_tex], o, turb);
                    T = T * tex; // DiffuseLight's emission (the path has ended) or Lambertian / Metal attenuation
                }
            }
        }
        RT_REGION(10); // Noise rounds
        d3 sph = mk(0.0, 0.0, 0.0); // (left uninitialised, three moves fewer per iteration cost the plain variants 16 bytes of scratch)
        {
            const uint64_t got = coop_random_in_unit_sphere<(TEXTURED || SPECULAR) ? 4 : 2>(waiting_m, rng.pixel, rng.sample, seg, cand_base, A.seed_lo,
                                                                                           A.seed_hi, lane, L.scratch.sphere, sph);
            waiting_m &= ~got;
            finish_m |= got;
        }

        RT_REGION(5); // sampler
        double facing = 0.0; // Metal: the new direction against the normal
        if (__builtin_amdgcn_inverse_ballot_w64(finish_m)) {
            if (!SPECULAR || __builtin_amdgcn_inverse_ballot_w64(lambert_m)) { // lambertian.rs:27-33 (without SPECULAR every open hit is a Lambertian one)
                const d3 dir = d + unit_fast(sph); // d holds the normal since the hit
                // vec3.rs:127-130 near_zero keeps the normal: once in 10^23 samples, so the wave branches
                // around the six selects it would otherwise issue every time.  (The ballots of the three comparisons,
                // ANDed as scalars: no short-circuit branch, no lane mask turned into an integer and back.)
                const uint64_t near_zero = ballot(fabs(dir.x) < 1e-8) & ballot(fabs(dir.y) < 1e-8) & ballot(fabs(dir.z) < 1e-8);
#ifndef RT_EXACT_DIV
                if (PRIMS == PRIMS_RECTS) {
                    // A rect's normal is +-1 on its axis and +0 on the others (set_face_normal_axis), and a near-zero
                    // direction means the unit sample is within 1e-8 of its opposite: rounding the negated sample to
                    // integers gives the normal back exactly (+ 0.0 turns -0 into +0).  So d takes the new direction
                    // in place, and the normal is not kept beside it (three v_mov_b64 per iteration at the join).
                    d = dir;
                    if (near_zero != 0) {
                        asm volatile("; near_zero (keeps the compiler from turning the branch back into selects)");
                        if ((near_zero >> lane) & 1ull) {
                            const d3 u = unit_fast(sph);
                            d = mk(rint(-u.x) + 0.0, rint(-u.y) + 0.0, rint(-u.z) + 0.0);
                        }
                    }
                } else
#endif
                {
                    const d3 normal = d;
                    d = dir;
                    if (near_zero != 0) {
                        asm volatile("; near_zero (keeps the compiler from turning the branch back into selects)");
                        if ((near_zero >> lane) & 1ull) d = normal;
                    }
                }
            } else if (SPECULAR) { // metal.rs:31-42: d holds the reflected direction since the hit
                if (fuzz != 0.0) d = d + fuzz * sph;
                facing = dot(d, hit_normal);
                if (facing < 0.0) T = mk(0.0, 0.0, 0.0);
            }
        }
        if (!SPECULAR) {
            scattered_m = finish_m;
        } else {
            const uint64_t absorbed = finish_m & ~lambert_m & ballot(facing < 0.0);
            ended_m |= absorbed;
            scattered_m |= finish_m & ~absorbed;
        }
        // renderer.rs:48-55: the recursion's next level has depth 0 -> white
        increment_masked(seg, scattered_m);
        ended_m |= scattered_m & ballot((int)seg >= A.max_depth);
        ended_m &= alive_m;
        if (__builtin_amdgcn_inverse_ballot_w64(ended_m)) { // vec3.rs:38-42 Color::add into the pixel's sum
            // (the scale is a power of two: its upper half lives in ONE scalar register across the loop — a scalar load and its
            // wait here, in every iteration, showed in the frame time)
            if (FIXED_SUMS) {
                const uint32_t scale_hi = sum_scale_hi;
                // T * scale + 2^52 (one fma: the product is exact, the sum rounds T to a multiple of 1 / scale) has the
                // integer in its mantissa; integer adds commute exactly (start_item has taken the exponent fields off)
                const double scale = __longlong_as_double((long long)((unsigned long long)scale_hi << 32));
                unsigned long long *sum = reinterpret_cast<unsigned long long *>(L.sum[spix]);
                atomicAdd(sum + 0, (unsigned long long)__double_as_longlong(fma(T.x, scale, 0x1p52)));
                atomicAdd(sum + 1, (unsigned long long)__double_as_longlong(fma(T.y, scale, 0x1p52)));
                atomicAdd(sum + 2, (unsigned long long)__double_as_longlong(fma(T.z, scale, 0x1p52)));
            } else {
                atomicAdd(&L.sum[spix][0], T.x);
                atomicAdd(&L.sum[spix][1], T.y);
                atomicAdd(&L.sum[spix][2], T.z);
            }
        }
        alive_m &= ~ended_m;
        RT_REGION(6); // scatter + accumulate
        // ---- ONE way out of the path loop, down here (a second `break`, or one inside an else-arm of the hand-out, had the
        // compiler merge the lanes' alive / waiting / material masks under the exec mask at two more joins: +20 scalar
        // instructions per iteration on a kernel whose scalar unit is busy 70 % of the time): an item event is due — the pool
        // has run dry and the other slot is free to take what is in flight of it, or the draining item's last path has ended.
        // ("Nothing in flight" is one of the two: a pool that is not dry feeds the lanes in the next iteration.)
        if (OVERLAP) {
            uint32_t st = state;
            asm volatile("" : "+s"(st)); // (opaque: `state` does not change in this loop)
            if ((st & (DRAINING | POOL_DRY)) != 0u) { // (one scalar test in the usual iteration)
                uint64_t go = 0ull; // (a scalar 64-bit value, not a bool: see the flags above)
                if ((st & DRAINING) != 0u) go = alive_m & ballot((((uint32_t)spix ^ st) & CUR) != 0u);
                if (go == 0ull) break;
            }
        }
        }
    }
    RT_REGION(7); // item end
    RT_REGION_FLUSH
    unsigned long long total_segments = n_segments; // one atomic per wave for the statistic
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total_segments += __shfl_down(total_segments, off, 64);
    if (lane == 0 && total_segments) atomicAdd(A.segments + RT_STAT_SEGMENTS, total_segments);
    if constexpr (PRETRACE) {
        int first = lane_of_wave;
        asm volatile("" : "+v"(first));
        n_started = first == 0 ? L.n_started : 0u;
    }
    unsigned long long started = n_started; // primary rays (RtRenderStats.samples)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) started += __shfl_down(started, off, 64);
    if (lane == 0 && started) atomicAdd(A.segments + RT_STAT_SAMPLES, started);
}

} // namespace RT_KNS

#if defined(RT_BB_COUNT) && !defined(RT_EXACT_DIV)
// -DRT_BB_COUNT (tools/bb_build.sh, never the product): the basic-block counters that tools/bb_instrument.py's inserted
// instructions add to, and the host call that reads them.  Nothing in the C++ below touches the array on the device.
enum { RT_BB_MAX = 8192 };
extern "C" {
__device__ __attribute__((used)) unsigned long long rt_bb_counts[RT_BB_MAX];
int rtdev_bb_counts(unsigned long long *out, int n, int reset) {
    if (n > RT_BB_MAX) n = RT_BB_MAX;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(rt_bb_counts), (size_t)n * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long zeros[RT_BB_MAX];
        if (hipMemcpyToSymbol(HIP_SYMBOL(rt_bb_counts), zeros, sizeof zeros) != hipSuccess) return -1;
    }
    return n;
}
}
#endif

namespace {
// One table entry per compiled variant: PRIMS x TEXTURED x SPECULAR with the
// linear closest-hit loop, plus PRIMS_ANY x TEXTURED x SPECULAR with the BVH.
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH> struct PoolVariant {
    static void launch(const rtdev::TraceArgs &a, const rtdev::PrimaryRects &r, unsigned blocks, hipStream_t stream) {
        const size_t dyn = rtdev::pool_lds_layout(BVH, TEXTURED, a.n_prims, a.n_textures, a.bvh_lds_nodes, a.perlin_in_lds, a.lens_lds,
                                                  a.time_lds).bytes;
        hipLaunchKernelGGL((RT_KNS::k_trace_pool_f64<PRIMS, TEXTURED, SPECULAR, BVH>), dim3(blocks), dim3(256), dyn, stream, a, r);
    }
    static int blocks_per_cu(size_t dyn_lds) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, RT_KNS::k_trace_pool_f64<PRIMS, TEXTURED, SPECULAR, BVH>, 256, dyn_lds) != hipSuccess)
            return 1;
        // The calculator divides the CU's 160 KB by the block's LDS bytes; the hardware hands LDS out in granules of 1280
        // bytes, 128 to a CU (tools/microbench/lds_fit.hip: 23 168 bytes per block already leave 6 blocks where the
        // calculator says 7).  A persistent grid one block per CU too large runs that block when the others are done.
        hipFuncAttributes attr;
        if (hipFuncGetAttributes(&attr, (const void *)RT_KNS::k_trace_pool_f64<PRIMS, TEXTURED, SPECULAR, BVH>) == hipSuccess) {
            const size_t granules = (attr.sharedSizeBytes + dyn_lds + 1279) / 1280;
            if (granules > 0 && (int)(128 / granules) < n) n = (int)(128 / granules);
        }
        return n < 0 ? 0 : n; // 0: a block does not fit a CU (rt_api.hip: enqueue_render refuses the launch)
    }
    static int static_lds() {
        hipFuncAttributes attr;
        if (hipFuncGetAttributes(&attr, (const void *)RT_KNS::k_trace_pool_f64<PRIMS, TEXTURED, SPECULAR, BVH>) != hipSuccess) return -1;
        return (int)attr.sharedSizeBytes;
    }
};
} // namespace

// Resident blocks per CU of the variant (the persistent grid is CUs x this).
extern "C" int RT_LAUNCHER(rtdev_pool_blocks_per_cu)(int prims_class, int textured, int specular, int bvh, size_t dyn_lds) {
    return rtdev::dispatch_variant<PoolVariant>(prims_class, textured != 0, specular != 0, bvh != 0,
                                                [dyn_lds](auto v) { return decltype(v)::blocks_per_cu(dyn_lds); });
}

// Static LDS of the variant's kernel (its WaveLds), -1 when the runtime cannot say.
extern "C" int RT_LAUNCHER(rtdev_pool_static_lds)(int prims_class, int textured, int specular, int bvh) {
    return rtdev::dispatch_variant<PoolVariant>(prims_class, textured != 0, specular != 0, bvh != 0,
                                                [](auto v) { return decltype(v)::static_lds(); });
}

extern "C" hipError_t RT_LAUNCHER(rtdev_launch_trace_pool)(const rtdev::TraceArgs *args, const rtdev::PrimaryRects *rects, int prims_class,
                                              int textured, int specular, int bvh, unsigned blocks, hipStream_t stream) {
    if (blocks == 0 || args->n_items == 0) return hipSuccess;
    rtdev::dispatch_variant<PoolVariant>(prims_class, textured != 0, specular != 0, bvh != 0, [&](auto v) {
        decltype(v)::launch(*args, *rects, blocks, stream);
    });
    return hipGetLastError();
}
