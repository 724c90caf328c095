// rt_nee_stream_kernel.hip — the next-event estimator as a tile stream, behind rt_render_nee:
// k_nee_stream_f64 is a persistent grid whose waves draw 8x8 tiles from a region-ordered queue, trace ALL samples of a
// tile with rt_nee_common.h's nee_samples — the loop k_nee_f64 runs, a pixel's samples added in sample order to an f64 sum
// that starts at +0.0 — and write the tile's finished pixels, sqrt((1 / samples) * sum), straight into the caller's pinned
// tile-column frame.  The wave that finishes a region's last tile publishes the region to the host.  A pixel is therefore
// rt_render_frame_nee's pixel, bit for bit, whatever the tile grid, the grid size or the order the waves run in — and whatever
// share of the frame's rows the launch owns (TraceArgs.strip_*: rt_render_frame_nee_multi / rt_render_nee_multi):
// the tiles are those of the launch's owned-row grid, and a lane's row is mapped to its image row before anything is drawn.
#include "rt_nee_stream.h"
#include "rt_variant_dispatch.h"

namespace RT_KNS {

// 256 threads = 4 waves, each on its own: a wave draws a tile (lane 0: one atomicAdd on TraceArgs.queue), lane = pixel,
// and keeps the tile until its `samples` samples are added, kNeeStreamChunk at a time.  Lane 0 reads the host's cancel
// word (TraceArgs.cancel_flag, pinned host memory; NULL: the call has no hook) before every hand-out and before every
// chunk while the word is down; a wave that sees it up idles through the rest of its tile's chunks without asking again
// (no early exit: those cost registers and a stack frame), publishes nothing of the tile and takes no
// more work.  The word only ever goes up while
// a launch runs.  The host ends the launch the way it ends the pooled kernel's: the word, and the item counter poisoned
// with 2^31.  What a tile needs of the arguments is re-read through kernargs_here() per tile, so that nothing of the
// tile's prologue is hoisted in front of the loops and kept in registers across the path loop.
// PRIMS / TEXTURED / SPECULAR / BVH as k_nee_f64; TraceArgs comes FIRST (closest_hit_bvh reads the kernarg segment).
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
__global__ __launch_bounds__(256, (kStreamWaves<PRIMS, TEXTURED, SPECULAR, BVH>)) void k_nee_stream_f64(const TraceArgs A, const NeeArgs N) {
    nee_stream<PRIMS, TEXTURED, SPECULAR, BVH, PlainLights>(A, N, NoLightArgs());
}

} // namespace RT_KNS

namespace {
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH> struct StreamVariant {
    static void launch(const rtdev::TraceArgs &a, const rtdev::NeeArgs &n, unsigned blocks, hipStream_t stream) {
        hipLaunchKernelGGL((RT_KNS::k_nee_stream_f64<PRIMS, TEXTURED, SPECULAR, BVH>), dim3(blocks), dim3(256), 0, stream, a, n);
    }
    // Resident blocks per CU, as the pooled kernel's grid is sized (rt_trace_pool_kernel.hip: blocks_per_cu; no LDS here).
    // At most 8 blocks of 256 threads are admitted whatever the calculator says.
    static int blocks_per_cu() {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, RT_KNS::k_nee_stream_f64<PRIMS, TEXTURED, SPECULAR, BVH>, 256, 0) != hipSuccess)
            return 1;
        return n < 1 ? 1 : (n > 8 ? 8 : n);
    }
};
} // namespace

// Resident blocks per CU of the variant (the persistent grid is CUs x this).
extern "C" int RT_LAUNCHER(rtdev_nee_stream_blocks_per_cu)(int prims_class, int textured, int specular, int bvh) {
    return rtdev::dispatch_variant<StreamVariant>(prims_class, textured != 0, specular != 0, bvh != 0,
                                                  [](auto v) { return decltype(v)::blocks_per_cu(); });
}

// The chunk length this flavour was compiled with (the tests size their sample counts by it).
extern "C" int RT_LAUNCHER(rtdev_nee_stream_chunk)(void) { return RT_KNS::kNeeStreamChunk; }

// args->n_items tiles of args->regions, every sample of each, delivered into args->deliver_out by `blocks` blocks (at most
// the resident ones).  prims_class: rtdev::PRIMS_*; bvh: closest hits through args' tree (then PRIMS_ANY).
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_nee_stream)(const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee, int prims_class,
                                                           int textured, int specular, int bvh, unsigned blocks, hipStream_t stream) {
    if (blocks == 0 || args->n_items == 0 || args->samples <= 0) return hipSuccess;
    rtdev::dispatch_variant<StreamVariant>(prims_class, textured != 0, specular != 0, bvh != 0, [&](auto v) {
        decltype(v)::launch(*args, *nee, blocks, stream);
    });
    return hipGetLastError();
}
