// rt_nee_pass_kernel.hip — the next-event estimator in passes, behind rt_render_progressive_nee and
// rt_render_adaptive_nee: k_nee_pass_f64 traces the samples of one pass for a list of 8x8 tiles on top of the running
// per-pixel sums, k_nee_decide_f64 then writes the pass's frame, measures every running tile and stops it or lists it for
// the next pass.  The estimator itself is rt_nee_common.h's nee_samples, the loop k_nee_f64 runs: a pixel's samples are
// added in sample order to a sum that travels from launch to launch in TraceArgs.accum, so after any pass the sums are
// the ones k_nee_f64 forms with that many samples, bit for bit.
#include "rt_nee_pass.h"
#include "rt_tile_decide.h"
#include "rt_variant_dispatch.h"

namespace RT_KNS {

// 256 threads = 4 waves; wave w of block b traces item 4 b + w: tile tile_list[item] of the 8x8 tile grid (tiles_x wide),
// or tile `item` itself without a list; lane = pixel.  A launch traces ONE chunk of the frame's chunk plan, samples
// [sample_begin, sample_end); the host launches a pass's chunks one behind the other (rt_nee.hip: enqueue_nee_pass).
// That keeps the kernel k_nee_f64 with a prologue and an epilogue — same path loop, entered once, nothing more alive in
// it — where a loop over the pass's chunks around the path loop cost every variant 4 to 9 VGPRs and six of them their
// occupancy step.
//
// BATCH MEANS.  The error of rt_render_adaptive_nee needs Q = sum_j S_j^2 / n_j over the chunks, S_j being what chunk j
// added to the pixel.  The trace kernel knows nothing of it: k_nee_chunk_f64 runs behind every chunk's launch, takes S_j as
// the difference of the running sum and its copy from the last boundary and adds S_j^2 / n_j to Q.  (Updating Q in the
// trace kernel's epilogue left ten of its variants with a stack frame; elementwise over the frame it costs 0.1 ms.)
//
// CANCEL.  The host's cancel word (TraceArgs.cancel_flag, pinned host memory) is read by lane 0 of every wave when it
// starts, i.e. at every chunk boundary of a pass; when it is up the wave leaves at once.  What a cancelled pass leaves in
// accum / squares is not read again: the host delivers nothing of it and the next call starts its sums afresh.
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
__global__ __launch_bounds__(256) void k_nee_pass_f64(const TraceArgs A, const NeeArgs N) {
    nee_pass<PRIMS, TEXTURED, SPECULAR, BVH, PlainLights>(A, N, NoLightArgs());
}

// Behind every chunk: per pixel and channel S_j = running - boundary, squares += S_j^2 / n_j, boundary = running.  A
// stopped tile's sums no longer move: S_j = 0 there, so the whole frame is swept.
__global__ __launch_bounds__(256) void k_nee_chunk_f64(const double *__restrict__ running, double *__restrict__ boundary,
                                                       double *__restrict__ squares, size_t n, double inv_samples) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double now = running[i], s = now - boundary[i];
        squares[i] += s * s * inv_samples;
        boundary[i] = now;
    }
}

// The decision step of a pass (rtdev::NeeDecide), a kernel of its own behind k_nee_pass_f64: rt_tile_decide.h's step with
// nothing to fold — k_fold_adaptive_f64 (rt_frame_kernels.hip) without the fold, the sums and Q being where the trace
// kernel and k_nee_chunk_f64 left them.  Every tile writes its pixels into the pass's frame slot; a running tile is
// measured and stops or is appended to the next pass's list.  next_list NULL (rt_render_progressive_nee): nothing stops,
// nothing is listed.
__global__ __launch_bounds__(1024) void k_nee_decide_f64(const NeeDecide F) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = (int)blockIdx.x * 16 + wave; // wave-uniform
    uint32_t keep = 0; // (lane 0) this wave's tile runs on
    if (t < F.d.n_tiles) keep = decide_tile(F.d, t, lane, [](size_t, double (&)[3], double (&)[3]) {});
    if (F.d.next_list == nullptr) return; // (uniform over the grid)
    append_running_tiles(F.d, t, lane, wave, keep);
}

} // namespace RT_KNS

namespace {
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH> struct PassVariant {
    static void launch(const rtdev::TraceArgs &a, const rtdev::NeeArgs &n, unsigned blocks, hipStream_t stream) {
        hipLaunchKernelGGL((RT_KNS::k_nee_pass_f64<PRIMS, TEXTURED, SPECULAR, BVH>), dim3(blocks), dim3(256), 0, stream, a, n);
    }
};
} // namespace

// Samples [sample_begin, sample_end), one chunk, of args->n_items tiles (args->tile_list, or every tile of the grid in order)
// added to args->accum.  prims_class: rtdev::PRIMS_*; bvh: closest hits through args'
// tree (then PRIMS_ANY).
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_nee_pass)(const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee,
                                                         int prims_class, int textured, int specular, int bvh,
                                                         hipStream_t stream) {
    if (args->n_items == 0 || args->sample_end <= args->sample_begin) return hipSuccess;
    const unsigned blocks = (args->n_items + 3u) / 4u;
    rtdev::dispatch_variant<PassVariant>(prims_class, textured != 0, specular != 0, bvh != 0, [&](auto v) {
        decltype(v)::launch(*args, *nee, blocks, stream);
    });
    return hipGetLastError();
}

// n = W*H*3 elements; samples: those of the chunk just traced
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_nee_chunk)(const double *running, double *boundary, double *squares, size_t n,
                                                          int samples, hipStream_t stream) {
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (blocks > 4096u) blocks = 4096u;
    if (blocks == 0 || samples <= 0) return hipSuccess;
    hipLaunchKernelGGL(RT_KNS::k_nee_chunk_f64, dim3(blocks), dim3(256), 0, stream, running, boundary, squares, n, 1.0 / (double)samples);
    return hipGetLastError();
}

extern "C" hipError_t RT_LAUNCHER(rtdev_launch_nee_decide)(const rtdev::NeeDecide *f, hipStream_t stream) {
    if (f->d.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(RT_KNS::k_nee_decide_f64, dim3((unsigned)(f->d.n_tiles + 15) / 16), dim3(1024), 0, stream, *f);
    return hipGetLastError();
}
