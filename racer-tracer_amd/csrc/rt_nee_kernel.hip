// rt_nee_kernel.hip — the next-event-estimation path kernel (f64) behind rt_render_frame_nee: the plain
// estimator of rt_trace_kernel.hip with one light sample per Lambertian vertex, both terms weighted by multiple
// importance sampling.  Every draw of the plain estimator stays at its address (include/rt_rng.h), so the BSDF path of a
// sample is the very path the plain kernels trace; the light sample draws from its own purpose, RT_RNG_LIGHT.
//
// One lane owns one pixel, as in the v1 kernel, and adds its samples' radiance in sample order: the frame does not
// depend on scheduling or tiling.  A lane's pending ray is a path segment or a shadow ray, and the loop has ONE
// closest-hit site: a Lambertian vertex that takes a light sample first traces the shadow ray, folds its answer in,
// and then continues with the bounce ray it drew.  (Two trace calls per iteration would leave every lane that has no
// shadow ray idle through the second one.)
#include "rt_nee_common.h"
#include "rt_variant_dispatch.h"

namespace RT_KNS {

// 256 threads = 4 waves; each wave owns an 8x8 pixel tile, each block a 16x16 one (k_trace_f64's layout, whole frames).
// PRIMS / TEXTURED / SPECULAR as k_trace_f64; BVH: closest hits through the scene's tree in global memory (PRIMS_ANY).
// TraceArgs comes FIRST: closest_hit_bvh reads the root box through the kernarg segment (rt_trace_common.h).
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
__global__ __launch_bounds__(256) void k_nee_f64(const TraceArgs A, const NeeArgs N) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tiles_x = (A.width + 15) >> 4;
    const int bx = blockIdx.x % tiles_x;
    const int by = blockIdx.x / tiles_x;
    const int px = bx * 16 + (wave & 1) * 8 + (lane & 7);
    const int vrow = by * 16 + (wave >> 1) * 8 + (lane >> 3); // a row of the launch's owned-row grid
    int py = vrow;
    { // owned row -> image row, once: the draws and the sums below are the IMAGE pixel's.  The strip fields are read through
      // kernargs_here(), next to their one use, so that a launch without strips keeps no register for them.
        const RT_CONSTANT TraceArgs *K = kernargs_here();
        if (K->strip_count > 1)
            py = ((vrow / K->strip_rows) * K->strip_count + K->strip_index) * K->strip_rows + vrow % K->strip_rows;
    }
    // (an owned row at or beyond owned_rows lies in a strip that starts below the image: its image row is >= height)
    const bool in_image = px < A.width && py < A.height;

    PathRng rng;
    rng.pixel = (uint32_t)py * (uint32_t)A.width + (uint32_t)px;
    rng.k0 = A.seed_lo;
    rng.k1 = A.seed_hi;

    // cpu.rs:35-36: one horizontal jitter per pixel
    rng.sample = RT_RNG_SAMPLE_PIXEL;
    const u4 bj = rng.block(0, RT_RNG_PIXEL, 0);
    const double u = ((double)px + u53(bj.a, bj.b)) / (double)(A.width - 1);

    d3 sum = mk(0.0, 0.0, 0.0); // the pixel's sum
    unsigned int n_segments = 0, n_started = 0;
    nee_samples<PRIMS, TEXTURED, SPECULAR, BVH>(A, N, rng, px, py, u, in_image ? A.sample_begin : A.sample_end, A.sample_end, sum,
                                                n_segments, n_started);

    if (in_image) {
        double *px_out = A.accum + 3 * (size_t)rng.pixel;
        px_out[0] = sum.x;
        px_out[1] = sum.y;
        px_out[2] = sum.z;
    }
    // one atomic per wave for each statistic: path segments (shadow rays excluded) and primary rays
    unsigned long long total = n_segments;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
    if (lane == 0 && total) atomicAdd(A.segments + RT_STAT_SEGMENTS, total);
    unsigned long long started = n_started;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) started += __shfl_down(started, off, 64);
    if (lane == 0 && started) atomicAdd(A.segments + RT_STAT_SAMPLES, started);
}

} // namespace RT_KNS

namespace {
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH> struct NeeVariant {
    static void launch(const rtdev::TraceArgs &a, const rtdev::NeeArgs &n, unsigned blocks, hipStream_t stream) {
        hipLaunchKernelGGL((RT_KNS::k_nee_f64<PRIMS, TEXTURED, SPECULAR, BVH>), dim3(blocks), dim3(256), 0, stream, a, n);
    }
};
} // namespace

// The samples [sample_begin, sample_end) of the launch's owned rows (args->strip_*; the whole frame without strips) into
// args->accum, a full-frame buffer (written, not added to; rows not owned are left alone).  prims_class: rtdev::PRIMS_*;
// bvh: closest hits through args' tree (then PRIMS_ANY).
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_nee)(const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee, int prims_class,
                                                    int textured, int specular, int bvh, hipStream_t stream) {
    const int tiles_x = (args->width + 15) / 16;
    const int tiles_y = (args->owned_rows + 15) / 16; // the grid covers width x owned_rows
    if (tiles_x <= 0 || tiles_y <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(tiles_x * tiles_y);
    rtdev::dispatch_variant<NeeVariant>(prims_class, textured != 0, specular != 0, bvh != 0, [&](auto v) {
        decltype(v)::launch(*args, *nee, blocks, stream);
    });
    return hipGetLastError();
}
