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
#include "rt_nee_frame.h"
#include "rt_variant_dispatch.h"

namespace RT_KNS {

// 256 threads = 4 waves; each wave owns an 8x8 pixel tile, each block a 16x16 one (k_trace_f64's layout, whole frames).
// PRIMS / TEXTURED / SPECULAR as k_trace_f64; BVH: closest hits through the scene's tree in global memory (PRIMS_ANY).
// TraceArgs comes FIRST: closest_hit_bvh reads the root box through the kernarg segment (rt_trace_common.h).
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
__global__ __launch_bounds__(256) void k_nee_f64(const TraceArgs A, const NeeArgs N) {
    nee_frame<PRIMS, TEXTURED, SPECULAR, BVH, PlainLights>(A, N, NoLightArgs());
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
    const unsigned blocks = rtdev::frame_blocks(*args);
    if (blocks == 0) return hipSuccess;
    rtdev::dispatch_variant<NeeVariant>(prims_class, textured != 0, specular != 0, bvh != 0, [&](auto v) {
        decltype(v)::launch(*args, *nee, blocks, stream);
    });
    return hipGetLastError();
}
