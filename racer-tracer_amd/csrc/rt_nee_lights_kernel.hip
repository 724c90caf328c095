// rt_nee_lights_kernel.hip — k_nee_f64 (rt_nee_kernel.hip) with the light code of rt_scene_set_lights' list (rt_nee_lights.h):
// wrapped, box and moving lights, a pick by power.  The same body (rt_nee_frame.h), the same launch; the pick's arrays
// travel in an argument block of their own behind NeeArgs.  PRIMS_ANY only: linear and BVH x TEXTURED x SPECULAR, in both
// arithmetic flavours.
#include "rt_nee_frame.h"
#include "rt_nee_lights.h"
#include "rt_variant_dispatch.h"

namespace RT_KNS {

// TraceArgs comes FIRST, as everywhere: closest_hit_bvh reads the root box through the kernarg segment.
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
__global__ __launch_bounds__(256) void k_nee_lights_f64(const TraceArgs A, const NeeArgs N, const NeeLightArgs X) {
    nee_frame<PRIMS, TEXTURED, SPECULAR, BVH, ExtendedLights>(A, N, X);
}

} // namespace RT_KNS

namespace {
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH> struct NeeLightsVariant {
    static void launch(const rtdev::TraceArgs &a, const rtdev::NeeArgs &n, const rtdev::NeeLightArgs &x, unsigned blocks, hipStream_t stream) {
        hipLaunchKernelGGL((RT_KNS::k_nee_lights_f64<PRIMS, TEXTURED, SPECULAR, BVH>), dim3(blocks), dim3(256), 0, stream, a, n, x);
    }
};
} // namespace

// rtdev_launch_nee's launch with the extended light code; bvh: closest hits through args' tree, else the linear loop over
// every kind.
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_nee_lights)(const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee,
                                                           const rtdev::NeeLightArgs *lights, int textured, int specular, int bvh,
                                                           hipStream_t stream) {
    const unsigned blocks = rtdev::frame_blocks(*args);
    if (blocks == 0) return hipSuccess;
    rtdev::dispatch_any_variant<NeeLightsVariant>(textured != 0, specular != 0, bvh != 0, [&](auto v) {
        decltype(v)::launch(*args, *nee, *lights, blocks, stream);
    });
    return hipGetLastError();
}
