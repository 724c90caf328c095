// rt_nee_lights_pass_kernel.hip — k_nee_pass_f64 (rt_nee_pass_kernel.hip) with the light code of rt_scene_set_lights' list
// (rt_nee_lights.h), behind rt_render_progressive_nee and rt_render_adaptive_nee on a scene that carries such a list.  The
// same body (rt_nee_pass.h); k_nee_chunk_f64 and k_nee_decide_f64 run behind it unchanged.  PRIMS_ANY only.
#include "rt_nee_pass.h"
#include "rt_nee_lights.h"
#include "rt_variant_dispatch.h"

namespace RT_KNS {

template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
__global__ __launch_bounds__(256) void k_nee_lights_pass_f64(const TraceArgs A, const NeeArgs N, const NeeLightArgs X) {
    nee_pass<PRIMS, TEXTURED, SPECULAR, BVH, ExtendedLights>(A, N, X);
}

} // namespace RT_KNS

namespace {
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH> struct LightsPassVariant {
    static void launch(const rtdev::TraceArgs &a, const rtdev::NeeArgs &n, const rtdev::NeeLightArgs &x, unsigned blocks, hipStream_t stream) {
        hipLaunchKernelGGL((RT_KNS::k_nee_lights_pass_f64<PRIMS, TEXTURED, SPECULAR, BVH>), dim3(blocks), dim3(256), 0, stream, a, n, x);
    }
};
} // namespace

// rtdev_launch_nee_pass's launch with the extended light code.
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_nee_lights_pass)(const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee,
                                                                const rtdev::NeeLightArgs *lights, int textured, int specular,
                                                                int bvh, hipStream_t stream) {
    if (args->n_items == 0 || args->sample_end <= args->sample_begin) return hipSuccess;
    const unsigned blocks = (args->n_items + 3u) / 4u;
    rtdev::dispatch_any_variant<LightsPassVariant>(textured != 0, specular != 0, bvh != 0, [&](auto v) {
        decltype(v)::launch(*args, *nee, *lights, blocks, stream);
    });
    return hipGetLastError();
}
