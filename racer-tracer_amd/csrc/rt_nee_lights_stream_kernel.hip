// rt_nee_lights_stream_kernel.hip — k_nee_stream_f64 (rt_nee_stream_kernel.hip) with the light code of rt_scene_set_lights'
// list (rt_nee_lights.h), behind rt_render_nee and rt_render_nee_multi on a scene that carries such a list.  The same body
// (rt_nee_stream.h), the same queue, delivery and cancel.  PRIMS_ANY only.
#include "rt_nee_stream.h"
#include "rt_nee_lights.h"
#include "rt_variant_dispatch.h"

namespace RT_KNS {

// Held to the waves per SIMD and compiled in the prologue shape of k_nee_stream_f64's form of the same key (rt_nee_stream.h:
// kStreamWaves, kStreamShape); DESIGN.md 4.8 has the registers this leaves the extended forms with.
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH>
__global__ __launch_bounds__(256, (kStreamWaves<PRIMS, TEXTURED, SPECULAR, BVH>)) void k_nee_lights_stream_f64(const TraceArgs A, const NeeArgs N,
                                                                                                             const NeeLightArgs X) {
    nee_stream<PRIMS, TEXTURED, SPECULAR, BVH, ExtendedLights>(A, N, X);
}

} // namespace RT_KNS

namespace {
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH> struct LightsStreamVariant {
    static void launch(const rtdev::TraceArgs &a, const rtdev::NeeArgs &n, const rtdev::NeeLightArgs &x, unsigned blocks, hipStream_t stream) {
        hipLaunchKernelGGL((RT_KNS::k_nee_lights_stream_f64<PRIMS, TEXTURED, SPECULAR, BVH>), dim3(blocks), dim3(256), 0, stream, a, n, x);
    }
    // Resident blocks per CU, as StreamVariant's (rt_nee_stream_kernel.hip): at most 8 blocks of 256 threads.
    static int blocks_per_cu() {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, RT_KNS::k_nee_lights_stream_f64<PRIMS, TEXTURED, SPECULAR, BVH>, 256, 0) != hipSuccess)
            return 1;
        return n < 1 ? 1 : (n > 8 ? 8 : n);
    }
};
} // namespace

// Resident blocks per CU of the variant (the persistent grid is CUs x this).
extern "C" int RT_LAUNCHER(rtdev_nee_lights_stream_blocks_per_cu)(int textured, int specular, int bvh) {
    return rtdev::dispatch_any_variant<LightsStreamVariant>(textured != 0, specular != 0, bvh != 0,
                                                            [](auto v) { return decltype(v)::blocks_per_cu(); });
}

// rtdev_launch_nee_stream's launch with the extended light code.
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_nee_lights_stream)(const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee,
                                                                  const rtdev::NeeLightArgs *lights, int textured, int specular,
                                                                  int bvh, unsigned blocks, hipStream_t stream) {
    if (blocks == 0 || args->n_items == 0 || args->samples <= 0) return hipSuccess;
    rtdev::dispatch_any_variant<LightsStreamVariant>(textured != 0, specular != 0, bvh != 0, [&](auto v) {
        decltype(v)::launch(*args, *nee, *lights, blocks, stream);
    });
    return hipGetLastError();
}
