// rt_occlusion_kernel.hip — the occlusion query behind rt_trace_occlusion_device (include/rt_occlusion.h; DESIGN.md section
// 4.16): is there a hit inside the ray's window, one lane per ray, four bytes written per ray.  Linear scenes run the
// any-mode loop of rt_rays_kernel.hip over the wave-uniform table, scenes with a tree any_hit_bvh (rt_bvh_any.h), which
// leaves at the first accepted primitive.  Compiled in both arithmetic flavours, like k_trace_rays_f64: the answer is that
// kernel's closest query's "prim >= 0", bit for bit.
// No hit record, no `order` table, no LDS, no scratch, no inline assembly of its own.
#include "rt_bvh_any.h"
#include "rt_scene.h"
#include "rt_query_ray.h"

namespace RT_KNS {

// Lane i = ray i, 256 lanes per block.  TraceArgs comes FIRST in the kernel's arguments: any_hit_bvh reads the root box
// through the kernarg segment (rt_trace_common.h: kernargs_here).  A NULL optional plane of R is the default of every ray.
template <bool BVH>
__global__ __launch_bounds__(256) void k_occluded_f64(const TraceArgs A, const RtRays R, int32_t *__restrict__ occluded, const int n) {
    const unsigned ray = blockIdx.x * 256u + threadIdx.x; // (n <= INT32_MAX: the last block's lanes stay below 2^31)
    if (ray >= (unsigned)n) return;
    const size_t r = (size_t)ray;

    // judged and normalised before any hit code runs (rt_query_ray.h): the walk sees dn and [lo, hi]
    const QueryRay q = load_query_ray(R, r);
    const d3 o = q.o, dn = q.dn;
    const double time = q.time, t_min = q.lo, t_max = q.hi;
    const bool valid = q.valid;

    bool found = false;
    if (valid) {
        const d3 inv_d = rcp3(dn);
        const double inv_a = rcp_f64(len2(dn));
        if (BVH) {
            found = any_hit_bvh<PRIMS_ANY>(A, bvh_nodes_for(A, dn), o, dn, inv_d, inv_a, time, t_min, t_max);
        } else {
            // a lane stops at its first accepted primitive; the wave leaves when all its lanes have stopped
            for (int i = 0; i < A.n_prims; ++i) {
                double t;
                int aux;
                if (!found && prim_t<PRIMS_ANY>(load_prim_uniform(A.prims, i), o, dn, inv_d, inv_a, time, t_min, t_max, t, aux)) found = true;
                if (ballot(!found) == 0) break;
            }
        }
    }
    occluded[r] = valid ? (found ? 1 : 0) : RT_RAY_INVALID;
}

} // namespace RT_KNS

// n rays (0 < n) of device planes against args' scene; the tree is walked when args->n_bvh_nodes > 0.
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_occlusion)(const rtdev::TraceArgs *args, const RtRays *rays, int32_t *occluded, int n,
                                                          hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)n + 255) / 256)), block(256);
    if (args->n_bvh_nodes > 0) hipLaunchKernelGGL((RT_KNS::k_occluded_f64<true>), grid, block, 0, stream, *args, *rays, occluded, n);
    else hipLaunchKernelGGL((RT_KNS::k_occluded_f64<false>), grid, block, 0, stream, *args, *rays, occluded, n);
    return hipGetLastError();
}
