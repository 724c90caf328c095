// rt_rays_kernel.hip — the ray query behind rt_trace_rays_device (include/rt_rays.h): the scene's
// closest hit, or any hit, of rays the caller brings, one lane per ray.  The hit functions are rt_trace_common.h's, which
// all take the ray's window: prim_t<PRIMS_ANY> over the wave-uniform table for linear scenes, closest_hit_bvh<PRIMS_ANY>
// for scenes with a tree (rt_path_steps.h's closest_hit fixes [0.001, inf) and is not used).  Compiled in both arithmetic
// flavours: an RT_ARITH_REFERENCE scene is answered with IEEE divisions and the six-rect box.
// No LDS, no scratch, no inline assembly of its own.
#include "rt_trace_common.h"
#include "rt_scene.h"
#include "rt_query_ray.h"

namespace RT_KNS {

// Lane i = ray i, 256 lanes per block.  TraceArgs comes FIRST in the kernel's arguments: closest_hit_bvh reads the root box
// through the kernarg segment (rt_trace_common.h: kernargs_here).  `order`: the description index of every device record
// (rt_plan.h).  A NULL optional plane of R is the default of every ray; a NULL plane of H is not written.
template <bool BVH, bool ANY_HIT>
__global__ __launch_bounds__(256) void k_trace_rays_f64(const TraceArgs A, const RtRays R, const RtRayHits H,
                                                        const int32_t *__restrict__ order, const int n) {
    const unsigned ray = blockIdx.x * 256u + threadIdx.x; // (n <= INT32_MAX: the last block's lanes stay below 2^31)
    if (ray >= (unsigned)n) return;
    const size_t r = (size_t)ray;

    // judged and normalised before any hit code runs (rt_query_ray.h): the walk sees dn and [lo, hi], the record o, d and t
    const QueryRay q = load_query_ray(R, r);
    const d3 o = q.o, dn = q.dn;
    const double time = q.time, t_min = q.lo, t_max = q.hi;
    const bool valid = q.valid;
    const double INF = __builtin_inf();

    double best_t = t_max;
    int best = -1, best_aux = 0;
    if (valid) {
        const d3 inv_d = rcp3(dn);
        const double inv_a = rcp_f64(len2(dn));
        if (BVH) { // (any mode too: an early-out walk would be a second closest_hit_bvh)
            closest_hit_bvh<PRIMS_ANY>(A, bvh_nodes_for(A, dn), o, dn, inv_d, inv_a, time, t_min, best_t, best, best_aux);
        } else if (ANY_HIT) {
            // a lane stops at its first accepted primitive; the wave leaves when all its lanes have stopped
            for (int i = 0; i < A.n_prims; ++i) {
                double t;
                int aux;
                if (best < 0 && prim_t<PRIMS_ANY>(load_prim_uniform(A.prims, i), o, dn, inv_d, inv_a, time, t_min, best_t, t, aux)) {
                    best_t = t;
                    best = i;
                    best_aux = aux;
                }
                if (ballot(best < 0) == 0) break;
            }
        } else {
            for (int i = 0; i < A.n_prims; ++i) { // the render's loop: t == best_t is accepted, the later primitive wins a tie
                double t;
                int aux;
                if (prim_t<PRIMS_ANY>(load_prim_uniform(A.prims, i), o, dn, inv_d, inv_a, time, t_min, best_t, t, aux)) {
                    best_t = t;
                    best = i;
                    best_aux = aux;
                }
            }
        }
    }

    d3 x = mk(0.0, 0.0, 0.0), nrm = x;
    double t = INF, u = 0.0, v = 0.0;
    int prim = valid ? RT_RAY_MISS : RT_RAY_INVALID, id = -1, front = 0;
    if (best >= 0) {
        const Prim &P = A.prims[best];
        // the f64 sphere_uv (FAST_UV = false): the f32 form is the pooled kernel's own business
        const d3 d = caller_direction(R, r);
        t = caller_t(d, best_t); // in units of the caller's d, which forms the point with it
        const Hit h = prim_hit_record<PRIMS_ANY, true, false>(P, o, d, time, t, best_aux, H.uv != nullptr);
        x = h.point;
        nrm = h.normal;
        u = h.u;
        v = h.v;
        front = h.front ? 1 : 0;
        prim = order[best];
        id = P.obj_id;
    }
    if (H.t) H.t[r] = t;
    if (H.point) {
        H.point[3 * r + 0] = x.x;
        H.point[3 * r + 1] = x.y;
        H.point[3 * r + 2] = x.z;
    }
    if (H.normal) {
        H.normal[3 * r + 0] = nrm.x;
        H.normal[3 * r + 1] = nrm.y;
        H.normal[3 * r + 2] = nrm.z;
    }
    if (H.uv) {
        H.uv[2 * r + 0] = u;
        H.uv[2 * r + 1] = v;
    }
    if (H.prim) H.prim[r] = prim;
    if (H.obj_id) H.obj_id[r] = id;
    if (H.front_face) H.front_face[r] = front;
}

} // namespace RT_KNS

// n rays (0 < n) of device planes against args' scene; the tree is walked when args->n_bvh_nodes > 0.
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_trace_rays)(const rtdev::TraceArgs *args, const RtRays *rays, const RtRayHits *hits,
                                                           const int32_t *order, int n, int any_hit, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)n + 255) / 256)), block(256);
    const bool bvh = args->n_bvh_nodes > 0;
    // (a tree answers any mode with its closest walk: one instantiation)
    if (bvh) hipLaunchKernelGGL((RT_KNS::k_trace_rays_f64<true, false>), grid, block, 0, stream, *args, *rays, *hits, order, n);
    else if (any_hit) hipLaunchKernelGGL((RT_KNS::k_trace_rays_f64<false, true>), grid, block, 0, stream, *args, *rays, *hits, order, n);
    else hipLaunchKernelGGL((RT_KNS::k_trace_rays_f64<false, false>), grid, block, 0, stream, *args, *rays, *hits, order, n);
    return hipGetLastError();
}
