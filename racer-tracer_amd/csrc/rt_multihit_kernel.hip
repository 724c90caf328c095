// rt_multihit_kernel.hip — the multi-hit query behind rt_trace_rays_multi_device (include/rt_multihit.h; DESIGN.md section
// 4.17): the first k primitives along each ray the caller brings, one lane per ray.  Each lane keeps the k nearest accepted
// hits in registers (rt_bvh_kbest.h: KBest) and tests every primitive over [t_min, far], far being t_max until k hits are
// held and the k-th hit's t from then on.  Linear scenes run the render's loop over the wave-uniform table with
// prim_t<PRIMS_ANY>, scenes with a tree kbest_hit_bvh.  Compiled in both arithmetic flavours, like k_trace_rays_f64, whose
// closest answer slot 0 repeats.
// No LDS, no scratch (the list is a compile-time recursion over scalars, never an array), no inline assembly of its own.
#include "rt_bvh_kbest.h"
#include "rt_scene.h"
#include "rt_query_ray.h"

namespace RT_KNS {

// Lane i = ray i, 256 lanes per block.  TraceArgs comes FIRST in the kernel's arguments: kbest_hit_bvh reads the root box
// through the kernarg segment (rt_trace_common.h: kernargs_here).  1 <= k <= CAP.  `order`: the description index of every
// device record (rt_plan.h).  A NULL optional plane of R is the default of every ray; a NULL plane of H, or a NULL count,
// is not written.  The planes of H are slot-major: entry (slot j, ray r) is entry j * n + r.
template <bool BVH, int CAP>
__global__ __launch_bounds__(256) void k_trace_rays_multi_f64(const TraceArgs A, const RtRays R, const RtRayHits H,
                                                              int32_t *__restrict__ count, const int32_t *__restrict__ order,
                                                              const int n, const int k) {
    const unsigned ray = blockIdx.x * 256u + threadIdx.x; // (n <= INT32_MAX: the last block's lanes stay below 2^31)
    if (ray >= (unsigned)n) return;
    const size_t r = (size_t)ray;

    // judged and normalised before any hit code runs (rt_query_ray.h): the walk sees dn and [lo, hi], the record o, d and t
    const QueryRay q = load_query_ray(R, r);
    const d3 o = q.o, dn = q.dn;
    const double time = q.time, t_min = q.lo, t_max = q.hi;
    const bool valid = q.valid;
    const double INF = __builtin_inf();

    KBest<CAP> L;
    kbest_clear(L);
    if (valid) {
        const d3 inv_d = rcp3(dn);
        const double inv_a = rcp_f64(len2(dn));
        if (BVH) {
            kbest_hit_bvh<PRIMS_ANY, CAP>(A, bvh_nodes_for(A, dn), o, dn, inv_d, inv_a, time, t_min, t_max, k, L);
        } else {
            double far = t_max;
            for (int i = 0; i < A.n_prims; ++i) { // the render's loop, with the k-th hit where it has the best one
                double t;
                int aux;
                if (prim_t<PRIMS_ANY>(load_prim_uniform(A.prims, i), o, dn, inv_d, inv_a, time, t_min, far, t, aux)) {
                    kbest_insert(L, t, i, aux);
                    far = kbest_far(L, k, t_max);
                }
            }
        }
    }

    // the slots in order: each turn takes the list's first entry (no subscript, one copy of the record code)
    int filled = 0;
    const d3 d = caller_direction(R, r);
    for (int j = 0; j < k; ++j) {
        double best_t;
        int best, best_aux;
        kbest_pop(L, best_t, best, best_aux);
        d3 x = mk(0.0, 0.0, 0.0), nrm = x;
        double t = INF, u = 0.0, v = 0.0;
        int prim = valid ? RT_RAY_MISS : RT_RAY_INVALID, id = -1, front = 0;
        if (best >= 0) {
            const Prim &P = A.prims[best];
            // the f64 sphere_uv (FAST_UV = false), as in k_trace_rays_f64
            t = caller_t(d, best_t); // in units of the caller's d, as in k_trace_rays_f64
            const Hit h = prim_hit_record<PRIMS_ANY, true, false>(P, o, d, time, t, best_aux, H.uv != nullptr);
            x = h.point;
            nrm = h.normal;
            u = h.u;
            v = h.v;
            front = h.front ? 1 : 0;
            prim = order[best];
            id = P.obj_id;
            ++filled;
        }
        const size_t e = (size_t)j * (size_t)n + r; // consecutive lanes, consecutive entries, in every slot
        if (H.t) H.t[e] = t;
        if (H.point) {
            H.point[3 * e + 0] = x.x;
            H.point[3 * e + 1] = x.y;
            H.point[3 * e + 2] = x.z;
        }
        if (H.normal) {
            H.normal[3 * e + 0] = nrm.x;
            H.normal[3 * e + 1] = nrm.y;
            H.normal[3 * e + 2] = nrm.z;
        }
        if (H.uv) {
            H.uv[2 * e + 0] = u;
            H.uv[2 * e + 1] = v;
        }
        if (H.prim) H.prim[e] = prim;
        if (H.obj_id) H.obj_id[e] = id;
        if (H.front_face) H.front_face[e] = front;
    }
    if (count) count[r] = valid ? filled : RT_RAY_INVALID;
}

} // namespace RT_KNS

// n rays (0 < n) of device planes against args' scene, 1 <= k <= RT_MULTIHIT_MAX; the tree is walked when
// args->n_bvh_nodes > 0.  Two list lengths are compiled, 4 and 8: k <= 4 takes the short one (DESIGN.md 4.17 has the
// register counts behind the split).
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_multihit)(const rtdev::TraceArgs *args, const RtRays *rays, const RtRayHits *hits,
                                                                 int32_t *count, const int32_t *order, int n, int k, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (k < 1 || k > RT_MULTIHIT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((int64_t)n + 255) / 256)), block(256);
    const bool bvh = args->n_bvh_nodes > 0;
    if (bvh && k <= 4) hipLaunchKernelGGL((RT_KNS::k_trace_rays_multi_f64<true, 4>), grid, block, 0, stream, *args, *rays, *hits, count, order, n, k);
    else if (bvh) hipLaunchKernelGGL((RT_KNS::k_trace_rays_multi_f64<true, 8>), grid, block, 0, stream, *args, *rays, *hits, count, order, n, k);
    else if (k <= 4) hipLaunchKernelGGL((RT_KNS::k_trace_rays_multi_f64<false, 4>), grid, block, 0, stream, *args, *rays, *hits, count, order, n, k);
    else hipLaunchKernelGGL((RT_KNS::k_trace_rays_multi_f64<false, 8>), grid, block, 0, stream, *args, *rays, *hits, count, order, n, k);
    return hipGetLastError();
}
