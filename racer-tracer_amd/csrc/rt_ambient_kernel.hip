// rt_ambient_kernel.hip — the ambient-occlusion query behind rt_trace_ambient_device and rt_render_ambient_device
// (include/rt_ambient.h): the rays of a point's hemisphere samples are formed in registers, walked
// with the occlusion kernel's own walk (rt_occlusion_kernel.hip) and counted with one ballot per round: four bytes written
// per point where the caller's route writes some 80 per ray.  Compiled in both arithmetic flavours.
// No atomics, no LDS, no scratch; its only inline assembly is the empty statement that pins dhat (below).
#include "rt_bvh_any.h"
#include "rt_scene.h"
#include "rt_query_ray.h"
#include "../../include/rt_ambient.h"

namespace RT_KNS {

// What a launch brings beside the points: the params as the lanes use them, where the answer goes and the optional export.
struct AmbientArgs {
    int samples, shift;        // S; log2 of G = min(S, 64), the lanes of one point
    double bias, radius;       // where the points bring no plane
    double time;               // ... and the time where they bring none (0; a frame's (time_a + time_b) / 2)
    uint32_t k0, k1, base;     // the seed's halves; (uint32)index_base
    int32_t *open;             // [n], or NULL: the frame form
    double *frame;             // [n * 3]: sqrt(open / S) in three channels, 1 where obj_id == -1; or NULL
    const int32_t *obj_id;     // the frame's guide plane
    RtAmbientRays rays;        // the export: any plane may be NULL
};

// x as it stands in its register: the products that form dhat are rounded HERE, never contracted into a sum further down the
// walk, which the occlusion kernel, loading the exported dhat from memory, could not do either.
__device__ __forceinline__ double pinned(double x) {
    asm volatile("" : "+v"(x));
    return x;
}

// One lane per ray, 256 lanes per block.  With G = min(S, 64) a wave holds 64 / G points: lane l of the grid handles point
// l / G and the samples (l mod G) + 64 * round of S / G rounds (one round unless S > 64).  A point's open samples are one
// ballot ANDed with its group's mask and a popcount per round; the group's first lane writes.  TraceArgs comes FIRST in the
// kernel's arguments (any_hit_bvh reads the root box through the kernarg segment).
//
// The walk is k_occluded_f64's on the values that kernel would load from the exported ray: dhat's largest component lies
// in [1 / sqrt 3, 1], inside rt_query_ray.h's band, so its prologue multiplies direction and window by 1.0 and hands the
// walk these very bits.
template <bool BVH>
__global__ __launch_bounds__(256) void k_ambient_f64(const TraceArgs A, const RtRays P, const AmbientArgs Q, const int n) {
    const uint64_t lane = (uint64_t)blockIdx.x * 256u + threadIdx.x; // (n * G <= 2^37)
    const int group = 1 << Q.shift;
    const uint64_t point = lane >> Q.shift;
    if (point >= (uint64_t)n) return; // whole groups leave: G divides 64
    const size_t p = (size_t)point;
    const int sub = (int)(lane & (unsigned)(group - 1));
    const int in_wave = (int)(threadIdx.x & 63u);
    const uint64_t mask = group == 64 ? ~0ull : ((1ull << group) - 1ull) << (in_wave - sub);

    // the point, judged by the ray query's own comparisons (rt_query_ray.h) with the normal in the direction's place
    const d3 o = ld3(P.origin + 3 * p);
    const d3 normal = ld3(P.direction + 3 * p);
    const double t_min = P.t_min ? P.t_min[p] : Q.bias;
    const double t_max = P.t_max ? P.t_max[p] : Q.radius;
    const double time = P.time ? P.time[p] : Q.time;
    const bool valid = rt_query::ray_valid(o.x, o.y, o.z, normal.x, normal.y, normal.z, time, t_min, t_max);
    const d3 nhat = unit_fast(normal * rt_query::ray_scale(normal.x, normal.y, normal.z).down);
    const uint32_t g = Q.base + (uint32_t)p; // index_base + n <= 2^32: no wrap

    int open = 0;
    for (int s = sub; s < Q.samples; s += 64) { // wave-uniform trip count
        d3 dhat = mk(0.0, 0.0, 0.0);
        bool found = false;
        if (valid) {
            d3 u;
            for (uint32_t i = 0;; ++i) { // vec3.rs:424-430 under the addressed-draw contract, purpose RT_RNG_AMBIENT
                u = sphere_candidate(philox4x32(g, (uint32_t)s, RT_RNG_AMBIENT, i, Q.k0, Q.k1));
                if (len2(u) < 1.0) break;
            }
            d3 dir = nhat + unit_fast(u); // lambertian.rs:27
            if (fabs(dir.x) < 1e-8 && fabs(dir.y) < 1e-8 && fabs(dir.z) < 1e-8) dir = nhat; // vec3.rs near_zero
            dhat = unit_fast(dir);
            dhat = mk(pinned(dhat.x), pinned(dhat.y), pinned(dhat.z));
            // ---- k_occluded_f64's walk
            const d3 inv_d = rcp3(dhat);
            const double inv_a = rcp_f64(len2(dhat));
            if (BVH) {
                found = any_hit_bvh<PRIMS_ANY>(A, bvh_nodes_for(A, dhat), o, dhat, inv_d, inv_a, time, t_min, t_max);
            } else {
                for (int i = 0; i < A.n_prims; ++i) {
                    double t;
                    int aux;
                    if (!found && prim_t<PRIMS_ANY>(load_prim_uniform(A.prims, i), o, dhat, inv_d, inv_a, time, t_min, t_max, t, aux)) found = true;
                    if (ballot(!found) == 0) break;
                }
            }
        }
        open += __builtin_popcountll(ballot(valid && !found) & mask);
        const size_t j = p * (size_t)Q.samples + (size_t)s;
        if (Q.rays.origin) {
            Q.rays.origin[3 * j] = o.x;
            Q.rays.origin[3 * j + 1] = o.y;
            Q.rays.origin[3 * j + 2] = o.z;
        }
        if (Q.rays.direction) {
            Q.rays.direction[3 * j] = dhat.x;
            Q.rays.direction[3 * j + 1] = dhat.y;
            Q.rays.direction[3 * j + 2] = dhat.z;
        }
        if (Q.rays.t_min) Q.rays.t_min[j] = t_min;
        if (Q.rays.t_max) Q.rays.t_max[j] = t_max;
        if (Q.rays.time) Q.rays.time[j] = time;
    }
    if (sub != 0) return;
    const int answer = valid ? open : RT_RAY_INVALID;
    if (Q.open) Q.open[p] = answer;
    if (Q.frame) {
        // IEEE division and square root in both flavours (a guide hit is never an invalid point)
        const double v = Q.obj_id[p] == -1 ? 1.0 : sqrt((double)answer / (double)Q.samples);
        Q.frame[3 * p] = v;
        Q.frame[3 * p + 1] = v;
        Q.frame[3 * p + 2] = v;
    }
}

} // namespace RT_KNS

// n points (0 < n) of device planes against args' scene, params checked by the caller; the tree is walked when
// args->n_bvh_nodes > 0.  open / frame + obj_id: where the answer goes (rt_ambient.h's two forms); walked may be NULL.
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_ambient)(const rtdev::TraceArgs *args, const RtRays *points, int n,
                                                        const RtAmbientParams *params, double default_time, int32_t *open,
                                                        double *frame, const int32_t *obj_id, const RtAmbientRays *walked,
                                                        hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    RT_KNS::AmbientArgs q;
    q.samples = params->samples;
    const int group = params->samples < 64 ? params->samples : 64; // a power of two
    q.shift = __builtin_ctz((unsigned)group);
    q.bias = params->bias;
    q.radius = params->radius;
    q.time = default_time;
    q.k0 = (uint32_t)(params->seed & 0xffffffffu);
    q.k1 = (uint32_t)(params->seed >> 32);
    q.base = (uint32_t)params->index_base;
    q.open = open;
    q.frame = frame;
    q.obj_id = obj_id;
    q.rays = walked ? *walked : RtAmbientRays{nullptr, nullptr, nullptr, nullptr, nullptr};
    const dim3 grid((unsigned)(((int64_t)n * group + 255) / 256)), block(256);
    if (args->n_bvh_nodes > 0) hipLaunchKernelGGL((RT_KNS::k_ambient_f64<true>), grid, block, 0, stream, *args, *points, q, n);
    else hipLaunchKernelGGL((RT_KNS::k_ambient_f64<false>), grid, block, 0, stream, *args, *points, q, n);
    return hipGetLastError();
}
