// rt_bvh_kbest.h — the k-nearest list of the multi-hit query and its walk of the skip-link BVH: the k primitives with the
// smallest hit inside [t_min, t_max].  (include/rt_multihit.h.)
//
// A THIRD COPY of closest_hit_bvh (rt_trace_common.h), next to any_hit_bvh (rt_bvh_any.h), on purpose and for that
// header's reason: the descent step is 58 % of the BVH variant's vector instructions, and a helper shared with it would
// move instructions in the pooled kernel.  Whoever changes one of the three reads the other two.  Copied line for line:
// the f64 clip to the root box through kernargs_here(), the f32 SlabRay, the window ends rounded outward, the
// sentinel-terminated descent with its v_pk_fma_f32 step, and the leaf test that runs sphere_t on the LeafGeo record
// before the tag is asked.
// What differs: the far end of the window is not the best hit but the K-TH best.  Until k hits are held it is t_max's;
// from then on it is the k-th entry's t, and its f32 form (best_f) is recomputed whenever that entry changed in a leaf,
// with the outward rounding closest_hit_bvh applies when best_t moves.
//
// WHY NO PRIMITIVE AMONG THE TRUE FIRST k CAN BE CULLED.  Let far be the f64 far end at some moment: t_max, or the t of
// the k-th entry of a list that holds k hits of k different primitives, all inside the window.  Let P be a primitive whose
// hit t_P belongs to the true first k and is not in the list.  Then t_P <= far: otherwise the list's k entries, all
// <= far < t_P, would be k primitives other than P that come before it.  far never grows (an insertion can only lower the
// k-th entry), so t_P <= far held at every earlier moment too.  (1) A node box that contains P contains the point at t_P,
// so the ray's exact interval with it reaches down to t_P <= far; the f32 test sees the box padded and the window's ends
// rounded outward by more than its own error (closest_hit_bvh's budget), so it cannot reject the node: P's leaf is
// entered, in any node array order.  (2) In the leaf P is tested over [t_min, far].  Its hit over [t_min, t_max] is t_P,
// and the hit over the shorter window is the same one: for a sphere the root chosen is the nearer one inside the window,
// else the farther, and shortening the far end to a value >= t_P removes neither t_P nor adds a nearer root; every other
// primitive has one candidate.  So P is accepted and inserted.  (3) An entry is only ever pushed out by k others that
// are not behind it.  Hits with t EXACTLY equal to the k-th entry are where the order of the walk shows: include/
// rt_multihit.h leaves those unspecified.
#pragma once
#include "rt_trace_common.h"

namespace RT_KNS {

// CAP entries of (t, record index, aux), sorted by t, in registers.  The list is a head and a shorter list, and every
// function below recurses over that at compile time: there is no array and no subscript at all, so nothing the optimiser
// does or leaves undone can turn the list into an indexed object in scratch or LDS (as arrays with fully unrolled loops
// did: the alloca was promoted to LDS for CAP = 4 and spilled for CAP = 8).  An empty entry is (+inf, -1, 0); a hit has a
// finite t, so "k entries are held" is "the k-th entry's t < inf".
template <int CAP>
struct KBest {
    double t;
    int rec, aux;
    KBest<CAP - 1> rest;
};
template <>
struct KBest<0> {};

template <int CAP>
__device__ __forceinline__ void kbest_clear(KBest<CAP> &L) {
    if constexpr (CAP > 0) {
        L.t = __builtin_inf();
        L.rec = -1;
        L.aux = 0;
        kbest_clear(L.rest);
    }
}

// Compare-and-shift: at every entry the nearer of (entry, carried hit) stays and the other is carried on; what is carried
// past the last entry is gone.  A hit equal in t to an entry goes behind it.
template <int CAP>
__device__ __forceinline__ void kbest_insert(KBest<CAP> &L, double t, int rec, int aux) {
    if constexpr (CAP > 0) {
        const bool here = t < L.t;
        const double t_on = here ? L.t : t;
        const int rec_on = here ? L.rec : rec, aux_on = here ? L.aux : aux;
        L.t = here ? t : L.t;
        L.rec = here ? rec : L.rec;
        L.aux = here ? aux : L.aux;
        kbest_insert(L.rest, t_on, rec_on, aux_on);
    }
}

// The t of entry k (counted from 1; wave-uniform), +inf where the list is shorter: a chain of selects.
template <int CAP>
__device__ __forceinline__ double kbest_kth(const KBest<CAP> &L, int k) {
    if constexpr (CAP > 0) {
        const double behind = kbest_kth(L.rest, k - 1);
        return k == 1 ? L.t : behind;
    } else {
        return __builtin_inf();
    }
}

// The far end of the window for a list that is to hold k (1 <= k <= CAP) entries: t_max until k are held, then the k-th
// entry's t, which lies inside the window.
template <int CAP>
__device__ __forceinline__ double kbest_far(const KBest<CAP> &L, int k, double t_max) {
    return fmin(kbest_kth(L, k), t_max); // (an empty entry is +inf; t_max is not NaN for a valid ray)
}

// The first entry, taken out; the others move up.  k calls hand out the list in order.
template <int CAP>
__device__ __forceinline__ void kbest_move_up(KBest<CAP> &L) {
    if constexpr (CAP > 1) {
        L.t = L.rest.t;
        L.rec = L.rest.rec;
        L.aux = L.rest.aux;
        kbest_move_up(L.rest);
    } else if constexpr (CAP == 1) {
        L.t = __builtin_inf();
        L.rec = -1;
        L.aux = 0;
    }
}
template <int CAP>
__device__ __forceinline__ void kbest_pop(KBest<CAP> &L, double &t, int &rec, int &aux) {
    t = L.t;
    rec = L.rec;
    aux = L.aux;
    kbest_move_up(L);
}

// `nodes`: the caller's choice, as for the closest walk (bvh_nodes_for(A, d)); any child order is correct (above).
// The kernel's FIRST argument must be the TraceArgs: the root box is read through the kernarg segment.
// L: cleared by the caller; on return its first k entries are the answer (entries behind them are leftovers).
template <int PRIMS, int CAP>
__device__ __forceinline__ void kbest_hit_bvh(const TraceArgs &A, const BvhNode *nodes, d3 o, d3 d, d3 inv_d, double inv_a,
                                              double time, double t_min, double t_max, int k, KBest<CAP> &L) {
    // culling in single precision, as in closest_hit_bvh: the ray clipped to the root box in f64, f32 boxes around the
    // root's centre, the window's ends rounded outward by 2^-20 relative
    const RT_CONSTANT TraceArgs *K = kernargs_here();
    double t0 = 0.0; // ray parameter of the clipped origin
    {
        const double ax = (K->bvh_root_mn[0] - o.x) * inv_d.x, bx = (K->bvh_root_mx[0] - o.x) * inv_d.x;
        const double ay = (K->bvh_root_mn[1] - o.y) * inv_d.y, by = (K->bvh_root_mx[1] - o.y) * inv_d.y;
        const double az = (K->bvh_root_mn[2] - o.z) * inv_d.z, bz = (K->bvh_root_mx[2] - o.z) * inv_d.z;
        // fmin/fmax drop NaNs (0 * inf on a slab boundary), which keeps the test conservative
        const double t_enter = fmax(fmax(fmin(ax, bx), fmin(ay, by)), fmin(az, bz));
        const double t_exit = fmin(fmin(fmax(ax, bx), fmax(ay, by)), fmin(fmax(az, bz), t_max));
        if (!(fmax(t_enter, t_min) <= t_exit)) return; // misses the scene's bounds
        if (t_enter > 0.0) t0 = t_enter;
    }
    const SlabRay sr = slab_ray((float)(fma(t0, d.x, o.x) - K->bvh_center[0]), (float)(fma(t0, d.y, o.y) - K->bvh_center[1]),
                                (float)(fma(t0, d.z, o.z) - K->bvh_center[2]), inv_d.x, inv_d.y, inv_d.z); // rt_bvh_slab.h
    const float slack = 0x1p-20f; // of the WINDOW ends only (f64 -> f32, rounded outward); the box test itself carries none
    // the window [t_min, far] seen from the clipped origin, rounded outward
    const float tmin_f = (float)(t_min - t0) - fabsf((float)(t_min - t0)) * slack - 0x1p-126f;
    auto far_of = [&](double bt) { // upper end of the window; never below its lower end, so that the sentinel is always "hit"
        const float f = (float)(bt - t0);
        return fmaxf(f + fabsf(f) * slack, tmin_f);
    };
    double far = t_max; // the f64 far end: t_max until k entries are held, then the k-th entry's t
    float best_f = far_of(far);
    if (!(tmin_f <= best_f)) return; // NaN somewhere in the ray: nothing can be hit (and the walk below relies on the order)
    // the ray's six constants as the three register pairs v_pk_fma_f32 reads (SlabRay's order)
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 p01 = {sr.ivx, sr.ivy}, p23 = {sr.ivz, sr.nox}, p45 = {sr.noy, sr.noz};
    int i = 0;
    const int n = A.n_bvh_nodes;
    while (i < n) {
        int fc = 0;
        // DESCENT: closest_hit_bvh's, unchanged (its comment has the termination argument: the index only grows, and at
        // the sentinel, index n, the test cannot fail because tmin_f <= best_f are ordered and not NaN; far_of keeps
        // best_f there)
        for (;;) {
            const uint4 *raw = reinterpret_cast<const uint4 *>(&nodes[i]);
            const uint4 q0 = raw[0], q1 = raw[1]; // the whole 32-byte node in two 128-bit reads BEFORE the test
            const f2 qx = {__uint_as_float(q0.x), __uint_as_float(q0.y)}, qy = {__uint_as_float(q0.z), __uint_as_float(q0.w)},
                     qz = {__uint_as_float(q1.x), __uint_as_float(q1.y)};
            f2 tx, ty, tz;
            float nx, ny, nz, fx, fy, fz, t_near, t_far;
            // (lo, hi) * (iv, iv) + (no, no): op_sel picks the half of each 64-bit source for the low result, op_sel_hi for the high one
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(tx) : "v"(qx), "v"(p01), "v"(p23)); // x: ivx = p01.lo, nox = p23.hi
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,0]" : "=v"(ty) : "v"(qy), "v"(p01), "v"(p45)); // y: ivy = p01.hi, noy = p45.lo
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(tz) : "v"(qz), "v"(p23), "v"(p45)); // z: ivz = p23.lo, noz = p45.hi
            // (one statement: between separate asm statements the compiler puts an s_nop for hazards it cannot rule out)
            asm("v_min_f32 %0, %8, %9\n\tv_max_f32 %1, %8, %9\n\t"
                "v_min_f32 %2, %10, %11\n\tv_max_f32 %3, %10, %11\n\t"
                "v_min_f32 %4, %12, %13\n\tv_max_f32 %5, %12, %13\n\t"
                "v_max_f32 %4, %4, %14\n\tv_min_f32 %5, %5, %15\n\t"
                "v_max3_f32 %6, %0, %2, %4\n\tv_min3_f32 %7, %1, %3, %5"
                : "=&v"(nx), "=&v"(fx), "=&v"(ny), "=&v"(fy), "=&v"(nz), "=&v"(fz), "=&v"(t_near), "=&v"(t_far)
                : "v"(tx.x), "v"(tx.y), "v"(ty.x), "v"(ty.y), "v"(tz.x), "v"(tz.y), "v"(tmin_f), "v"(best_f));
            const bool hit = !(t_near > t_far); // (a NaN, which the window's ends exclude, would step on: the walk still ends)
            fc = (int)q1.w;
            i = hit ? i + 1 : (int)q1.z; // inner: first child; leaf: its skip link is i + 1 as well
            if (hit && fc != 0) break; // a leaf (or the sentinel) was entered
        }
        const int count = fc & 7, first = fc >> 3; // the sentinel: no primitives, and i = n + 1 ends the walk
        const double far_was = far;
        for (int q = 0; q < count; ++q) { // the leaf's primitives (stored contiguously in leaf order)
            const int pi = first + q;
            double t;
            int aux = 0;
            // the compact record and the sphere test WITHOUT asking the tag first, as in closest_hit_bvh: a record of
            // another kind (tag 1) holds zeros here, its sphere test is discarded and the general routine runs for it
            const LeafGeo &G = A.leaf_geo[pi];
            const long long tag = G.tag;
            const d3 center = ld3(G.c0) + ((time - A.leaf_time_a) * A.leaf_inv_dt) * ld3(G.dc); // sphere.rs:39-59 / moving_sphere.rs:37-39,49-69
            bool hit = sphere_t(center, G.radius2, o, d, inv_a, t_min, far, t) && tag == 0;
            if (tag != 0) hit = prim_t<PRIMS>(A.prims[pi], o, d, inv_d, inv_a, time, t_min, far, t, aux);
            if (hit) {
                kbest_insert(L, t, pi, aux);
                far = kbest_far(L, k, t_max); // (inside the leaf too: the next primitive of it is tested over the new window)
            }
        }
        // t_max's until k entries are held; from then on recomputed whenever the k-th entry changed (far only ever falls)
        if (far < far_was) best_f = far_of(far);
    }
}

} // namespace RT_KNS
