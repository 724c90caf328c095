// rt_bvh_any.h — the any-hit walk of the skip-link BVH: is there a primitive with a hit in [t_min, t_max]?  (DESIGN.md
// section 4.16; include/rt_occlusion.h.)
//
// A SECOND COPY of closest_hit_bvh (rt_trace_common.h), on purpose: that function's descent step is 58 % of the BVH
// variant's vector instructions, and a helper shared with it would move instructions in the pooled kernel.  (That was
// compiled once, a shared prologue plus a shared `bvh_descend`, all __forceinline__, for this walk, the closest one and
// kbest_hit_bvh: tools/device_asm_digests.py --counts showed 16 of 84 functions moved, all eight PRETRACE variants of
// k_trace_pool_f64 among them, and one exact variant gained scratch loads and stores.)  Whoever
// changes one of the two reads the other.  Copied from it, line for line: the f64 clip to the root box through
// kernargs_here(), the f32 SlabRay, the window ends rounded outward, the sentinel-terminated descent with its
// v_pk_fma_f32 step, and the leaf test that runs sphere_t on the LeafGeo record before the tag is asked.
// What differs: the far end of the window never moves (there is no best, best_aux or far_of update), and a lane leaves
// the walk at its first accepted primitive; the wave goes on until every lane has left or has finished the tree.
//
// Until a lane's first acceptance both walks visit the same nodes in the same order with the same window — the closest
// walk's far end only moves at an acceptance — and make the same decisions where there is none: the answer IS
// "closest_hit_bvh finds a hit", bit for bit, for the same node array.
#pragma once
#include "rt_trace_common.h"

namespace RT_KNS {

// `nodes`: the caller's choice, as for the closest walk (bvh_nodes_for(A, d)); any child order is correct for a yes or no.
// The kernel's FIRST argument must be the TraceArgs: the root box is read through the kernarg segment.
template <int PRIMS>
__device__ __forceinline__ bool any_hit_bvh(const TraceArgs &A, const BvhNode *nodes, d3 o, d3 d, d3 inv_d, double inv_a,
                                            double time, double t_min, double t_max) {
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
        if (!(fmax(t_enter, t_min) <= t_exit)) return false; // misses the scene's bounds
        if (t_enter > 0.0) t0 = t_enter;
    }
    const SlabRay sr = slab_ray((float)(fma(t0, d.x, o.x) - K->bvh_center[0]), (float)(fma(t0, d.y, o.y) - K->bvh_center[1]),
                                (float)(fma(t0, d.z, o.z) - K->bvh_center[2]), inv_d.x, inv_d.y, inv_d.z); // rt_bvh_slab.h
    const float slack = 0x1p-20f; // of the WINDOW ends only (f64 -> f32, rounded outward); the box test itself carries none
    // the window [t_min, t_max] seen from the clipped origin, rounded outward; the far end never below the near one, so
    // that the sentinel is always "hit"
    const float tmin_f = (float)(t_min - t0) - fabsf((float)(t_min - t0)) * slack - 0x1p-126f;
    const float far_raw = (float)(t_max - t0);
    const float tmax_f = fmaxf(far_raw + fabsf(far_raw) * slack, tmin_f);
    if (!(tmin_f <= tmax_f)) return false; // NaN somewhere in the ray: nothing can be hit (and the walk below relies on the order)
    // the ray's six constants as the three register pairs v_pk_fma_f32 reads (SlabRay's order)
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 p01 = {sr.ivx, sr.ivy}, p23 = {sr.ivz, sr.nox}, p45 = {sr.noy, sr.noz};
    int i = 0;
    const int n = A.n_bvh_nodes;
    bool found = false;
    while (i < n) {
        int fc = 0;
        // DESCENT: closest_hit_bvh's, unchanged (its comment has the termination argument: the index only grows, and at
        // the sentinel, index n, the test cannot fail because tmin_f <= tmax_f are ordered and not NaN)
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
                : "v"(tx.x), "v"(tx.y), "v"(ty.x), "v"(ty.y), "v"(tz.x), "v"(tz.y), "v"(tmin_f), "v"(tmax_f));
            const bool hit = !(t_near > t_far); // (a NaN, which the window's ends exclude, would step on: the walk still ends)
            fc = (int)q1.w;
            i = hit ? i + 1 : (int)q1.z; // inner: first child; leaf: its skip link is i + 1 as well
            if (hit && fc != 0) break; // a leaf (or the sentinel) was entered
        }
        const int count = fc & 7, first = fc >> 3; // the sentinel: no primitives, and i = n + 1 ends the walk
        for (int k = 0; k < count && !found; ++k) { // the leaf's primitives, up to the first accepted one
            const int pi = first + k;
            double t;
            int aux = 0;
            // the compact record and the sphere test WITHOUT asking the tag first, as in closest_hit_bvh: a record of
            // another kind (tag 1) holds zeros here, its sphere test is discarded and the general routine runs for it
            const LeafGeo &G = A.leaf_geo[pi];
            const long long tag = G.tag;
            const d3 center = ld3(G.c0) + ((time - A.leaf_time_a) * A.leaf_inv_dt) * ld3(G.dc); // sphere.rs:39-59 / moving_sphere.rs:37-39,49-69
            bool hit = sphere_t(center, G.radius2, o, d, inv_a, t_min, t_max, t) && tag == 0;
            if (tag != 0) hit = prim_t<PRIMS>(A.prims[pi], o, d, inv_d, inv_a, time, t_min, t_max, t, aux);
            found = hit;
        }
        if (found) break; // this lane leaves; the others walk on
    }
    return found;
}

} // namespace RT_KNS
