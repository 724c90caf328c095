// rt_variant_dispatch.h — the one place where a scene's runtime flags become the template arguments of a kernel variant.
// The trace kernels are compiled as PRIMS x TEXTURED x SPECULAR with the linear closest-hit loop plus PRIMS_ANY x
// TEXTURED x SPECULAR with the BVH; each kernel file wraps its kernel in a struct V<PRIMS, TEXTURED, SPECULAR, BVH> of
// static functions (launch, occupancy queries) and calls dispatch_variant<V>.  Plain C++: no HIP header is needed, so the
// mapping is tested with the host compiler alone (tests/test_variant_dispatch.py).
#pragma once
#include "rt_device_types.h"

namespace rtdev {

template <template <int, bool, bool, bool> class V, int PRIMS, bool BVH, class F>
auto dispatch_features(bool textured, bool specular, F &f) {
    if (textured) return specular ? f(V<PRIMS, true, true, BVH>()) : f(V<PRIMS, true, false, BVH>());
    return specular ? f(V<PRIMS, false, true, BVH>()) : f(V<PRIMS, false, false, BVH>());
}

// Kernels that exist for PRIMS_ANY only (the extended-light NEE kernels: a box or a wrapper forces that class, and
// its linear loop takes every kind of a rects-only or spheres-only table too): the tree's or the linear loop's
// <PRIMS_ANY, t, s, bvh>.
template <template <int, bool, bool, bool> class V, class F>
auto dispatch_any_variant(bool textured, bool specular, bool bvh, F f) {
    if (bvh) return dispatch_features<V, PRIMS_ANY, true>(textured, specular, f);
    return dispatch_features<V, PRIMS_ANY, false>(textured, specular, f);
}

// f(V<P, T, S, B>()) for the variant the flags select: with `bvh` the tree's <PRIMS_ANY, t, s, true>, whatever the class;
// otherwise the linear loop of the scene's class, any value other than PRIMS_RECTS / PRIMS_SPHERES being PRIMS_ANY.
// f is a generic callable (`[](auto v) { return decltype(v)::...; }`) with one return type for every variant.
template <template <int, bool, bool, bool> class V, class F>
auto dispatch_variant(int prims_class, bool textured, bool specular, bool bvh, F f) {
    if (bvh) return dispatch_features<V, PRIMS_ANY, true>(textured, specular, f);
    if (prims_class == PRIMS_RECTS) return dispatch_features<V, PRIMS_RECTS, false>(textured, specular, f);
    if (prims_class == PRIMS_SPHERES) return dispatch_features<V, PRIMS_SPHERES, false>(textured, specular, f);
    return dispatch_features<V, PRIMS_ANY, false>(textured, specular, f);
}

// Blocks of a launch that gives every 16x16 pixels of width x owned_rows (args.strip_*: the whole frame without strips) one
// block of 256 threads, as k_trace_f64 and the whole-frame NEE kernels index them; 0: nothing to launch.
inline unsigned frame_blocks(const TraceArgs &args) {
    const int tiles_x = (args.width + 15) / 16;
    const int tiles_y = (args.owned_rows + 15) / 16;
    return tiles_x <= 0 || tiles_y <= 0 ? 0u : (unsigned)(tiles_x * tiles_y);
}

} // namespace rtdev
