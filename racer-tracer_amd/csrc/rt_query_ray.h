// rt_query_ray.h — what the three ray queries (rt_rays_kernel.hip, rt_occlusion_kernel.hip, rt_multihit_kernel.hip) do
// with a ray the caller brings before any hit code sees it: the validity rule, once, and a power-of-two normalisation of
// the direction.  (rt_ambient_kernel.hip judges its points by the same rule and scales their normals by the same factor.)
//
// Why the direction is normalised.  "The direction has any length and t is in units of it" (include/rt_rays.h), but the
// tree walks cull in single precision with 1 / d clamped to +-2^64 (rt_bvh_slab.h: slab_finite — the clamp is there for
// axis-parallel rays).  A direction whose components are all below 2^-64 has all three reciprocals clamped: the f32 walk
// then follows the diagonal (+-1, +-1, +-1) instead of the ray and culls real hits, and beyond 2^+-126 the f32 window
// ends (tmin_f, far_of) underflow or overflow as well.  The render kernels never meet such a ray; a caller's segment
// (a, b - a) between two close points is one.
//
// The rule.  E = the binary exponent of the largest |component| of d.  Inside the band |E| <= RAY_BAND the ray is walked
// as it is (both factors are 1.0, every product below is exact: today's arithmetic, bit for bit).  Outside it the walk
// sees d * 2^-E, whose largest component lies in [1, 2), and the window [t_min, t_max] * 2^E; a reported t' is handed
// back as t' * 2^-E.  Every factor is a power of two, so each product is exact unless it leaves the range of a double:
// the hit code works on the same significands at every scale.  A window end that overflows to inf or underflows to 0
// under the scaling behaves as that value does.  E is clamped to +-1022 so that 2^E and 2^-E are both normal numbers
// (a direction of subnormal components is scaled by 2^1022 and no further).
//
// Plain C++ down to the last section: the host compiles it too (tests/query_ray_driver.cpp).  The last section, for the
// kernels alone, is the prologue itself in the device's own types.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RT_QRAY_FN __host__ __device__ inline
#else
#define RT_QRAY_FN inline
#endif

namespace rt_query {

enum : int { RAY_BAND = 32, RAY_E_MAX = 1022 };

// Decided before any hit code runs.  Every comparison is false on a NaN: a NaN anywhere but t_max fails `< inf` or
// `>= 0`, a NaN t_max fails `t_max >= t_min`.  t_max = +inf is the open window.
RT_QRAY_FN bool ray_valid(double ox, double oy, double oz, double dx, double dy, double dz, double time, double t_min, double t_max) {
    const double INF = __builtin_inf();
    return fabs(ox) < INF && fabs(oy) < INF && fabs(oz) < INF && fabs(dx) < INF && fabs(dy) < INF && fabs(dz) < INF &&
           fabs(time) < INF && t_min >= 0.0 && t_min < INF && t_max >= t_min && (dx != 0.0 || dy != 0.0 || dz != 0.0);
}

// The unbiased binary exponent field of |x|: floor(log2 |x|) for a normal x, -1023 for 0 and subnormals, 1024 for inf / NaN.
RT_QRAY_FN int exponent_of(double x) {
    uint64_t bits;
    memcpy(&bits, &x, sizeof bits);
    return (int)((bits >> 52) & 0x7ffu) - 1023;
}

// 2^k for -1022 <= k <= 1023, from its bits (no libm call, no rounding).
RT_QRAY_FN double pow2_of(int k) {
    const uint64_t bits = (uint64_t)(k + 1023) << 52;
    double x;
    memcpy(&x, &bits, sizeof x);
    return x;
}

// The exponent the ray is normalised by: 0 inside the band.  (An invalid ray gets some exponent and is never walked.)
RT_QRAY_FN int ray_exponent(double dx, double dy, double dz) {
    const int e = exponent_of(fmax(fmax(fabs(dx), fabs(dy)), fabs(dz)));
    if (e >= -RAY_BAND && e <= RAY_BAND) return 0;
    return e < -RAY_E_MAX ? -RAY_E_MAX : (e > RAY_E_MAX ? RAY_E_MAX : e);
}

struct RayScale {
    double down; // 2^-E: times the caller's direction = the walked direction; times a walked t = the caller's t
    double up;   // 2^E: times the caller's window = the walked window
};

RT_QRAY_FN RayScale ray_scale(double dx, double dy, double dz) {
    const int e = ray_exponent(dx, dy, dz);
    return RayScale{pow2_of(-e), pow2_of(e)};
}

} // namespace rt_query

#if defined(__HIPCC__) && defined(RT_KNS)
// ---- the kernels' prologue (after rt_trace_common.h and rt_scene.h): ray r of the caller's planes, judged and normalised
namespace RT_KNS {

struct QueryRay {
    d3 o;           // the caller's origin
    d3 dn;          // the walked direction, d * 2^-E
    double time;
    double lo, hi;  // the walked window, [t_min, t_max] * 2^E
    bool valid;
};

// A NULL optional plane of R is the default of every ray.
__device__ __forceinline__ QueryRay load_query_ray(const RtRays &R, size_t r) {
    QueryRay q;
    q.o = ld3(R.origin + 3 * r);
    const d3 d = ld3(R.direction + 3 * r);
    const double t_min = R.t_min ? R.t_min[r] : 0.001; // renderer.rs:58
    const double t_max = R.t_max ? R.t_max[r] : __builtin_inf();
    q.time = R.time ? R.time[r] : 0.0;
    q.valid = rt_query::ray_valid(q.o.x, q.o.y, q.o.z, d.x, d.y, d.z, q.time, t_min, t_max);
    const rt_query::RayScale s = rt_query::ray_scale(d.x, d.y, d.z);
    q.dn = d * s.down;
    q.lo = t_min * s.up;
    q.hi = t_max * s.up;
    return q;
}

// Behind the walk, for a hit's record: the caller's own direction, READ AGAIN — kept in registers beside dn through the
// walk it cost the k = 8 tree kernel 8 VGPRs (124 -> 132, past the 128 that four waves per SIMD allow: 15 % of its time
// on 1920 x 1080 rays) — and a walked t in its units.  (volatile: the compiler may not reuse the prologue's load;
// tests/test_query_rays_cpu.py pins the kernel's VGPR count, so a compiler that keeps d after all is noticed.)  The plane is
// read twice, and caller_t forms the scale from the second read: the caller's planes must not change while a launch is in
// flight (include/rt_rays.h says so).
__device__ __forceinline__ d3 caller_direction(const RtRays &R, size_t r) {
    const volatile double *p = R.direction + 3 * r;
    return d3{p[0], p[1], p[2]};
}
__device__ __forceinline__ double caller_t(d3 d, double t_walked) { return t_walked * rt_query::ray_scale(d.x, d.y, d.z).down; }

} // namespace RT_KNS
#endif
