// rt_nee_lights.h — the light code of rt_scene_set_lights' list ("the extended list"): the ExtendedLights policy
// of rt_nee_common.h's nee_samples.  A listed light is a Sphere, a rect or a Box, bare or inside RotateY and / or Translate,
// or a MovingSphere; light k is picked uniformly or by power (rtdev::NeeLightArgs).
//
// ONE RULE: sample and pdf are both computed in the light's OBJECT FRAME from (x_o, w_o) alone, x_o = rot_fwd(x - tr) —
// Translate is the outer wrapper, RotateY the inner one, as in prim_t — and a world direction is rot_back(w_o).  Rigid
// motions keep solid-angle densities, so the object-frame density is the world's.  The recorded hit point is never read.
//
// Both halves are OUT OF LINE (sphere_uv is the precedent): the TEXTURED PRIMS_ANY forms of nee_samples sit at 229-244
// VGPRs, and what stays alive in the path loop around a call is what it is with PlainLights: w, the weight, the target.
#pragma once
#include "rt_nee_common.h"

namespace RT_KNS {

// The six sides of a Boxx in box_side order and their areas: sides 0, 1 span (x, y), 2, 3 (x, z), 4, 5 (y, z).
__device__ __forceinline__ double box_light_area(const Prim &L, double &a_xy, double &a_xz, double &a_yz) {
    const double ex = fabs(L.p[3] - L.p[0]), ey = fabs(L.p[4] - L.p[1]), ez = fabs(L.p[5] - L.p[2]);
    a_xy = ex * ey;
    a_xz = ex * ez;
    a_yz = ey * ez;
    return 2.0 * (a_xy + a_yz + a_xz);
}

// Density of the direction wo from xo for a point uniform on the box's surface: the shadow ray may meet the box on a
// nearer side than the sampled one and that hit is taken, so every side the half-line xo + t wo, t > 0, crosses counts:
// p_k / A_tot * sum t^2 / |w_axis| (two sides from outside, one from inside).  A side the line runs parallel to gives
// t = +-inf or NaN and an in-plane point that fails every comparison.
__device__ __forceinline__ double box_light_pdf(const Prim &L, d3 xo, d3 wo, double p_k) {
    double a_xy, a_xz, a_yz;
    const double a_tot = box_light_area(L, a_xy, a_xz, a_yz);
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        int axis;
        double a0, a1, b0, b1, k;
        box_side(L.p, s, axis, a0, a1, b0, b1, k);
        const int ia = axis == 0 ? 1 : 0, ib = axis == 2 ? 1 : 2;
        const double wa = comp(wo, axis);
        const double t = (k - comp(xo, axis)) / wa;
        const double a = comp(xo, ia) + t * comp(wo, ia), b = comp(xo, ib) + t * comp(wo, ib);
        if (t > 0.0 && a >= a0 && a <= a1 && b >= b0 && b <= b1) sum += t * t / fabs(wa);
    }
    return p_k / a_tot * sum;
}

struct LightSample {
    double wx, wy, wz, p; // the WORLD direction and its density (0: no sample)
};

// A sample of light L from the world point x.  `face`: the box's face draw (block 1 of RT_RNG_LIGHT, include/rt_rng.h);
// time: the path's ray time (MovingSphere).  A MovingSphere's record keeps its motion where the wrappers' fields are
// (rt_plan.cpp: pack_prims) and cannot be wrapped.
__device__ __noinline__ LightSample extended_light_sample(const Prim *Lp, double x0, double x1, double x2, double e1, double e2,
                                                          double face, double p_k, double time) {
    const Prim &L = *Lp;
    const int kind = L.kind;
    const int flags = kind == RT_PRIM_MOVING_SPHERE ? 0 : L.flags;
    d3 xo = mk(x0, x1, x2);
    if (flags & RT_PRIM_HAS_TRANSLATE) xo = xo - ld3(L.tr);
    if (flags & RT_PRIM_HAS_ROTATE_Y) xo = rot_fwd(xo, L.rot_sin, L.rot_cos);
    d3 wo = mk(0.0, 0.0, 0.0);
    double p = 0.0;
    if (kind == RT_PRIM_SPHERE || kind == RT_PRIM_MOVING_SPHERE) {
        d3 center = ld3(L.p);
        if (kind == RT_PRIM_MOVING_SPHERE) center = center + ((time - L.rot_sin) * L.rot_cos) * ld3(L.tr); // moving_sphere.rs:37-39
        p = sample_sphere_light(center, L.radius2, xo, e1, e2, p_k, wo);
    } else if (kind == RT_PRIM_BOX) {
        double a_xy, a_xz, a_yz;
        const double target = face * box_light_area(L, a_xy, a_xz, a_yz);
        // the first side whose running area exceeds the target, else side 5
        const double c0 = a_xy, c1 = c0 + a_xy, c2 = c1 + a_xz, c3 = c2 + a_xz, c4 = c3 + a_yz;
        const int s = target < c0 ? 0 : (target < c1 ? 1 : (target < c2 ? 2 : (target < c3 ? 3 : (target < c4 ? 4 : 5))));
        int axis;
        double a0, a1, b0, b1, k;
        box_side(L.p, s, axis, a0, a1, b0, b1, k);
        const double ca = a0 + (a1 - a0) * e1, cb = b0 + (b1 - b0) * e2;
        const d3 y = axis == 2 ? mk(ca, cb, k) : (axis == 1 ? mk(ca, k, cb) : mk(k, ca, cb));
        const d3 v = y - xo;
        const double dist2 = len2(v);
        if (dist2 > 0.0) {
            wo = v * (1.0 / sqrt(dist2));
            p = box_light_pdf(L, xo, wo, p_k);
        }
    } else {
        const int axis = kind == RT_PRIM_XY_RECT ? 2 : (kind == RT_PRIM_XZ_RECT ? 1 : 0);
        p = sample_rect_light(axis, L.p[0], L.p[1], L.p[2], L.p[3], L.p[4], xo, e1, e2, p_k, wo);
    }
    if (!(p > 0.0)) return LightSample{0.0, 0.0, 0.0, 0.0};
    if (flags & RT_PRIM_HAS_ROTATE_Y) wo = rot_back(wo, L.rot_sin, L.rot_cos);
    return LightSample{wo.x, wo.y, wo.z, p};
}

// Density the light sampler has for the unit WORLD direction w from x, which a bounce ray found light L along.
__device__ __noinline__ double extended_light_pdf(const Prim *Lp, double x0, double x1, double x2, double w0, double w1, double w2,
                                                  double p_k, double time) {
    const Prim &L = *Lp;
    const int kind = L.kind;
    const int flags = kind == RT_PRIM_MOVING_SPHERE ? 0 : L.flags;
    d3 xo = mk(x0, x1, x2), wo = mk(w0, w1, w2);
    if (flags & RT_PRIM_HAS_TRANSLATE) xo = xo - ld3(L.tr);
    if (flags & RT_PRIM_HAS_ROTATE_Y) {
        xo = rot_fwd(xo, L.rot_sin, L.rot_cos);
        wo = rot_fwd(wo, L.rot_sin, L.rot_cos);
    }
    if (kind == RT_PRIM_SPHERE || kind == RT_PRIM_MOVING_SPHERE) {
        d3 center = ld3(L.p);
        if (kind == RT_PRIM_MOVING_SPHERE) center = center + ((time - L.rot_sin) * L.rot_cos) * ld3(L.tr);
        return sphere_light_pdf(center, L.radius2, xo, p_k);
    }
    if (kind == RT_PRIM_BOX) return box_light_pdf(L, xo, wo, p_k);
    const int axis = kind == RT_PRIM_XY_RECT ? 2 : (kind == RT_PRIM_XZ_RECT ? 1 : 0);
    const double wa = comp(wo, axis);
    const double t = (L.p[4] - comp(xo, axis)) / wa;
    const double area = fabs((L.p[1] - L.p[0]) * (L.p[3] - L.p[2]));
    return p_k * (t * t) / (fabs(wa) * area); // (inf when grazing)
}

struct ExtendedLights {
    typedef NeeLightArgs Args;
    // k: uniform as PlainLights, or the first index with e0 < cdf[k] — the number of running sums at or below e0, at most
    // n - 1 of them (cdf[n - 1] = 1 > e0); the sums are read with a wave-uniform index
    static __device__ __forceinline__ void pick(const NeeArgs &N, const Args &X, double e0, double p_uniform, int &k, double &p_k) {
        if (X.pick == RT_PICK_UNIFORM) {
            PlainLights::pick(N, NoLightArgs(), e0, p_uniform, k, p_k);
            return;
        }
        const RT_CONSTANT double *cdf = (const RT_CONSTANT double *)X.cdf;
        k = 0;
        for (int j = 0; j + 1 < N.n_lights; ++j) k += e0 >= cdf[j] ? 1 : 0;
        p_k = X.p[k];
    }
    static __device__ __forceinline__ double sample(const Prim &L, d3 x, double e1, double e2, double p_k, const PathRng &rng,
                                                    uint32_t seg, double time, d3 &w) {
        double face = 0.0;
        if (L.kind == RT_PRIM_BOX) { // one more addressed draw: block 1 of RT_RNG_LIGHT, its first 53-bit draw
            const u4 bf = rng.block(seg, RT_RNG_LIGHT, 1);
            face = u53(bf.a, bf.b);
        }
        const LightSample ls = extended_light_sample(&L, x.x, x.y, x.z, e1, e2, face, p_k, time);
        w = mk(ls.wx, ls.wy, ls.wz);
        return ls.p;
    }
    static __device__ __forceinline__ double pdf(const Args &X, const Prim &L, int k, d3 x, d3, d3 w, double time, double p_uniform) {
        const double p_k = X.pick == RT_PICK_UNIFORM ? p_uniform : X.p[k];
        return extended_light_pdf(&L, x.x, x.y, x.z, w.x, w.y, w.z, p_k, time);
    }
};

} // namespace RT_KNS
