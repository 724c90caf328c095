// rt_nee_common.h — the ONE statement of the next-event estimator: the light-sampling helpers and the
// per-pixel sample loop that k_nee_f64 (rt_nee_kernel.hip: a whole frame in one launch) and k_nee_pass_f64
// (rt_nee_pass_kernel.hip: listed tiles, a range of samples on top of a carried-in sum) both inline.  The loop adds a
// pixel's samples to `sum` in sample order and every draw is addressed by (pixel, sample, ...), so what a sample adds does
// not depend on the launch it is traced in: the passes' sums are the one-shot launch's, bit for bit.  The loop's light
// code — the pick, the sample, the pdf of a bounce direction — is a policy: PlainLights below, the list rt_scene_create
// makes, and ExtendedLights (rt_nee_lights.h), the list of rt_scene_set_lights.
#pragma once
#include "rt_path_steps.h"

namespace RT_KNS {

// p^beta / (p^beta + q^beta) for pdfs p, q >= 0 (q may be inf: a grazing rect); 0 when p = 0
__device__ __forceinline__ double mis_weight(double p, double q, int heuristic) {
    if (heuristic == 0) {
        p *= p;
        q *= q;
    }
    return p > 0.0 ? p / (p + q) : 0.0;
}

// Solid-angle pdf of light L (a plain Sphere or an untransformed rect) from x toward the point y it was hit at, along
// the unit direction w: rect: p_pick |y - x|^2 / (|n_L . w| A) (inf when grazing); sphere: p_pick / (2 pi (1 - cos_max)),
// 0 from inside.
// (the sphere's part on its own: the extended lights of rt_nee_lights.h evaluate it around other centres)
__device__ __forceinline__ double sphere_light_pdf(d3 center, double radius2, d3 x, double p_pick) {
    const double PI = 3.14159265358979323846;
    const double dc2 = len2(center - x);
    if (dc2 <= radius2) return 0.0;
    const double cos_max = sqrt(fmax(0.0, 1.0 - radius2 / dc2));
    return p_pick / (2.0 * PI * (1.0 - cos_max));
}
__device__ __forceinline__ double light_pdf(const Prim &L, d3 x, d3 y, d3 w, double p_pick) {
    if (L.kind == RT_PRIM_SPHERE) return sphere_light_pdf(ld3(L.p), L.radius2, x, p_pick);
    const int axis = L.kind == RT_PRIM_XY_RECT ? 2 : (L.kind == RT_PRIM_XZ_RECT ? 1 : 0);
    const double area = fabs((L.p[1] - L.p[0]) * (L.p[3] - L.p[2]));
    return p_pick * len2(y - x) / (fabs(comp(w, axis)) * area);
}

// A light sample from x: the unit direction toward the sampled point and its solid-angle pdf (0: no sample).  The sphere's
// and the rect's parts stand on their own: the extended lights of rt_nee_lights.h take them in a light's object frame.
__device__ __forceinline__ double sample_sphere_light(d3 center, double radius2, d3 x, double e1, double e2, double p_pick, d3 &w) {
    const double PI = 3.14159265358979323846;
    // uniform in the cone the sphere subtends
    const d3 cx = center - x;
    const double dc2 = len2(cx);
    if (dc2 <= radius2) return 0.0; // from inside: no sample
    const double cos_max = sqrt(fmax(0.0, 1.0 - radius2 / dc2));
    const double one_m = 1.0 - cos_max;
    if (!(one_m > 0.0)) return 0.0;
    const double cos_t = 1.0 - e1 * one_m;
    const double sin_t = sqrt(fmax(0.0, 1.0 - cos_t * cos_t));
    const double phi = 2.0 * PI * e2;
    const d3 z = cx * (1.0 / sqrt(dc2));
    // Duff et al. 2017, "Building an orthonormal basis, revisited"
    const double sign = copysign(1.0, z.z);
    const double a = -1.0 / (sign + z.z);
    const double b = z.x * z.y * a;
    const d3 b1 = mk(1.0 + sign * z.x * z.x * a, sign * b, -sign * z.x);
    const d3 b2 = mk(b, sign + z.y * z.y * a, -z.y);
    // (sin_lean: the library's sin / cos carry a Payne-Hanek path that costs scratch memory; phi is in [0, 2 pi))
    w = (sin_t * sin_lean(phi + 0.5 * PI)) * b1 + (sin_t * sin_lean(phi)) * b2 + cos_t * z;
    return p_pick / (2.0 * PI * one_m);
}
// (axis: the rect's constant axis, at k; [a0, a1] x [b0, b1] on the two others in order)
__device__ __forceinline__ double sample_rect_light(int axis, double a0, double a1, double b0, double b1, double k, d3 x, double e1,
                                                    double e2, double p_pick, d3 &w) {
    const double ca = a0 + (a1 - a0) * e1, cb = b0 + (b1 - b0) * e2;
    const d3 y = axis == 2 ? mk(ca, cb, k) : (axis == 1 ? mk(ca, k, cb) : mk(k, ca, cb));
    const d3 v = y - x;
    const double dist2 = len2(v);
    w = v * (1.0 / sqrt(dist2));
    const double area = fabs((a1 - a0) * (b1 - b0));
    const double g = fabs(comp(w, axis)) * area;
    if (!(g > 0.0) || !(dist2 > 0.0)) return 0.0; // grazing: nothing
    return p_pick * dist2 / g;
}
__device__ __forceinline__ double sample_light(const Prim &L, d3 x, double e1, double e2, double p_pick, d3 &w) {
    if (L.kind == RT_PRIM_SPHERE) return sample_sphere_light(ld3(L.p), L.radius2, x, e1, e2, p_pick, w);
    const int axis = L.kind == RT_PRIM_XY_RECT ? 2 : (L.kind == RT_PRIM_XZ_RECT ? 1 : 0);
    return sample_rect_light(axis, L.p[0], L.p[1], L.p[2], L.p[3], L.p[4], x, e1, e2, p_pick, w);
}

// THE LIGHT CODE of nee_samples, a policy: how light k is picked from the draw e0, sampled from a vertex, and what density
// the light sampler has for a bounce direction that found a listed light.  PlainLights is the code of rt_render_frame_nee
// since its first day — unwrapped spheres and rects, a uniform pick — and the default; ExtendedLights (rt_nee_lights.h)
// is rt_scene_set_lights' list.  X: the policy's own argument block, p_uniform: 1 / n_lights.
struct NoLightArgs {};
struct PlainLights {
    typedef NoLightArgs Args;
    static __device__ __forceinline__ void pick(const NeeArgs &N, const Args &, double e0, double p_uniform, int &k, double &p_k) {
        k = (int)floor(e0 * (double)N.n_lights);
        if (k > N.n_lights - 1) k = N.n_lights - 1;
        p_k = p_uniform;
    }
    static __device__ __forceinline__ double sample(const Prim &L, d3 x, double e1, double e2, double p_k, const PathRng &, uint32_t,
                                                    double, d3 &w) {
        return sample_light(L, x, e1, e2, p_k, w);
    }
    static __device__ __forceinline__ double pdf(const Args &, const Prim &L, int, d3 x, d3 y, d3 w, double, double p_uniform) {
        return light_pdf(L, x, y, w, p_uniform);
    }
};

// Samples [s_begin, s_end) of pixel (px, py) added to `sum` in sample order (s_begin == s_end: none, the lane idles through
// the wave's loop).  u: the pixel's horizontal coordinate (cpu.rs:35-36).  n_segments / n_started: path segments (shadow
// rays excluded) and primary rays, added to.
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH, class LIGHTS = PlainLights>
__device__ __forceinline__ void nee_samples(const TraceArgs &A, const NeeArgs &N, PathRng &rng, int px, int py, double u, int s_begin,
                                            int s_end, d3 &sum, unsigned int &n_segments, unsigned int &n_started,
                                            const typename LIGHTS::Args &X = typename LIGHTS::Args()) {
    const double INV_PI = 0.31830988618379067154;
    const double p_pick = N.n_lights > 0 ? 1.0 / (double)N.n_lights : 0.0;

    const d3 zero = mk(0.0, 0.0, 0.0);
    d3 acc = zero; // the radiance of the sample in flight
    d3 o = zero, d = zero, T = zero;
    int s = s_begin;
    uint32_t seg = 0;
    double ray_time = 0.0;
    bool alive = false;
    // SHADOW RAY pending (o, d are the shadow ray): its target light, its weight cos_x / pi / p_l * w_l, and the bounce
    // direction the path continues with from o afterwards
    bool shadow = false;
    int target = -1;
    double nee_w = 0.0;
    d3 bounce = zero;
    // the path's last vertex was an NEE-eligible Lambertian one: its point and n . d^ of the bounce (for w_b)
    bool eligible = false;
    d3 x_prev = zero;
    double cos_b = 0.0;

    while (s < s_end) {
        if (!alive) {
            ++n_started;
            const PrimaryRay r = primary_ray(A, rng, s, py, u);
            o = r.o;
            d = r.d;
            ray_time = r.time;
            T = mk(1.0, 1.0, 1.0);
            acc = mk(0.0, 0.0, 0.0);
            seg = 0;
            eligible = false;
            alive = true;
        }

        d3 contrib = mk(0.0, 0.0, 0.0); // what is added to the sample's radiance when it ends here
        bool ended = false;
        if (A.max_depth <= 0) { // renderer.rs:48-55 with max_depth 0: white, nothing traced
            contrib = T;
            ended = true;
        } else {
            if (!shadow) ++n_segments;
            // THE closest-hit site, t in [0.001, inf) (renderer.rs:58): a path segment or a shadow ray.  rt_path_steps.h's
            // closest_hit, written out: as a call the linear loop is optimised on its own first and the register counts move
            // by two, which takes exact <PRIMS_RECTS, plain, SPECULAR> out of the pair tests/test_nee_stream_isa.py pins.
            double best_t = __builtin_inf();
            int best = -1, best_aux = 0;
            const d3 inv_d = rcp3(d);
            const double inv_a = PRIMS == PRIMS_RECTS ? 0.0 : rcp_f64(len2(d));
            if (BVH) {
                closest_hit_bvh<PRIMS_ANY>(A, bvh_nodes_for(A, d), o, d, inv_d, inv_a, ray_time, 0.001, best_t, best, best_aux);
            } else {
                for (int i = 0; i < A.n_prims; ++i) {
                    double t;
                    int aux;
                    if (prim_t<PRIMS>(load_prim_uniform(A.prims, i), o, d, inv_d, inv_a, ray_time, 0.001, best_t, t, aux)) {
                        best_t = t;
                        best = i;
                        best_aux = aux;
                    }
                }
            }
            if (shadow) { // the light is visible iff the closest primitive is the sampled one; Le at that hit
                if (best == target) {
                    const Prim &P = A.prims[best];
                    const Hit h = prim_hit_record<PRIMS, TEXTURED>(P, o, d, ray_time, best_t, best_aux, P.mat.needs_uv != 0);
                    acc = acc + (T * texture_value<TEXTURED>(A, nullptr, A.textures, P.mat, h.u, h.v, h.point)) * nee_w;
                }
                shadow = false;
                d = bounce; // the path goes on from the same vertex
            } else if (best < 0) {
                contrib = T * background_colour(A, d);
                ended = true;
            } else {
                const Prim &P = A.prims[best];
                const Material &M = P.mat;
                const Hit h = prim_hit_record<PRIMS, TEXTURED>(P, o, d, ray_time, best_t, best_aux, M.needs_uv != 0);
                if (M.kind == RT_MAT_DIFFUSE_LIGHT) { // diffuse_light.rs:25-37
                    contrib = T * texture_value<TEXTURED>(A, nullptr, A.textures, M, h.u, h.v, h.point);
                    const int k = N.slot[best];
                    if (eligible && k >= 0 && k < N.n_lights) { // a listed light found by the bounce of an NEE vertex
                        const double inv_len = rsqrt_f64(len2(d));
                        const double p_l = LIGHTS::pdf(X, P, k, x_prev, h.point, d * inv_len, ray_time, p_pick);
                        contrib = contrib * mis_weight(cos_b * INV_PI, p_l, N.heuristic);
                    }
                    ended = true;
                } else if (M.kind == RT_MAT_LAMBERTIAN) { // lambertian.rs:26-38
                    d3 dir = h.normal + unit_fast(random_in_unit_sphere(rng, seg));
                    if (fabs(dir.x) < 1e-8 && fabs(dir.y) < 1e-8 && fabs(dir.z) < 1e-8) dir = h.normal;
                    T = T * texture_value<TEXTURED>(A, nullptr, A.textures, M, h.u, h.v, h.point);
                    o = h.point;
                    d = dir;
                    eligible = N.n_lights > 0 && (int)seg + 1 < A.max_depth; // the child ray is really traced
                    if (eligible) {
                        x_prev = h.point;
                        cos_b = dot(h.normal, dir) * rsqrt_f64(len2(dir));
                        // the light sample: RT_RNG_LIGHT, three 42-bit draws packed as RT_RNG_SCATTER packs them
                        const u4 bl = rng.block(seg, RT_RNG_LIGHT, 0);
                        const double e0 = (sym42_bits(__builtin_amdgcn_alignbit(bl.a, bl.d << 22, 12), bl.a) + 1.0) * 0.5;
                        const double e1 = (sym42(bl.b, bl.d & 0x000FFC00u) + 1.0) * 0.5;
                        const double e2 = (sym42(bl.c, (bl.d >> 10) & 0x000FFC00u) + 1.0) * 0.5;
                        int k;
                        double p_k;
                        LIGHTS::pick(N, X, e0, p_pick, k, p_k);
                        const int li = N.prim[k];
                        d3 w;
                        const double p_l = LIGHTS::sample(A.prims[li], h.point, e1, e2, p_k, rng, seg, ray_time, w);
                        const double cos_x = dot(h.normal, w);
                        if (p_l > 0.0 && cos_x > 0.0) { // trace the shadow ray next: 2 cos_x w, the bounce ray toward w
                            const double p_b = cos_x * INV_PI;
                            nee_w = p_b / p_l * mis_weight(p_l, p_b, N.heuristic);
                            target = li;
                            bounce = dir;
                            d = (2.0 * cos_x) * w;
                            shadow = true;
                        }
                    }
                } else if (SPECULAR && M.kind == RT_MAT_METAL) {
                    eligible = false;
                    const d3 dir = metal_scatter(M, h, d, rng, seg);
                    if (dot(dir, h.normal) < 0.0) { // absorbed
                        ended = true;
                    } else {
                        T = T * texture_value<TEXTURED>(A, nullptr, A.textures, M, h.u, h.v, h.point);
                        o = h.point;
                        d = dir;
                    }
                } else if (SPECULAR) {
                    eligible = false;
                    d = dielectric_scatter(M, h, d, rng, seg);
                    o = h.point;
                } else { // unreachable: the host picks SPECULAR whenever such a material exists
                    ended = true;
                }
                // renderer.rs:48-55: the recursion's next level has depth 0 -> white
                if (!ended && (int)++seg >= A.max_depth) {
                    contrib = T;
                    ended = true;
                }
            }
        }
        if (ended) {
            sum = sum + (acc + contrib); // the sample's radiance, in sample order
            ++s;
            alive = false;
        }
    }
}

} // namespace RT_KNS
