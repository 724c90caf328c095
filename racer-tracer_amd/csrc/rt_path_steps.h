// rt_path_steps.h — the per-lane steps of the per-pixel path tracers, each stated ONCE: the pixel's jitter, the primary ray,
// the closest hit, the background, the Metal and Dielectric arms, the wave's statistics and the owned-row map.  k_trace_f64
// (rt_trace_kernel.hip), nee_samples (rt_nee_common.h) and its three bodies (rt_nee_frame.h, rt_nee_pass.h,
// rt_nee_stream.h) and k_guides_f64 (rt_denoise.hip) inline them; the loops around them — what a sample is, when a path
// ends, the Lambertian and DiffuseLight vertices, the shadow ray — stay with their kernels.  Plain functions only: a step
// owns no state of the path (the caller keeps T, o, eligible and ended).  The pooled kernel (rt_trace_pool_kernel.hip,
// rt_pool_*.h) states its steps wave-wide and does not come here.
#pragma once
#include "rt_trace_common.h"

namespace RT_KNS {

// cpu.rs:35-36: one horizontal jitter per pixel.  Returns the pixel's u (rng.pixel names the pixel; rng.sample is overwritten).
__device__ __forceinline__ double pixel_jitter(PathRng &rng, int px, int width) {
    rng.sample = RT_RNG_SAMPLE_PIXEL;
    const u4 bj = rng.block(0, RT_RNG_PIXEL, 0);
    return ((double)px + u53(bj.a, bj.b)) / (double)(width - 1);
}

// cpu.rs:39-40 + camera.rs:326-337: the primary ray of sample s of the pixel in image row py with horizontal coordinate u;
// rng.sample becomes s.  (Returned by value: with o, d and the time as reference arguments the plain-colour NEE kernels
// take 2 to 6 VGPRs more and leave their occupancy step, LABNOTES 16.)
struct PrimaryRay {
    d3 o, d;
    double time; // ray.rs:26-28; scattered rays inherit it
};
__device__ __forceinline__ PrimaryRay primary_ray(const TraceArgs &A, PathRng &rng, int s, int py, double u) {
    rng.sample = (uint32_t)s;
    const u4 bc = rng.block(0, RT_RNG_CAMERA, 0);
    const double v = ((double)py + u53(bc.a, bc.b)) / (double)(A.height - 1);
    d3 offset = mk(0.0, 0.0, 0.0);
    if (A.cam.lens_radius != 0.0) { // aperture 0: the disk is multiplied by 0 -> skip its draws
        double rx, ry;
        for (uint32_t i = 0;; ++i) { // util.rs:25-39
            const u4 b = rng.block(0, RT_RNG_LENS, i);
            rx = sym53(b.a, b.b);
            ry = sym53(b.c, b.d);
            if (rx * rx + ry * ry >= 1.0) continue;
            break;
        }
        rx *= A.cam.lens_radius;
        ry *= A.cam.lens_radius;
        offset = ld3(A.cam.right) * rx + ld3(A.cam.up) * ry;
    }
    const d3 co = ld3(A.cam.origin);
    PrimaryRay r;
    r.o = co + offset;
    r.d = ld3(A.cam.ulc) + u * ld3(A.cam.horizontal) - v * ld3(A.cam.vertical) - co - offset;
    r.time = A.cam.time_a + (A.cam.time_b - A.cam.time_a) * u53(bc.c, bc.d); // camera.rs:335
    return r;
}

// THE closest-hit site, t in [0.001, inf) (renderer.rs:58): through the scene's tree (then PRIMS_ANY) or the linear loop
// of the scene's class.  best < 0: a miss.  (k_trace_f64 and k_guides_f64 call it; nee_samples has it written out, and
// says why.)
template <int PRIMS, bool BVH>
__device__ __forceinline__ void closest_hit(const TraceArgs &A, d3 o, d3 d, double ray_time, double &best_t, int &best, int &best_aux) {
    best_t = __builtin_inf();
    best = -1;
    best_aux = 0;
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
}

// background_color.rs:27-33 / :45-48: what a ray along d that hits nothing sees
__device__ __forceinline__ d3 background_colour(const TraceArgs &A, d3 d) {
    d3 bgc = ld3(A.bg.top);
    if (A.bg.kind == RT_BG_SKY) {
        const double t = 0.5 * (unit_fast(d).y + 1.0);
        bgc = (1.0 - t) * ld3(A.bg.top) + t * ld3(A.bg.bottom);
    }
    return bgc;
}

// metal.rs:26-43: the direction a ray along d leaves the hit with, mirrored and fuzzed.  The caller ends the path with nothing
// when it points into the surface (dot(dir, h.normal) < 0): with that test in here the compiler contracts two dot products
// of the fast <PRIMS_ANY, TEXTURED, SPECULAR, BVH> NEE kernels the other way round and their frames lose the last bit
// (LABNOTES 16).
__device__ __forceinline__ d3 metal_scatter(const Material &M, const Hit &h, d3 d, const PathRng &rng, uint32_t seg) {
    const d3 ud = unit_fast(d);
    d3 dir = ud - (2.0 * dot(ud, h.normal)) * h.normal;
    if (M.fuzz != 0.0) dir = dir + M.fuzz * random_in_unit_sphere(rng, seg);
    return dir;
}

// dialectric.rs:25-55: the direction a ray along d leaves the hit with, reflected or refracted
__device__ __forceinline__ d3 dielectric_scatter(const Material &M, const Hit &h, d3 d, const PathRng &rng, uint32_t seg) {
    const double ratio = h.front ? 1.0 / M.ior : M.ior;
    const d3 ud = unit_fast(d);
    const double cos_theta = fmin(dot(-ud, h.normal), 1.0);
    const double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
    bool reflect_it = ratio * sin_theta > 1.0;
#ifdef RT_EXACT_DIV
    // RT_ARITH_REFERENCE forms the Fresnel term on every lane, not under `if (!reflect_it)` (the draw is addressed, so an
    // unused one changes nothing).  With the nested branch the compiler's code for the <PRIMS_RECTS, plain, SPECULAR> NEE
    // kernels lost the caller's `o = h.point` on the lanes that reflect by the draw: LABNOTES 10 has the instructions;
    // tests/test_gpu_nee.py holds every variant to the oracle.
    const bool total_reflection = reflect_it;
    {
#else
    if (!reflect_it) { // the draw happens only when refraction is possible
#endif
        double r0 = (1.0 - ratio) / (1.0 + ratio);
        r0 = r0 * r0;
        const double m = 1.0 - cos_theta;
        const double m2 = m * m;
        const double refl = r0 + (1.0 - r0) * (m2 * m2 * m);
        const u4 b = rng.block(seg, RT_RNG_DIELECTRIC, 0);
        reflect_it = refl > u53(b.a, b.b);
    }
#ifdef RT_EXACT_DIV
    reflect_it = reflect_it || total_reflection;
#endif
    d3 dir;
    if (reflect_it) {
        dir = ud - (2.0 * dot(ud, h.normal)) * h.normal;
    } else { // vec3.rs:416-422
        const d3 perp = ratio * (ud + cos_theta * h.normal);
        dir = perp + (-sqrt(fabs(1.0 - len2(perp)))) * h.normal;
    }
    return dir;
}

// One atomic per wave for a statistic: the wave's sum of a per-lane count, added by lane 0 to A.segments[slot] (RT_STAT_*)
// when it is not zero.  lane: the caller's threadIdx.x & 63.
__device__ __forceinline__ void wave_stat_add(const TraceArgs &A, int lane, int slot, unsigned int count) {
    unsigned long long total = count;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
    if (lane == 0 && total) atomicAdd(A.segments + slot, total);
}

// Owned row -> image row: with strips (several GPUs) a launch covers only its rank's rows, compacted.  K: the kernel's
// copy of its arguments, or kernargs_here() where the strip fields are to be read next to this one use.
template <class ARGS> __device__ __forceinline__ int image_row(const ARGS *K, int vrow) {
    int py = vrow;
    if (K->strip_count > 1) py = ((vrow / K->strip_rows) * K->strip_count + K->strip_index) * K->strip_rows + vrow % K->strip_rows;
    return py;
}

} // namespace RT_KNS
