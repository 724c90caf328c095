// rt_trace_kernel.hip — v1 of the per-pixel path-tracing kernel (f64): one
// lane owns one pixel and regenerates its next sample as soon as a path ends
// (see DESIGN.md 4.2).  Kept as the simple, order-exact reference form of the
// device path (per-pixel sums in the oracle's sample order) and for A/B
// measurements against the pooled kernel of rt_trace_pool_kernel.hip, which is
// the default (its resolve pass: rt_frame_kernels.hip).  Selected with RtSceneOptions.kernel = RT_KERNEL_V1 (rt_scene_create_ex).
#include "rt_path_steps.h"
#include "rt_variant_dispatch.h"

namespace RT_KNS {

// ------------------------------------------------------------- the kernel
// 256 threads = 4 waves; each wave owns an 8x8 pixel tile, each block a
// 16x16 one.  Rows are "owned rows": with strips (multi-GPU) the launch
// covers only this rank's rows, compacted.
//
// Template flags specialise the kernel to what the scene contains (chosen on
// the host at launch), which keeps the register footprint of the common
// cases small:
//   PRIMS    : PRIMS_RECTS (untransformed rects only), PRIMS_SPHERES
//              (untransformed spheres only), PRIMS_ANY
//   TEXTURED : some material's texture is not a plain SolidColor
//   SPECULAR : some material is Metal or Dielectric
template <int PRIMS, bool TEXTURED, bool SPECULAR>
__global__ __launch_bounds__(256) void k_trace_f64(const TraceArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tiles_x = (A.width + 15) >> 4;
    const int bx = blockIdx.x % tiles_x;
    const int by = blockIdx.x / tiles_x;
    const int px = bx * 16 + (wave & 1) * 8 + (lane & 7);
    const int vrow = by * 16 + (wave >> 1) * 8 + (lane >> 3);
    const int py = image_row(&A, vrow);
    const bool in_image = px < A.width && vrow < A.owned_rows && py < A.height;

    PathRng rng;
    rng.pixel = (uint32_t)py * (uint32_t)A.width + (uint32_t)px;
    rng.k0 = A.seed_lo;
    rng.k1 = A.seed_hi;

    const double u = pixel_jitter(rng, px, A.width);

    d3 sum = mk(0.0, 0.0, 0.0);
    d3 o = sum, d = sum, T = sum;
    int s = in_image ? A.sample_begin : A.sample_end;
    uint32_t seg = 0;
    double ray_time = 0.0; // ray.rs:26-28; scattered rays inherit it
    bool alive = false;
    unsigned int n_segments = 0, n_started = 0;

    while (s < A.sample_end) {
        if (!alive) {
            ++n_started;
            const PrimaryRay r = primary_ray(A, rng, s, py, u);
            o = r.o;
            d = r.d;
            ray_time = r.time;
            T = mk(1.0, 1.0, 1.0);
            seg = 0;
            alive = true;
        }

        d3 contrib; // what this path adds to the pixel if it ends here
        bool ended;
        if (A.max_depth <= 0) { // renderer.rs:48-55 with max_depth 0: white, nothing traced
            contrib = T;
            ended = true;
        } else {
            ++n_segments;
            double best_t;
            int best, best_aux;
            closest_hit<PRIMS, false>(A, o, d, ray_time, best_t, best, best_aux);
            if (best < 0) {
                contrib = T * background_colour(A, d);
                ended = true;
            } else {
                const Prim &P = A.prims[best];
                const Material &M = P.mat;
                Hit h = prim_hit_record<PRIMS, TEXTURED>(P, o, d, ray_time, best_t, best_aux, M.needs_uv != 0);
                if (M.kind == RT_MAT_DIFFUSE_LIGHT) { // diffuse_light.rs:25-37
                    contrib = T * texture_value<TEXTURED>(A, nullptr, A.textures, M, h.u, h.v, h.point);
                    ended = true;
                } else if (M.kind == RT_MAT_LAMBERTIAN) { // lambertian.rs:26-38
                    d3 dir = h.normal + unit_fast(random_in_unit_sphere(rng, seg));
                    if (fabs(dir.x) < 1e-8 && fabs(dir.y) < 1e-8 && fabs(dir.z) < 1e-8) dir = h.normal;
                    T = T * texture_value<TEXTURED>(A, nullptr, A.textures, M, h.u, h.v, h.point);
                    o = h.point;
                    d = dir;
                    ended = false;
                } else if (SPECULAR && M.kind == RT_MAT_METAL) {
                    const d3 dir = metal_scatter(M, h, d, rng, seg);
                    if (dot(dir, h.normal) < 0.0) { // absorbed
                        contrib = mk(0.0, 0.0, 0.0);
                        ended = true;
                    } else {
                        T = T * texture_value<TEXTURED>(A, nullptr, A.textures, M, h.u, h.v, h.point);
                        o = h.point;
                        d = dir;
                        ended = false;
                    }
                } else if (SPECULAR) {
                    d = dielectric_scatter(M, h, d, rng, seg);
                    o = h.point;
                    ended = false;
                } else { // unreachable: the host picks SPECULAR whenever such a material exists
                    contrib = mk(0.0, 0.0, 0.0);
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
            sum = sum + contrib; // vec3.rs:38-42 Color::add, in sample order
            ++s;
            alive = false;
        }
    }

    if (in_image) {
        double *px_out = A.accum + 3 * (size_t)rng.pixel;
        if (A.sample_begin == 0) {
            px_out[0] = sum.x; px_out[1] = sum.y; px_out[2] = sum.z;
        } else {
            px_out[0] += sum.x; px_out[1] += sum.y; px_out[2] += sum.z;
        }
    }
    wave_stat_add(A, lane, RT_STAT_SEGMENTS, n_segments);
    wave_stat_add(A, lane, RT_STAT_SAMPLES, n_started); // primary rays (RtRenderStats.samples)
}

} // namespace RT_KNS

namespace {
// k_trace_f64 has no BVH form and the launcher below never asks for one: the BVH column of the variant table is empty
// (it names no kernel, so the twelve instantiations are the linear loop's, in the order of their classes)
template <int PRIMS, bool TEXTURED, bool SPECULAR, bool BVH> struct TraceVariant {
    static void launch(const rtdev::TraceArgs &a, unsigned blocks, hipStream_t stream) {
        if constexpr (!BVH)
            hipLaunchKernelGGL((RT_KNS::k_trace_f64<PRIMS, TEXTURED, SPECULAR>), dim3(blocks), dim3(256), 0, stream, a);
    }
};
} // namespace

// prims_class: rtdev::PRIMS_*; textured/specular: scene feature flags (see k_trace_f64)
extern "C" hipError_t RT_LAUNCHER(rtdev_launch_trace)(const rtdev::TraceArgs *args, int prims_class, int textured,
                                         int specular, hipStream_t stream) {
    const unsigned blocks = rtdev::frame_blocks(*args);
    if (blocks == 0) return hipSuccess;
    rtdev::dispatch_variant<TraceVariant>(prims_class, textured != 0, specular != 0, false, [&](auto v) {
        decltype(v)::launch(*args, blocks, stream);
    });
    return hipGetLastError();
}
