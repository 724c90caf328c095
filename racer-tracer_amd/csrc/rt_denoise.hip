// rt_denoise.hip — first-hit guide buffers and the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) behind
// rt_render_guides_device, rt_denoise_device, rt_denoise_frame and rt_render_progressive_denoised (include/rt_abi.h).
//
// The reference's ray_color returns the first hit's normal, position, depth and obj_id beside the colour (renderer.rs:
// RayImageData), and renderer/denoised.rs filters the frame pass by pass with them — a filter its author left unfinished.
// This is that filter, defined in DESIGN.md section 4.6:
//   guides   one deterministic ray per pixel through the pixel's centre (no draw), the scene's own closest-hit rule;
//   demod    I = g^2 / max(albedo, 1e-3) per channel (or g^2);
//   a-trous  K launches, step s = 2^i: I'_p = sum w_pq I_q / sum w_pq over q = p + s (dx, dy), dx, dy in -2..2, taps outside
//            the image dropped; w_pq = h(dx) h(dy) [id_p = id_q] w_n w_x w_c; misses pass through;
//   remod    sqrt(max(I_K * albedo, 0)) (or sqrt(max(I_K, 0))).
// Everything is f64; the tap loop adds in one fixed order (dy, then dx), so tests/denoise_model.py restates it to rounding.
// The loop itself is rt_filter_taps.h's atrous_pixel, which rt_temporal.hip's variance-guided level instantiates too; the
// host rules the three filter units share (guides_complete, pixel_grid, filter_stops, enqueue_levels) are defined below.
//
// Compiled once, with the fast arithmetic (RT_ARITH_FAST's hit functions of rt_trace_common.h).  The filter reads its taps
// straight from global memory: the planes of a 1080p frame (~130 MB for the guides, 50 MB per colour buffer) are served by
// L2 and the Infinity Cache, and the measured cost is in DESIGN.md.
#include "rt_path_steps.h"
#include "rt_filter_taps.h"
#include "rt_scene.h"

#include <cmath>
#include <cstring>
#include <utility>

namespace RT_KNS {

// ------------------------------------------------------------------------------------------------------------ guides
// One lane per pixel, 16x16 pixels per block.  TraceArgs comes FIRST in the kernel's arguments: closest_hit_bvh reads
// the root box through the kernarg segment (rt_trace_common.h: kernargs_here).
template <bool BVH>
__global__ __launch_bounds__(256) void k_guides_f64(const TraceArgs A, const RtGuides G) {
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= A.width || py >= A.height) return;
    const size_t pix = (size_t)py * (size_t)A.width + (size_t)px;

    // primary_ray's camera (rt_path_steps.h) with the lens offset at zero, through the pixel's centre, at the middle of the
    // shutter interval: a ray of its own, without a draw
    const double u = ((double)px + 0.5) / (double)(A.width - 1);
    const double v = ((double)py + 0.5) / (double)(A.height - 1);
    const d3 o = ld3(A.cam.origin);
    const d3 d = ld3(A.cam.ulc) + u * ld3(A.cam.horizontal) - v * ld3(A.cam.vertical) - o;
    const double time = (A.cam.time_a + A.cam.time_b) * 0.5;

    // the render's own closest-hit rule
    double best_t;
    int best, best_aux;
    closest_hit<PRIMS_ANY, BVH>(A, o, d, time, best_t, best, best_aux);

    d3 n = mk(0.0, 0.0, 0.0), x = n, albedo = mk(1.0, 1.0, 1.0);
    double footprint = __builtin_inf();
    int id = -1;
    if (best >= 0) {
        const Prim &P = A.prims[best];
        const Material &M = P.mat;
        const Hit h = prim_hit_record<PRIMS_ANY, true>(P, o, d, time, best_t, best_aux, M.needs_uv != 0);
        n = h.normal;
        x = h.point;
        if (M.kind == RT_MAT_LAMBERTIAN || M.kind == RT_MAT_METAL) {
            const d3 c = texture_value<true>(A, nullptr, A.textures, M, h.u, h.v, h.point);
            albedo = mk(clamp01(c.x), clamp01(c.y), clamp01(c.z));
        }
        footprint = best_t * sqrt(len2(ld3(A.cam.vertical))) / (double)(A.height - 1);
        id = P.obj_id;
    }
    G.normal[3 * pix + 0] = n.x;
    G.normal[3 * pix + 1] = n.y;
    G.normal[3 * pix + 2] = n.z;
    G.position[3 * pix + 0] = x.x;
    G.position[3 * pix + 1] = x.y;
    G.position[3 * pix + 2] = x.z;
    G.albedo[3 * pix + 0] = albedo.x;
    G.albedo[3 * pix + 1] = albedo.y;
    G.albedo[3 * pix + 2] = albedo.z;
    G.footprint[pix] = footprint;
    G.obj_id[pix] = id;
}

// ------------------------------------------------------------------------------------------------------------ filter
// demodulation: I = g^2 (/ max(albedo, 1e-3))
__global__ __launch_bounds__(256) void k_denoise_demod(const double *__restrict__ g, const double *__restrict__ albedo,
                                                       double *__restrict__ out, size_t n, int demodulate) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = demodulated(g[i], albedo[i], demodulate);
}

// remodulation: sqrt(max(I * albedo, 0)) (or sqrt(max(I, 0)))
__global__ __launch_bounds__(256) void k_denoise_remod(const double *__restrict__ I, const double *__restrict__ albedo,
                                                       double *__restrict__ out, size_t n, int demodulate) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double L = demodulate ? I[i] * albedo[i] : I[i];
        out[i] = sqrt(fmax(L, 0.0));
    }
}

struct AtrousArgs {
    int width, height, step;
    double inv_sn2;    // 1 / sigma_n^2, or 0: the normal stop is off
    double inv_sx;     // 1 / (sigma_x * step), or 0: the plane stop is off
    double inv_sc2;    // 1 / (sigma_c * 2^-i)^2, or 0: the colour stop is off
};

// One a-trous level: lane = pixel, 16x16 pixels per block (rt_filter_taps.h: atrous_pixel).
__global__ __launch_bounds__(256) void k_denoise_atrous(const AtrousArgs P, const double *__restrict__ I,
                                                        const RtGuides G, double *__restrict__ out) {
    atrous_pixel<false>(P.width, P.height, P.step, P.inv_sn2, P.inv_sx, P.inv_sc2, 0.0, I, nullptr, G, out, nullptr);
}

} // namespace RT_KNS

extern "C" hipError_t rtdev_launch_guides(const rtdev::TraceArgs *args, const RtGuides *guides, hipStream_t stream) {
    const dim3 grid = rtapi::pixel_grid(args->width, args->height);
    if (args->n_bvh_nodes > 0) hipLaunchKernelGGL(RT_KNS::k_guides_f64<true>, grid, dim3(256), 0, stream, *args, *guides);
    else hipLaunchKernelGGL(RT_KNS::k_guides_f64<false>, grid, dim3(256), 0, stream, *args, *guides);
    return hipGetLastError();
}

extern "C" hipError_t rtdev_launch_denoise_step(const RtDenoiseParams *d, int step, int width, int height, const double *in,
                                                const RtGuides *guides, double *out, hipStream_t stream) {
    const size_t n = (size_t)width * (size_t)height * 3;
    const int demodulate = (d->flags & RT_DENOISE_DEMODULATE) != 0;
    if (step < 0 || step >= d->iterations) {
        unsigned blocks = (unsigned)((n + 255) / 256);
        if (blocks > 4096u) blocks = 4096u;
        if (step < 0) hipLaunchKernelGGL(RT_KNS::k_denoise_demod, dim3(blocks), dim3(256), 0, stream, in, guides->albedo, out, n, demodulate);
        else hipLaunchKernelGGL(RT_KNS::k_denoise_remod, dim3(blocks), dim3(256), 0, stream, in, guides->albedo, out, n, demodulate);
        return hipGetLastError();
    }
    const rtapi::FilterStops st = rtapi::filter_stops(d, step);
    const RT_KNS::AtrousArgs a = {width, height, 1 << step, st.inv_sn2, st.inv_sx, st.inv_sc2};
    hipLaunchKernelGGL(RT_KNS::k_denoise_atrous, rtapi::pixel_grid(width, height), dim3(256), 0, stream, a, in, *guides, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------ host side
using rtapi::fail;

namespace {

constexpr int kMaxIterations = 10;
// calibrated on tests/denoise_model.py (cornell_box_boxes, 16 spp against 512 spp)
constexpr double kSigmaNormal = 0.1, kSigmaPlane = 1.0;

} // namespace

bool rtapi::guides_complete(const RtGuides *g) {
    return g && g->normal && g->position && g->albedo && g->footprint && g->obj_id;
}

dim3 rtapi::pixel_grid(int width, int height) { return dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)); }

rtapi::FilterStops rtapi::filter_stops(const RtDenoiseParams *d, int level) {
    FilterStops st;
    st.inv_sn2 = d->sigma_normal > 0.0 ? 1.0 / (d->sigma_normal * d->sigma_normal) : 0.0;
    st.inv_sx = d->sigma_plane > 0.0 ? 1.0 / (d->sigma_plane * (double)(1 << level)) : 0.0;
    const double sc = d->sigma_color > 0.0 ? ldexp(d->sigma_color, -level) : 0.0;
    st.inv_sc2 = sc > 0.0 ? 1.0 / (sc * sc) : 0.0;
    return st;
}

int rtapi::check_denoise(const RtRenderParams *p, const RtDenoiseParams *d) {
    if (!p || !d) return fail(RT_ERR_INVALID_ARGUMENT, "params/denoise is NULL");
    if (d->iterations < 0 || d->iterations > kMaxIterations) return fail(RT_ERR_INVALID_ARGUMENT, "denoise->iterations must be in 0..10");
    if (!std::isfinite(d->sigma_color) || !std::isfinite(d->sigma_normal) || !std::isfinite(d->sigma_plane))
        return fail(RT_ERR_INVALID_ARGUMENT, "denoise sigmas must be finite");
    for (int32_t r : d->_reserved)
        if (r != 0) return fail(RT_ERR_INVALID_ARGUMENT, "denoise->_reserved must be 0");
    if (p->width < 2 || p->height < 2) return fail(RT_ERR_INVALID_ARGUMENT, "width and height must be at least 2");
    if ((uint64_t)p->width * (uint64_t)p->height > 0xFFFFFFFFull) return fail(RT_ERR_INVALID_ARGUMENT, "image too large for the pixel counter");
    if (p->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "denoising works on whole frames: params->strip_* is not supported here");
    if (p->scale > 1) return fail(RT_ERR_INVALID_ARGUMENT, "denoising works on full-resolution frames: params->scale must be 0 or 1");
    return RT_OK;
}

int rtapi::reserve_denoise(RtScene *s, size_t pixels, bool own_guides, bool variance_planes) {
    RenderBuffers &b = s->buf;
    const size_t scratch = (variance_planes ? 8 : 6) * pixels;
    RT_HIP(b.denoise_scratch.reserve(scratch));
    if (own_guides) {
        RT_HIP(b.guide_planes.reserve(10 * pixels));
        RT_HIP(b.guide_ids.reserve(pixels));
    }
    return RT_OK;
}

RtGuides rtapi::scene_guides(RtScene *s, size_t pixels) {
    RtGuides g;
    double *planes = s->buf.guide_planes.ptr;
    g.normal = planes;
    g.position = planes + 3 * pixels;
    g.albedo = planes + 6 * pixels;
    g.footprint = planes + 9 * pixels;
    g.obj_id = s->buf.guide_ids.ptr;
    return g;
}

int rtapi::enqueue_guides(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtGuides &g, hipStream_t stream) {
    // the render's own argument block: the scene's tables, its tree and the camera (fill_args refuses nothing that
    // check_params has let through but a sample count the fixed-point sums cannot hold, which the guides do not use)
    rtdev::TraceArgs a;
    memset(&a, 0, sizeof a);
    RtRenderParams one = *p;
    one.samples = 1;
    int rc = rtapi::fill_trace_args(s, camera, &one, a);
    if (rc != RT_OK) return rc;
    if (!s->use_bvh) a.n_bvh_nodes = 0;
    RT_HIP(rtdev_launch_guides(&a, &g, stream));
    return RT_OK;
}

int rtapi::enqueue_denoise(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb, const RtGuides &g,
                           double *out, hipStream_t stream) {
    const size_t n = (size_t)p->width * (size_t)p->height * 3;
    if (d->iterations == 0) { // an exact copy
        RT_HIP(hipMemcpyAsync(out, rgb, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        return RT_OK;
    }
    double *ping = s->buf.denoise_scratch.ptr, *pong = ping + n;
    RT_HIP(rtdev_launch_denoise_step(d, -1, p->width, p->height, rgb, &g, ping, stream));
    for (int i = 0; i < d->iterations; ++i) {
        RT_HIP(rtdev_launch_denoise_step(d, i, p->width, p->height, ping, &g, pong, stream));
        std::swap(ping, pong);
    }
    RT_HIP(rtdev_launch_denoise_step(d, d->iterations, p->width, p->height, ping, &g, out, stream));
    return RT_OK;
}

int rtapi::enqueue_levels(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, double sigma_l, const double *radiance,
                          const double *variance, const RtGuides &g, double *out, hipStream_t stream) {
    const size_t pixels = (size_t)p->width * (size_t)p->height, n = 3 * pixels;
    int rc = reserve_denoise(s, pixels, false, true);
    if (rc != RT_OK) return rc;
    const double *in = radiance, *var = variance;
    double *ping = s->buf.denoise_scratch.ptr, *pong = ping + n;
    double *var_next = ping + 2 * n, *var_other = var_next + pixels;
    for (int i = 0; i < d->iterations; ++i) {
        if (sigma_l > 0.0) {
            RT_HIP(rtdev_launch_atrous_var(d, sigma_l, i, p->width, p->height, in, var, &g, ping, var_next, stream));
            var = var_next;
            std::swap(var_next, var_other);
        } else { // rt_denoise_device's own levels
            RT_HIP(rtdev_launch_denoise_step(d, i, p->width, p->height, in, &g, ping, stream));
        }
        in = ping;
        std::swap(ping, pong);
    }
    RT_HIP(rtdev_launch_denoise_step(d, d->iterations, p->width, p->height, in, &g, out, stream)); // re-modulation
    return RT_OK;
}

namespace {

int render_guides_device(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtGuides *g, void *stream) {
    RtDenoiseParams none;
    rt_denoise_params_default(&none);
    int rc = rtapi::check_denoise(p, &none);
    if (rc != RT_OK) return rc;
    if (!rtapi::guides_complete(g)) return fail(RT_ERR_INVALID_ARGUMENT, "guides_device or one of its planes is NULL");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if ((rc = rtapi::check_params(camera, p)) != RT_OK) return rc;
    RT_HIP(hipSetDevice(s->device));
    return rtapi::enqueue_guides(s, camera, p, *g, (hipStream_t)stream);
}

int denoise_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb, const RtGuides *g,
                   double *out, void *stream) {
    int rc = rtapi::check_denoise(p, d);
    if (rc != RT_OK) return rc;
    if (!rgb || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_device/out_device is NULL");
    if (rgb == out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_device and out_device must differ");
    if (!rtapi::guides_complete(g)) return fail(RT_ERR_INVALID_ARGUMENT, "guides_device or one of its planes is NULL");
    if ((rc = rtapi::use_scene_device(s)) != RT_OK) return rc;
    if ((rc = rtapi::reserve_denoise(s, (size_t)p->width * (size_t)p->height, false)) != RT_OK) return rc;
    return rtapi::enqueue_denoise(s, p, d, rgb, *g, out, (hipStream_t)stream);
}

int denoise_frame(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb,
                  double *out) {
    int rc = rtapi::check_denoise(p, d);
    if (rc != RT_OK) return rc;
    if (!rgb || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_host/out_host is NULL");
    if (rgb == out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_host and out_host must differ");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if ((rc = rtapi::check_params(camera, p)) != RT_OK) return rc;
    RT_HIP(hipSetDevice(s->device));
    const size_t pixels = (size_t)p->width * (size_t)p->height, n = 3 * pixels;
    rtapi::RenderBuffers &b = s->buf;
    if ((rc = rtapi::reserve_denoise(s, pixels, true)) != RT_OK) return rc;
    RT_HIP(b.frame.reserve(2 * n));
    const hipStream_t stream = b.stream;
    const RtGuides g = rtapi::scene_guides(s, pixels);
    if ((rc = rtapi::enqueue_guides(s, camera, p, g, stream)) != RT_OK) return rc;
    RT_HIP(hipMemcpyAsync(b.frame.ptr, rgb, n * sizeof(double), hipMemcpyHostToDevice, stream));
    if ((rc = rtapi::enqueue_denoise(s, p, d, b.frame.ptr, g, b.frame.ptr + n, stream)) != RT_OK) return rc;
    RT_HIP(hipMemcpyAsync(out, b.frame.ptr + n, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

} // namespace

extern "C" {

void rt_denoise_params_default(RtDenoiseParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->iterations = 5;
    out->flags = RT_DENOISE_DEMODULATE;
    out->sigma_color = 0.0;
    out->sigma_normal = kSigmaNormal;
    out->sigma_plane = kSigmaPlane;
}

int rt_render_guides_device(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtGuides *guides_device,
                            void *hip_stream) {
    return rtapi::guarded("rt_render_guides_device", [&] { return render_guides_device(s, camera, p, guides_device, hip_stream); });
}

int rt_denoise_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb_device,
                      const RtGuides *guides_device, double *out_device, void *hip_stream) {
    return rtapi::guarded("rt_denoise_device", [&] { return denoise_device(s, p, d, rgb_device, guides_device, out_device, hip_stream); });
}

int rt_denoise_frame(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb_host,
                     double *out_host) {
    return rtapi::guarded("rt_denoise_frame", [&] { return denoise_frame(s, camera, p, d, rgb_host, out_host); });
}

} // extern "C"
