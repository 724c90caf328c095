// rt_temporal.hip — temporal accumulation and the variance-guided a-trous filter behind rt_temporal_accumulate_device,
// rt_denoise_history_device and rt_render_temporal (include/rt_abi.h), defined in DESIGN.md section 4.11.
//
// The reference's renderer/denoised.rs plans "Implement SVGF" with a temporal() blend; rt_denoise.hip is the spatial half
// of that plan, this is the other: a history of demodulated linear radiance and luminance moments that follows the camera
// by re-projecting the first hits of the guides, and a luminance stop scaled by the local standard deviation.
//   accumulate  C = g^2 (/ max(albedo, 1e-3)); the hit point through the PREVIOUS camera's pinhole (Cramer's rule), four
//               bilinear taps (j, then i) that agree in id, normal and plane; a = max(1 / (L + 1), alpha)
//   variance    (m2 - m1^2) / length where length >= 4, else the 7x7 neighbourhood's (dy, then dx)
//   a-trous     rt_denoise.hip's level with the factor exp(-|l_p - l_q| / (sigma_l sqrt(vbar_p) + 1e-10)); the variance is
//               filtered alongside with the squared weights
// With sigma_luminance <= 0 the levels are rt_denoise.hip's own launches, and the re-modulation always is.
// The demodulation, the 7x7 window and the level are rt_filter_taps.h's demodulated, spatial_variance and
// atrous_pixel<true>: the kernels here are its callers, as rt_denoise.hip's and rt_variance_filter.hip's are.  The
// re-projection with its taps, the blend and the stores of a history pixel are rt_history_taps.h's, which
// k_preview_accumulate (rt_preview_temporal.hip) calls too; the host side lends that unit its checks, the fill of the
// argument block's history fields and the whole-frame sequence (rt_temporal_state.h).
//
// Compiled once, with the fast arithmetic, as rt_denoise.hip.  Lane = pixel, 16x16 pixels per block, taps straight from
// global memory.  The launchers have internal linkage, but for rtdev_launch_atrous_var (rt_scene.h), through which
// rtapi::enqueue_levels (rt_denoise.hip) runs the levels of a history here and of a still frame's batch variance.
#include "rt_trace_common.h"
#include "rt_filter_taps.h"
#include "rt_history_taps.h"
#include "rt_scene.h"
#include "rt_temporal_state.h"

#include <cmath>
#include <cstring>
#include <memory>

namespace RT_KNS {

struct AccumulateArgs {
    int width, height;
    int has_prev, demodulate;
    double o[3], ulc[3], hor[3], ver[3]; // the previous camera
    double alpha, alpha_moments, max_history;
    double normal_tol2;                  // normal_tolerance^2
    double plane_tol;
};

// One pixel of the accumulation (rt_history_taps.h): the pixel's own sample first, then its history.
__global__ __launch_bounds__(256) void k_temporal_accumulate(const AccumulateArgs P, const double *__restrict__ g,
                                                             const RtGuides G, const RtHistory prev, const RtHistory out) {
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= P.width || py >= P.height) return;
    const size_t p = (size_t)py * (size_t)P.width + (size_t)px;

    double c[3]; // (k_denoise_demod's values)
    for (int k = 0; k < 3; ++k) c[k] = demodulated(g[3 * p + k], G.albedo[3 * p + k], P.demodulate);
    const d3 cp = mk(c[0], c[1], c[2]);
    const double lp = luminance(cp);
    const int id = G.obj_id[p];
    const d3 np = ld3(G.normal + 3 * p), xp = ld3(G.position + 3 * p);

    HistoryPixel v = fresh_pixel(cp, lp);
    HistorySums h;
    if (P.has_prev && id >= 0 && history_value<false>(P, G, prev, p, id, np, xp, h)) v = blended_pixel(P, h, cp, lp);
    store_history(out, p, v, np, xp, id);
}

struct VarianceArgs {
    int width, height;
    double inv_sn2; // 1 / sigma_n^2, or 0: the normal stop is off
    double inv_sx;  // 1 / sigma_x (step 1), or 0: the plane stop is off
};

// The variance of the accumulated luminance: the moments' where the history is long enough, else the neighbourhood's.
__global__ __launch_bounds__(256) void k_temporal_variance(const VarianceArgs P, const double *__restrict__ radiance,
                                                           const double *__restrict__ moments,
                                                           const double *__restrict__ length, const RtGuides G,
                                                           double *__restrict__ var) {
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= P.width || py >= P.height) return;
    const size_t p = (size_t)py * (size_t)P.width + (size_t)px;
    const int id = G.obj_id[p];
    if (id < 0) {
        var[p] = 0.0;
        return;
    }
    const double len = length[p];
    if (len >= 4.0) {
        const double m1 = moments[2 * p + 0], m2 = moments[2 * p + 1];
        var[p] = fmax(0.0, m2 - __dmul_rn(m1, m1)) / len; // the square rounded on its own: m2 == m1^2 gives exactly 0
        return;
    }
    var[p] = spatial_variance(px, py, P.width, P.height, P.inv_sn2, P.inv_sx, radiance, G, p, id);
}

struct AtrousVarArgs {
    int width, height, step;
    double inv_sn2, inv_sx, inv_sc2; // rt_denoise.hip: AtrousArgs
    double sigma_l;                  // > 0
};

// One variance-guided level (rt_filter_taps.h: atrous_pixel).
__global__ __launch_bounds__(256) void k_temporal_atrous(const AtrousVarArgs P, const double *__restrict__ I,
                                                         const double *__restrict__ var, const RtGuides G,
                                                         double *__restrict__ out, double *__restrict__ var_out) {
    atrous_pixel<true>(P.width, P.height, P.step, P.inv_sn2, P.inv_sx, P.inv_sc2, P.sigma_l, I, var, G, out, var_out);
}

} // namespace RT_KNS

// ------------------------------------------------------------------------------------------------------------ host side
using rtapi::fail;

namespace {

using rtapi::guides_complete;
using rtapi::pixel_grid;

int enqueue_accumulate(const RtRenderParams *p, const RtTemporalParams *t, const RtDenoiseParams *d, const double *rgb,
                       const RtGuides *g, const RtCamera *prev_camera, const RtHistory *prev, const RtHistory *out,
                       hipStream_t stream) {
    RT_KNS::AccumulateArgs a;
    memset(&a, 0, sizeof a);
    a.width = p->width;
    a.height = p->height;
    a.demodulate = (d->flags & RT_DENOISE_DEMODULATE) != 0;
    rtapi::fill_history_args(a, t, prev_camera);
    hipLaunchKernelGGL(RT_KNS::k_temporal_accumulate, pixel_grid(p->width, p->height), dim3(256), 0, stream, a, rgb, *g,
                       prev ? *prev : *out, *out);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

hipError_t launch_variance(const RtRenderParams *p, const RtDenoiseParams *d, const RtHistory *h, const RtGuides *g, double *var,
                           hipStream_t stream) {
    const rtapi::FilterStops st = rtapi::filter_stops(d);
    const RT_KNS::VarianceArgs a = {p->width, p->height, st.inv_sn2, st.inv_sx};
    hipLaunchKernelGGL(RT_KNS::k_temporal_variance, pixel_grid(p->width, p->height), dim3(256), 0, stream, a, h->radiance,
                       h->moments, h->length, *g, var);
    return hipGetLastError();
}

// calibrated on tests/temporal_model.py (cornell_box_boxes, eight 4-spp frames on a 1-degree orbit)
constexpr double kAlpha = 0.2, kMaxHistory = 32.0;
constexpr double kNormalTolerance = 0.25, kPlaneTolerance = 2.0, kSigmaLuminance = 4.0;

} // namespace

// what rt_preview_temporal.hip shares (rt_temporal_state.h)
namespace rtapi {

static bool history_complete(const RtHistory *h) {
    return h && h->radiance && h->moments && h->length && h->normal && h->position && h->obj_id;
}

int check_temporal(const RtTemporalParams *t) {
    if (!t) return fail(RT_ERR_INVALID_ARGUMENT, "temporal is NULL");
    for (double v : {t->alpha, t->alpha_moments, t->max_history, t->normal_tolerance, t->plane_tolerance, t->sigma_luminance})
        if (!std::isfinite(v)) return fail(RT_ERR_INVALID_ARGUMENT, "temporal parameters must be finite");
    if (t->alpha < 0.0 || t->alpha > 1.0 || t->alpha_moments < 0.0 || t->alpha_moments > 1.0)
        return fail(RT_ERR_INVALID_ARGUMENT, "temporal->alpha and alpha_moments must be in 0..1");
    if (t->max_history < 1.0) return fail(RT_ERR_INVALID_ARGUMENT, "temporal->max_history must be at least 1");
    for (int32_t r : t->_reserved)
        if (r != 0) return fail(RT_ERR_INVALID_ARGUMENT, "temporal->_reserved must be 0");
    return RT_OK;
}

int check_accumulate_buffers(const double *rgb, const RtGuides *g, const RtCamera *prev_camera, const RtHistory *prev,
                             const RtHistory *out) {
    if (!rgb) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_device is NULL");
    if (!guides_complete(g)) return fail(RT_ERR_INVALID_ARGUMENT, "guides_device or one of its planes is NULL");
    if (!history_complete(out)) return fail(RT_ERR_INVALID_ARGUMENT, "out_history or one of its planes is NULL");
    if ((prev_camera == nullptr) != (prev == nullptr))
        return fail(RT_ERR_INVALID_ARGUMENT, "prev_camera and prev_history are both NULL or neither is");
    if (prev) {
        if (!history_complete(prev)) return fail(RT_ERR_INVALID_ARGUMENT, "prev_history has a NULL plane");
        if (prev->radiance == out->radiance || prev->moments == out->moments || prev->length == out->length ||
            prev->normal == out->normal || prev->position == out->position || prev->obj_id == out->obj_id)
            return fail(RT_ERR_INVALID_ARGUMENT, "out_history and prev_history must differ");
    }
    return RT_OK;
}

// the filter of a history into `out`: its variance, where levels will use one, into the second variance plane of the
// scene's scratch (rt_scene.h: enqueue_levels)
int enqueue_denoise_history(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const RtTemporalParams *t,
                            const RtHistory *h, const RtGuides *g, double *out, hipStream_t stream) {
    const size_t pixels = (size_t)p->width * (size_t)p->height;
    double *var = nullptr;
    if (t->sigma_luminance > 0.0 && d->iterations > 0) {
        int rc = rtapi::reserve_denoise(s, pixels, false, true);
        if (rc != RT_OK) return rc;
        var = s->buf.denoise_scratch.ptr + 7 * pixels;
        RT_HIP(launch_variance(p, d, h, g, var, stream));
    }
    return rtapi::enqueue_levels(s, p, d, var ? t->sigma_luminance : 0.0, h->radiance, var, *g, out, stream);
}

int render_into_state(RtScene *s, RtTemporal *t, const char *v1_message, const RtCamera *camera, const RtCamera *render_camera,
                      const RtRenderParams *p, const RtRenderParams *full, const RtTemporalParams *tp, const RtDenoiseParams *d,
                      const EnqueueAccumulate &accumulate, double *out_rgb, double *out_length) {
    if (!out_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgb_host is NULL");
    if (!t) return fail(RT_ERR_INVALID_ARGUMENT, "temporal_state is NULL");
    if (p->width != t->width || p->height != t->height)
        return fail(RT_ERR_INVALID_ARGUMENT, "params->width and height must be the RtTemporal's");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (s->device != t->device) return fail(RT_ERR_INVALID_ARGUMENT, "the scene and the RtTemporal must be on the same device");
    if (s->use_v1) return fail(RT_ERR_UNSUPPORTED, v1_message);
    RT_HIP(hipSetDevice(s->device));
    const size_t pixels = (size_t)p->width * (size_t)p->height, n = 3 * pixels;
    const hipStream_t stream = s->buf.stream;
    double *frame = state_frame(t), *filtered = frame + n;
    const RtGuides g = state_guides(t);
    const RtHistory prev = state_history(t, t->current), next = state_history(t, t->current ^ 1);
    int rc = enqueue_render(s, render_camera, p, frame, stream, 0, Cancel());
    if (rc != RT_OK) return rc;
    if ((rc = enqueue_guides(s, camera, full, g, stream)) != RT_OK) return rc;
    if ((rc = accumulate(frame, &g, t->has_prev ? &t->camera : nullptr, t->has_prev ? &prev : nullptr, &next, stream)) != RT_OK)
        return rc;
    if ((rc = enqueue_denoise_history(s, full, d, tp, &next, &g, filtered, stream)) != RT_OK) return rc;
    RT_HIP(hipMemcpyAsync(out_rgb, filtered, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (out_length) RT_HIP(hipMemcpyAsync(t->host_length.ptr, next.length, pixels * sizeof(double), hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    if (out_length) memcpy(out_length, t->host_length.ptr, pixels * sizeof(double));
    t->current ^= 1;
    t->has_prev = true;
    t->camera = *camera;
    return RT_OK;
}

} // namespace rtapi

namespace {

using rtapi::check_temporal;
using rtapi::enqueue_denoise_history;
using rtapi::history_complete;
using rtapi::kStateDoubles;

int accumulate_device(RtScene *s, const RtRenderParams *p, const RtTemporalParams *t, const RtDenoiseParams *d, const double *rgb,
                      const RtGuides *g, const RtCamera *prev_camera, const RtHistory *prev, const RtHistory *out, void *stream) {
    int rc = rtapi::check_denoise(p, d);
    if (rc != RT_OK) return rc;
    if ((rc = check_temporal(t)) != RT_OK) return rc;
    if ((rc = rtapi::check_accumulate_buffers(rgb, g, prev_camera, prev, out)) != RT_OK) return rc;
    if ((rc = rtapi::use_scene_device(s)) != RT_OK) return rc;
    return enqueue_accumulate(p, t, d, rgb, g, prev_camera, prev, out, (hipStream_t)stream);
}

int denoise_history_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const RtTemporalParams *t,
                           const RtHistory *h, const RtGuides *g, double *out, void *stream) {
    int rc = rtapi::check_denoise(p, d);
    if (rc != RT_OK) return rc;
    if ((rc = check_temporal(t)) != RT_OK) return rc;
    if (!history_complete(h)) return fail(RT_ERR_INVALID_ARGUMENT, "history or one of its planes is NULL");
    if (!guides_complete(g)) return fail(RT_ERR_INVALID_ARGUMENT, "guides_device or one of its planes is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out_device is NULL");
    if (out == h->radiance) return fail(RT_ERR_INVALID_ARGUMENT, "out_device and the history's radiance must differ");
    if ((rc = rtapi::use_scene_device(s)) != RT_OK) return rc;
    return enqueue_denoise_history(s, p, d, t, h, g, out, (hipStream_t)stream);
}

int temporal_create(int device, int32_t width, int32_t height, RtTemporal **out) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (width < 2 || height < 2) return fail(RT_ERR_INVALID_ARGUMENT, "width and height must be at least 2");
    if ((uint64_t)width * (uint64_t)height > 0xFFFFFFFFull) return fail(RT_ERR_INVALID_ARGUMENT, "image too large for the pixel counter");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail(RT_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(RT_ERR_INVALID_ARGUMENT, "device out of range");
    RT_HIP(hipSetDevice(device));
    std::unique_ptr<RtTemporal> t(new RtTemporal()); // (a state half made frees what it got on the way out)
    t->device = device;
    t->width = width;
    t->height = height;
    const size_t pixels = (size_t)width * (size_t)height;
    hipError_t e = t->planes.alloc(kStateDoubles * pixels);
    if (e == hipSuccess) e = t->ids.alloc(3 * pixels);
    if (e == hipSuccess) e = t->host_length.alloc(pixels, hipHostMallocDefault);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP, std::string("rt_temporal_create: ") + hipGetErrorString(e));
    *out = t.release();
    return RT_OK;
}

int render_temporal(RtScene *s, RtTemporal *t, const RtCamera *camera, const RtRenderParams *p, const RtTemporalParams *tp,
                    const RtDenoiseParams *d, double *out_rgb, double *out_length) {
    int rc = rtapi::check_denoise(p, d);
    if (rc != RT_OK) return rc;
    if ((rc = check_temporal(tp)) != RT_OK) return rc;
    if ((rc = rtapi::check_params(camera, p)) != RT_OK) return rc;
    const auto accumulate = [&](const double *frame, const RtGuides *g, const RtCamera *prev_camera, const RtHistory *prev,
                                const RtHistory *out, hipStream_t stream) {
        return enqueue_accumulate(p, tp, d, frame, g, prev_camera, prev, out, stream);
    };
    return rtapi::render_into_state(s, t, "rt_render_temporal needs the pooled kernel", camera, camera, p, p, tp, d, accumulate,
                                    out_rgb, out_length);
}

} // namespace

extern "C" hipError_t rtdev_launch_atrous_var(const RtDenoiseParams *d, double sigma_l, int step, int width, int height,
                                              const double *in, const double *var, const RtGuides *guides, double *out,
                                              double *var_out, hipStream_t stream) {
    const rtapi::FilterStops st = rtapi::filter_stops(d, step);
    const RT_KNS::AtrousVarArgs a = {width, height, 1 << step, st.inv_sn2, st.inv_sx, st.inv_sc2, sigma_l};
    hipLaunchKernelGGL(RT_KNS::k_temporal_atrous, rtapi::pixel_grid(width, height), dim3(256), 0, stream, a, in, var, *guides, out,
                       var_out);
    return hipGetLastError();
}

extern "C" {

void rt_temporal_params_default(RtTemporalParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->alpha = kAlpha;
    out->alpha_moments = kAlpha;
    out->max_history = kMaxHistory;
    out->normal_tolerance = kNormalTolerance;
    out->plane_tolerance = kPlaneTolerance;
    out->sigma_luminance = kSigmaLuminance;
}

int rt_temporal_accumulate_device(RtScene *s, const RtRenderParams *p, const RtTemporalParams *t, const RtDenoiseParams *d,
                                  const double *rgb_device, const RtGuides *guides_device, const RtCamera *prev_camera,
                                  const RtHistory *prev_history, const RtHistory *out_history, void *hip_stream) {
    return rtapi::guarded("rt_temporal_accumulate_device", [&] {
        return accumulate_device(s, p, t, d, rgb_device, guides_device, prev_camera, prev_history, out_history, hip_stream);
    });
}

int rt_denoise_history_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const RtTemporalParams *t,
                              const RtHistory *history, const RtGuides *guides_device, double *out_device, void *hip_stream) {
    return rtapi::guarded("rt_denoise_history_device",
                          [&] { return denoise_history_device(s, p, d, t, history, guides_device, out_device, hip_stream); });
}

int rt_temporal_create(int device, int32_t width, int32_t height, RtTemporal **out) {
    return rtapi::guarded("rt_temporal_create", [&] { return temporal_create(device, width, height, out); });
}

void rt_temporal_destroy(RtTemporal *t) {
    delete t; // (~RtTemporal: on its own device)
}

int rt_temporal_reset(RtTemporal *t) {
    return rtapi::guarded("rt_temporal_reset", [&]() -> int {
        if (!t) return fail(RT_ERR_INVALID_ARGUMENT, "temporal_state is NULL");
        t->has_prev = false;
        return RT_OK;
    });
}

int rt_render_temporal(RtScene *s, RtTemporal *t, const RtCamera *camera, const RtRenderParams *p, const RtTemporalParams *tp,
                       const RtDenoiseParams *d, double *out_rgb_host, double *out_length_host) {
    return rtapi::guarded("rt_render_temporal", [&] { return render_temporal(s, t, camera, p, tp, d, out_rgb_host, out_length_host); });
}

} // extern "C"
