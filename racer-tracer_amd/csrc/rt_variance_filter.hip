// rt_variance_filter.hip — the variance-guided filter of a STILL frame behind rt_batch_variance_device,
// rt_denoise_variance_device and rt_render_adaptive_filtered (include/rt_abi.h), defined in DESIGN.md section 4.12.
//
// rt_temporal.hip's levels take a per-pixel variance of the luminance, which there comes from a history.  The adaptive
// renderer (rt_progressive.hip) already keeps what a single frame needs for one: per pixel and channel the running sum S
// and Q = sum_j S_j^2 / n_j over the chunks done, and per 8x8 tile the samples s and chunks k it stopped at — a batch-means
// estimate of every pixel's standard error.
//   batch variance  m = S / s; sigma = sqrt(max(0, Q - S m) / (k - 1) / s); C = m / a, sigma' = sigma / a with
//                   a = max(albedo, 1e-3) (or 1); var = (0.2126 sigma'_r + 0.7152 sigma'_g + 0.0722 sigma'_b)^2 where
//                   k >= min_chunks, 0 on a guide miss, else WAITING
//   spatial         a waiting pixel takes k_temporal_variance's neighbourhood estimate over C: the 7x7 window (dy, then dx),
//                   rt_filter_taps.h's spatial_variance for both
//   levels          rtapi::enqueue_levels (rt_denoise.hip), as rt_denoise_history_device: k_temporal_atrous's levels and
//                   the re-modulation of rtdev_launch_denoise_step
//
// Compiled once, with the fast arithmetic, as rt_denoise.hip and rt_temporal.hip.  Lane = pixel, 16x16 pixels per block,
// taps straight from global memory.
#include "rt_trace_common.h"
#include "rt_filter_taps.h"
#include "rt_scene.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace RT_KNS {

// what k_batch_variance leaves in var for a pixel whose tile has too few chunks: every variance is >= 0
constexpr double kWaiting = -1.0;

struct BatchVarianceArgs {
    int width, height;
    int demodulate, min_chunks;
};

// One pixel of the batch estimate.  The product S m is rounded on its own — no contraction in this kernel: __dmul_rn
// alone is a plain product to the compiler, and fma(-S, m, Q) would leave the rounding error of S m where equal chunk means
// (Q == S m) must give exactly no variance.
__global__ __launch_bounds__(256) void k_batch_variance(const BatchVarianceArgs P, const double *__restrict__ S,
                                                        const double *__restrict__ Q, const int32_t *__restrict__ samples,
                                                        const int32_t *__restrict__ chunks, const RtGuides G,
                                                        double *__restrict__ C, double *__restrict__ var) {
#pragma clang fp contract(off)
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= P.width || py >= P.height) return;
    const size_t p = (size_t)py * (size_t)P.width + (size_t)px;
    const double s = (double)samples[p];
    const int k = chunks[p];
    const bool batch = k >= P.min_chunks;
    const double batches = (double)(k - 1);
    double sl = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double Sc = S[3 * p + c];
        const double a = P.demodulate ? fmax(G.albedo[3 * p + c], 1e-3) : 1.0;
        const double m = Sc / s;
        C[3 * p + c] = m / a;
        if (batch) {
            const double sigma = sqrt(fmax(0.0, Q[3 * p + c] - __dmul_rn(Sc, m)) / batches / s);
            sl += luminance_weight(c) * (sigma / a);
        }
    }
    var[p] = G.obj_id[p] < 0 ? 0.0 : batch ? __dmul_rn(sl, sl) : kWaiting;
}

struct SpatialArgs {
    int width, height;
    double inv_sn2; // 1 / sigma_n^2, or 0: the normal stop is off
    double inv_sx;  // 1 / sigma_x (step 1), or 0: the plane stop is off
};

// The waiting pixels: the 7x7 estimate of k_temporal_variance's short histories (rt_filter_taps.h: spatial_variance) over
// C.  A pixel reads var at its own place only, so the pass needs no second plane.
__global__ __launch_bounds__(256) void k_batch_variance_spatial(const SpatialArgs P, const double *__restrict__ C,
                                                                const RtGuides G, double *var) {
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= P.width || py >= P.height) return;
    const size_t p = (size_t)py * (size_t)P.width + (size_t)px;
    if (!(var[p] < 0.0)) return;
    const int id = G.obj_id[p]; // (>= 0: a miss never waits)
    var[p] = spatial_variance(px, py, P.width, P.height, P.inv_sn2, P.inv_sx, C, G, p, id);
}

} // namespace RT_KNS

// ------------------------------------------------------------------------------------------------------------ host side
using rtapi::fail;

namespace {

// calibrated on tests/variance_filter_model.py (cornell_box_boxes and three_balls, 4 .. 256 spp)
constexpr double kSigmaLuminance = 4.0;
constexpr int kMinChunks = 4;

using rtapi::guides_complete;
using rtapi::pixel_grid;

int check_filter(const RtVarianceFilterParams *f) {
    if (!f) return fail(RT_ERR_INVALID_ARGUMENT, "filter is NULL");
    if (!std::isfinite(f->sigma_luminance)) return fail(RT_ERR_INVALID_ARGUMENT, "filter->sigma_luminance must be finite");
    if (f->min_chunks < 2) return fail(RT_ERR_INVALID_ARGUMENT, "filter->min_chunks must be at least 2");
    for (int32_t r : f->_reserved)
        if (r != 0) return fail(RT_ERR_INVALID_ARGUMENT, "filter->_reserved must be 0");
    return RT_OK;
}

int enqueue_batch_variance(const RtRenderParams *p, const RtDenoiseParams *d, const RtVarianceFilterParams *f,
                           const RtBatchPlanes *b, const RtGuides *g, double *radiance, double *var, hipStream_t stream) {
    RT_KNS::BatchVarianceArgs a;
    a.width = p->width;
    a.height = p->height;
    a.demodulate = (d->flags & RT_DENOISE_DEMODULATE) != 0;
    a.min_chunks = f->min_chunks;
    hipLaunchKernelGGL(RT_KNS::k_batch_variance, pixel_grid(p->width, p->height), dim3(256), 0, stream, a, b->sums, b->squares,
                       b->samples, b->chunks, *g, radiance, var);
    RT_HIP(hipGetLastError());
    const rtapi::FilterStops st = rtapi::filter_stops(d);
    const RT_KNS::SpatialArgs sa = {p->width, p->height, st.inv_sn2, st.inv_sx};
    hipLaunchKernelGGL(RT_KNS::k_batch_variance_spatial, pixel_grid(p->width, p->height), dim3(256), 0, stream, sa,
                       (const double *)radiance, *g, var);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int batch_variance_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const RtVarianceFilterParams *f,
                          const RtBatchPlanes *b, const RtGuides *g, double *radiance, double *var, void *stream) {
    int rc = rtapi::check_denoise(p, d);
    if (rc != RT_OK) return rc;
    if ((rc = check_filter(f)) != RT_OK) return rc;
    if (!b || !b->sums || !b->squares || !b->samples || !b->chunks)
        return fail(RT_ERR_INVALID_ARGUMENT, "batch_planes or one of its planes is NULL");
    if (!guides_complete(g)) return fail(RT_ERR_INVALID_ARGUMENT, "guides_device or one of its planes is NULL");
    if (!radiance || !var) return fail(RT_ERR_INVALID_ARGUMENT, "radiance_out_device/variance_out_device is NULL");
    if ((rc = rtapi::use_scene_device(s)) != RT_OK) return rc;
    return enqueue_batch_variance(p, d, f, b, g, radiance, var, (hipStream_t)stream);
}

int denoise_variance_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const RtVarianceFilterParams *f,
                            const double *radiance, const double *var, const RtGuides *g, double *out, void *stream) {
    int rc = rtapi::check_denoise(p, d);
    if (rc != RT_OK) return rc;
    if ((rc = check_filter(f)) != RT_OK) return rc;
    if (!radiance || !var) return fail(RT_ERR_INVALID_ARGUMENT, "radiance_device/variance_device is NULL");
    if (!guides_complete(g)) return fail(RT_ERR_INVALID_ARGUMENT, "guides_device or one of its planes is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out_device is NULL");
    if (out == radiance) return fail(RT_ERR_INVALID_ARGUMENT, "out_device and radiance_device must differ");
    if ((rc = rtapi::use_scene_device(s)) != RT_OK) return rc;
    return rtapi::enqueue_levels(s, p, d, f->sigma_luminance, radiance, var, *g, out, (hipStream_t)stream);
}

// the caller's cancel hook, remembering whether it was ever raised: a cancelled adaptive call returns RT_OK
struct CancelWatch {
    RtCancelCallback fn;
    void *user;
    bool raised;
};
int watch_cancel(void *w_) {
    CancelWatch *w = static_cast<CancelWatch *>(w_);
    const int r = w->fn(w->user);
    if (r != 0) w->raised = true;
    return r;
}

int render_adaptive_filtered(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                             const RtAdaptiveParams *ad, const RtDenoiseParams *d, const RtVarianceFilterParams *f,
                             double *out_rgb, RtBatchOutputs *outputs, RtFrameCallback callback, void *user,
                             RtCancelCallback cancelled, void *cancel_user) {
    int rc = rtapi::check_denoise(p, d); // (before the scene: the filter's refusals need no device)
    if (rc != RT_OK) return rc;
    if ((rc = check_filter(f)) != RT_OK) return rc;
    if (!out_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgb is NULL");
    const size_t pixels = (size_t)p->width * (size_t)p->height, n = 3 * pixels;
    std::vector<int32_t> own_samples;
    int32_t *samples = outputs ? outputs->samples : nullptr;
    if (!samples && ad) { // (a NULL adaptive is the adaptive call's to refuse)
        own_samples.resize(pixels);
        samples = own_samples.data();
    }
    double *tile_error = outputs ? outputs->tile_error : nullptr;
    CancelWatch watch{cancelled, cancel_user, false};
    const RtCancelCallback hook = cancelled ? watch_cancel : nullptr;
    rc = ls ? rt_render_adaptive_nee(s, camera, p, ls, ad, out_rgb, samples, tile_error, callback, user, hook, &watch)
            : rt_render_adaptive(s, camera, p, ad, out_rgb, samples, tile_error, callback, user, hook, &watch);
    if (rc != RT_OK || watch.raised) return rc;

    // every pixel's chunks done: its samples are a boundary of the frame's chunk plan
    const std::vector<int> starts = rtapi::chunk_plan(p->samples);
    std::vector<int32_t> chunks(pixels);
    for (size_t i = 0; i < pixels; ++i) {
        const auto at = std::lower_bound(starts.begin(), starts.end(), (int)samples[i]);
        if (samples[i] < 1 || at == starts.end() || *at != samples[i])
            return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_adaptive_filtered: a tile stopped off the chunk plan");
        chunks[i] = (int32_t)(at - starts.begin());
    }

    RT_HIP(hipSetDevice(s->device));
    rtapi::RenderBuffers &b = s->buf;
    if ((rc = rtapi::reserve_denoise(s, pixels, true)) != RT_OK) return rc;
    RT_HIP(b.batch_counts.reserve(2 * pixels));
    // the adaptive call has drained its streams: its frame slots (three of W*H*3) now hold C, var and the filtered frame
    RT_HIP(b.frame.reserve(7 * pixels));
    double *radiance = b.frame.ptr, *var = radiance + n, *filtered = var + pixels;
    const hipStream_t stream = b.stream;
    const RtGuides g = rtapi::scene_guides(s, pixels);
    RT_HIP(hipMemcpyAsync(b.batch_counts.ptr, samples, pixels * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    RT_HIP(hipMemcpyAsync(b.batch_counts.ptr + pixels, chunks.data(), pixels * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if ((rc = rtapi::enqueue_guides(s, camera, p, g, stream)) != RT_OK) return rc;
    const RtBatchPlanes planes = {b.accum.ptr, b.squares.ptr, b.batch_counts.ptr, b.batch_counts.ptr + pixels};
    if ((rc = enqueue_batch_variance(p, d, f, &planes, &g, radiance, var, stream)) != RT_OK) return rc;
    if ((rc = rtapi::enqueue_levels(s, p, d, f->sigma_luminance, radiance, var, g, filtered, stream)) != RT_OK) return rc;
    if (outputs && outputs->raw_rgb) memcpy(outputs->raw_rgb, out_rgb, n * sizeof(double));
    RT_HIP(hipMemcpyAsync(out_rgb, filtered, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (outputs && outputs->sums) RT_HIP(hipMemcpyAsync(outputs->sums, b.accum.ptr, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (outputs && outputs->squares)
        RT_HIP(hipMemcpyAsync(outputs->squares, b.squares.ptr, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (outputs && outputs->variance)
        RT_HIP(hipMemcpyAsync(outputs->variance, var, pixels * sizeof(double), hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    if (outputs && outputs->chunks) memcpy(outputs->chunks, chunks.data(), pixels * sizeof(int32_t));
    return RT_OK;
}

} // namespace

extern "C" {

void rt_variance_filter_params_default(RtVarianceFilterParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->sigma_luminance = kSigmaLuminance;
    out->min_chunks = kMinChunks;
}

int rt_batch_variance_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const RtVarianceFilterParams *f,
                             const RtBatchPlanes *batch_planes, const RtGuides *guides_device, double *radiance_out_device,
                             double *variance_out_device, void *hip_stream) {
    return rtapi::guarded("rt_batch_variance_device", [&] {
        return batch_variance_device(s, p, d, f, batch_planes, guides_device, radiance_out_device, variance_out_device, hip_stream);
    });
}

int rt_denoise_variance_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const RtVarianceFilterParams *f,
                               const double *radiance_device, const double *variance_device, const RtGuides *guides_device,
                               double *out_device, void *hip_stream) {
    return rtapi::guarded("rt_denoise_variance_device", [&] {
        return denoise_variance_device(s, p, d, f, radiance_device, variance_device, guides_device, out_device, hip_stream);
    });
}

int rt_render_adaptive_filtered(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                                const RtAdaptiveParams *adaptive, const RtDenoiseParams *d, const RtVarianceFilterParams *f,
                                double *out_rgb, RtBatchOutputs *outputs, RtFrameCallback callback, void *user,
                                RtCancelCallback cancelled, void *cancel_user) {
    return rtapi::guarded("rt_render_adaptive_filtered", [&] {
        return render_adaptive_filtered(s, camera, p, ls, adaptive, d, f, out_rgb, outputs, callback, user, cancelled, cancel_user);
    });
}

} // extern "C"
