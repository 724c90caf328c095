// rt_upsample.hip — the scaled preview frame upsampled with full-resolution guides, behind rt_preview_grid,
// rt_upsample_preview_device and rt_render_preview_upsampled (include/rt_preview.h).  DESIGN.md section 4.13:
//   grid     step, cover as rt_plan.h's preview_grid; GX = W / step_x, GY = H / step_y; anchor (i, j) is the pixel
//            (i step_x, j step_y), whose traced value the preview frame holds (replicated over its block);
//   pixel    i0 = min(x / step_x, GX - 1), i1 = min(i0 + 1, GX - 1), tx = (x - i0 step_x) / step_x (0 when i1 == i0), rows
//            likewise; the taps (j0,i0) (j0,i1) (j1,i0) (j1,i1) with b = by bx, bx in {1 - tx, tx}, by in {1 - ty, ty};
//            a tap with b == 0 or another obj_id is skipped; w = b w_n w_x (rt_filter_taps.h: guide_stops) with
//            inv_sx = 1 / (sigma_plane max(step_x, step_y)); value g_q^2 (/ max(albedo_q, 1e-3));
//   output   sqrt(max(acc / wsum (* albedo_p), 0)), or with wsum == 0 the input at anchor (j0, i0), bit for bit.
// Everything is f64, lane = pixel, 16x16 pixels per block as the other filter kernels; the four taps (10 doubles each)
// are read straight from global memory.  tests/upsample_model.py restates it in this order.  The taps' loop is
// rt_filter_taps.h's anchor_blend at phase (0, 0); k_preview_accumulate's fill (rt_preview_temporal.hip) is the same
// function at a frame's phase.
//
// Compiled once, with the fast arithmetic, like rt_denoise.hip.
#include "rt_filter_taps.h"
#include "rt_scene.h"
#include "../../include/rt_preview.h"

#include <cmath>

namespace RT_KNS {

struct UpsampleArgs {
    int width, height, step_x, step_y, gx, gy; // gx, gy >= 1: anchors per row and column
    int demodulate;
    double inv_sn2; // 1 / sigma_n^2, or 0: the normal stop is off
    double inv_sx;  // 1 / (sigma_x * max(step_x, step_y)), or 0: the plane stop is off
};

__global__ __launch_bounds__(256) void k_upsample_preview(const UpsampleArgs P, const double *__restrict__ rgb, const RtGuides G,
                                                          double *__restrict__ out) {
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= P.width || py >= P.height) return;
    const size_t p = (size_t)py * (size_t)P.width + (size_t)px;

    // the anchors around p on the unshifted grid: columns i0 <= i1 < gx, rows j0 <= j1 < gy, all of them pixels inside the
    // covered area (rt_filter_taps.h)
    const int id = G.obj_id[p];
    const d3 np = ld3(G.normal + 3 * p), xp = ld3(G.position + 3 * p);
    const AnchorBlend a = anchor_blend(P, 0, 0, rgb, G, px, py, p, id, np, xp);
    if (a.wsum > 0.0) {
        d3 L = mk(a.acc.x / a.wsum, a.acc.y / a.wsum, a.acc.z / a.wsum);
        if (P.demodulate) L = mk(L.x * G.albedo[3 * p + 0], L.y * G.albedo[3 * p + 1], L.z * G.albedo[3 * p + 2]);
        out[3 * p + 0] = sqrt(fmax(L.x, 0.0));
        out[3 * p + 1] = sqrt(fmax(L.y, 0.0));
        out[3 * p + 2] = sqrt(fmax(L.z, 0.0));
    } else { // no anchor qualifies: the block's own anchor, as the replicated preview has it
        const size_t q = (size_t)(a.j0 * P.step_y) * (size_t)P.width + (size_t)(a.i0 * P.step_x);
        out[3 * p + 0] = rgb[3 * q + 0];
        out[3 * p + 1] = rgb[3 * q + 1];
        out[3 * p + 2] = rgb[3 * q + 2];
    }
}

} // namespace RT_KNS

// ------------------------------------------------------------------------------------------------------------ host side
using rtapi::fail;

// (rt_scene.h) what both upsampling entry points, and rt_preview_temporal.hip's, refuse about params and denoise
int rtapi::check_upsample(const RtRenderParams *p, const RtDenoiseParams *d, RtRenderParams &full) {
    if (!p || !d) return fail(RT_ERR_INVALID_ARGUMENT, "params/denoise is NULL");
    if (p->scale <= 1) return fail(RT_ERR_INVALID_ARGUMENT, "params->scale must be greater than 1: there is no preview to upsample");
    if (p->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "the preview is a whole frame: params->strip_count must be 0 or 1");
    full = *p;
    full.scale = 0;
    int rc = rtapi::check_denoise(&full, d);
    if (rc != RT_OK) return rc;
    const rtapi::PreviewGrid g = rtapi::preview_grid(p);
    if (p->width / g.step_x < 1 || p->height / g.step_y < 1) // (tiles_w > width: a block larger than the image)
        return fail(RT_ERR_INVALID_ARGUMENT, "params->tiles_w / tiles_h leave the preview without an anchor pixel");
    return RT_OK;
}

namespace {

using rtapi::check_upsample;

// What the three entry points refuse about params: NULL aside, rt_render_frame's rules for the fields the grid reads.
int check_grid_params(const RtRenderParams *p) {
    if (p->width < 2 || p->height < 2) return fail(RT_ERR_INVALID_ARGUMENT, "width and height must be at least 2");
    if ((uint64_t)p->width * (uint64_t)p->height > 0xFFFFFFFFull) return fail(RT_ERR_INVALID_ARGUMENT, "image too large for the pixel counter");
    if (p->scale < 0) return fail(RT_ERR_INVALID_ARGUMENT, "scale must not be negative");
    if (p->scale > 1 && p->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "the preview scale cannot be combined with strips: params->strip_count must be 0 or 1");
    return RT_OK;
}

int preview_grid(const RtRenderParams *p, int32_t *step_x, int32_t *step_y, int32_t *cover_w, int32_t *cover_h) {
    if (!p || !step_x || !step_y || !cover_w || !cover_h) return fail(RT_ERR_INVALID_ARGUMENT, "params/step_x/step_y/cover_w/cover_h is NULL");
    int rc = check_grid_params(p);
    if (rc != RT_OK) return rc;
    const rtapi::PreviewGrid g = rtapi::preview_grid(p);
    *step_x = g.step_x;
    *step_y = g.step_y;
    *cover_w = g.cover_w;
    *cover_h = g.cover_h;
    return RT_OK;
}

int enqueue_upsample(const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb, const RtGuides &g, double *out,
                     hipStream_t stream) {
    RT_KNS::UpsampleArgs a;
    rtapi::fill_upsample_args(a, p, d);
    hipLaunchKernelGGL(RT_KNS::k_upsample_preview, rtapi::pixel_grid(p->width, p->height), dim3(256), 0, stream, a, rgb, g, out);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int upsample_preview_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb, const RtGuides *g,
                            double *out, void *stream) {
    RtRenderParams full;
    int rc = check_upsample(p, d, full);
    if (rc != RT_OK) return rc;
    if (!rgb || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_device/out_device is NULL");
    if (rgb == out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_device and out_device must differ");
    if (!rtapi::guides_complete(g)) return fail(RT_ERR_INVALID_ARGUMENT, "guides_device or one of its planes is NULL");
    if ((rc = rtapi::use_scene_device(s)) != RT_OK) return rc;
    return enqueue_upsample(p, d, rgb, *g, out, (hipStream_t)stream);
}

int render_preview_upsampled(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtDenoiseParams *d, double *out_rgb,
                             double *out_preview) {
    RtRenderParams full;
    int rc = check_upsample(p, d, full);
    if (rc != RT_OK) return rc;
    if ((rc = rtapi::check_params(camera, p)) != RT_OK) return rc;
    if (!out_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgb_host is NULL");
    if (out_rgb == out_preview) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgb_host and out_preview_host must differ");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (s->use_v1) return fail(RT_ERR_UNSUPPORTED, "rt_render_preview_upsampled needs the pooled kernel: the v1 kernel has no preview mode");
    RT_HIP(hipSetDevice(s->device));
    const size_t pixels = (size_t)p->width * (size_t)p->height, n = 3 * pixels;
    rtapi::RenderBuffers &b = s->buf;
    if ((rc = rtapi::reserve_denoise(s, pixels, true)) != RT_OK) return rc;
    RT_HIP(b.frame.reserve(3 * n));
    const hipStream_t stream = b.stream;
    double *preview = b.frame.ptr, *upsampled = preview + n, *result = upsampled;
    const RtGuides g = rtapi::scene_guides(s, pixels);
    if ((rc = rtapi::enqueue_render(s, camera, p, preview, stream, 0, rtapi::Cancel())) != RT_OK) return rc;
    if ((rc = rtapi::enqueue_guides(s, camera, &full, g, stream)) != RT_OK) return rc;
    if ((rc = enqueue_upsample(p, d, preview, g, upsampled, stream)) != RT_OK) return rc;
    if (d->iterations > 0) {
        result = upsampled + n;
        if ((rc = rtapi::enqueue_denoise(s, &full, d, upsampled, g, result, stream)) != RT_OK) return rc;
    }
    RT_HIP(hipMemcpyAsync(out_rgb, result, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (out_preview) RT_HIP(hipMemcpyAsync(out_preview, preview, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_preview_grid(const RtRenderParams *p, int32_t *step_x, int32_t *step_y, int32_t *cover_w, int32_t *cover_h) {
    return rtapi::guarded("rt_preview_grid", [&] { return preview_grid(p, step_x, step_y, cover_w, cover_h); });
}

int rt_upsample_preview_device(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb_device,
                               const RtGuides *guides_device, double *out_device, void *hip_stream) {
    return rtapi::guarded("rt_upsample_preview_device", [&] { return upsample_preview_device(s, p, d, rgb_device, guides_device, out_device, hip_stream); });
}

int rt_render_preview_upsampled(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtDenoiseParams *d,
                                double *out_rgb_host, double *out_preview_host) {
    return rtapi::guarded("rt_render_preview_upsampled", [&] { return render_preview_upsampled(s, camera, p, d, out_rgb_host, out_preview_host); });
}

} // extern "C"
