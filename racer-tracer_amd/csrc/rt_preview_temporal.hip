// rt_preview_temporal.hip — jittered preview frames accumulated into a full-resolution history, behind rt_preview_phase,
// rt_preview_phase_camera, rt_preview_accumulate_device and rt_render_preview_temporal (include/rt_preview_temporal.h).
// DESIGN.md section 4.14:
//   phase    the pixel (jx, jy) of its block that this frame's preview traced (rt_plan.h: preview_phase; the shift is a
//            camera's, preview_phase_camera); sampled(p): p inside the cover with x mod step_x == jx, y mod step_y == jy;
//   history  k_temporal_accumulate's re-projection and taps (rt_history_taps.h: history_value<true>, the function that
//            kernel calls with <false>), and a tap's length must be > 0;
//   pixel    sampled with history: 4.11's blend; sampled without: fresh, length 1; not sampled with history: carried,
//            value, moments and length as the taps give them; neither: a FILL, 4.13's blend of the four anchors around p
//            on the grid shifted by the phase (guides read at the anchors' own pixels, colour at their blocks' top-left
//            pixels), stored before its re-modulation, with moments (l, l^2) and length exactly 0.
// Everything is f64, lane = pixel, 16x16 pixels per block as the other filter kernels; taps are read straight from global
// memory.  tests/preview_temporal_model.py restates it in this order.  The sampled pixel's blend and the stores are
// rt_history_taps.h's too, and the fill's four anchors are rt_filter_taps.h's anchor_blend, which k_upsample_preview calls at
// phase (0, 0): identities (a) and (b) of 4.14 hold because each side of them is the same function.
//
// Compiled once, with the fast arithmetic, like rt_denoise.hip.
#include "rt_filter_taps.h"
#include "rt_history_taps.h"
#include "rt_scene.h"
#include "rt_temporal_state.h"
#include "../../include/rt_preview_temporal.h"

#include <cmath>
#include <cstring>

namespace RT_KNS {

struct PreviewAccumulateArgs {
    int width, height;
    int step_x, step_y, gx, gy, cover_w, cover_h; // the preview's grid; gx, gy >= 1: anchors per row and column
    int jx, jy;                                   // 0 <= jx < step_x, 0 <= jy < step_y
    int has_prev, demodulate;
    double o[3], ulc[3], hor[3], ver[3]; // the previous (unshifted) camera
    double alpha, alpha_moments, max_history;
    double normal_tol2; // normal_tolerance^2
    double plane_tol;
    double inv_sn2; // the fill's stops, as k_upsample_preview's: 1 / sigma_n^2, or 0: the normal stop is off
    double inv_sx;  // 1 / (sigma_x * max(step_x, step_y)), or 0: the plane stop is off
};

// One pixel of the accumulation.  Every index into the frame, the guides and the output is that of a pixel of the image:
// p itself, an anchor's own pixel (i step_x + jx, j step_y + jy) < cover, its block's top-left pixel, or p clamped into the
// cover (the anchors' indices are formed in anchor_blend).  Indices into the previous history are formed in history_value,
// after its range tests on doubles.
__global__ __launch_bounds__(256) void k_preview_accumulate(const PreviewAccumulateArgs P, const double *__restrict__ g,
                                                            const RtGuides G, const RtHistory prev, const RtHistory out) {
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= P.width || py >= P.height) return;
    const size_t p = (size_t)py * (size_t)P.width + (size_t)px;

    // the pixel's own sample, first and in k_temporal_accumulate's order (the frame is replicated: p holds its block's value)
    double c[3];
    for (int k = 0; k < 3; ++k) c[k] = demodulated(g[3 * p + k], G.albedo[3 * p + k], P.demodulate);
    const d3 cp = mk(c[0], c[1], c[2]);
    const double lp = luminance(cp);
    const int id = G.obj_id[p];
    const d3 np = ld3(G.normal + 3 * p), xp = ld3(G.position + 3 * p);
    const bool sampled = px < P.cover_w && py < P.cover_h && px % P.step_x == P.jx && py % P.step_y == P.jy;
    HistorySums h;
    const bool has_h = P.has_prev && id >= 0 && history_value<true>(P, G, prev, p, id, np, xp, h);

    HistoryPixel v = fresh_pixel(cp, lp);
    if (sampled) { // k_temporal_accumulate's pixel
        if (has_h) v = blended_pixel(P, h, cp, lp);
    } else if (has_h) { // carried; the length by a division of sums of its own: taps that share a length carry exactly it
        v.rad = h.c * h.inv;
        v.m1 = h.m1 * h.inv;
        v.m2 = h.m2 * h.inv;
        v.len = h.len_rn / h.w_rn;
    } else { // a fill: k_upsample_preview's blend on the shifted grid, before its re-modulation and square root
        const AnchorBlend a = anchor_blend(P, P.jx, P.jy, g, G, px, py, p, id, np, xp);
        if (a.wsum > 0.0) {
            v.rad = mk(a.acc.x / a.wsum, a.acc.y / a.wsum, a.acc.z / a.wsum);
        } else { // no anchor qualifies: the frame at p, or where p is outside the cover (the frame holds 0 there) at the
                 // nearest covered pixel, demodulated by p's own albedo
            const size_t qc = (size_t)min(py, P.cover_h - 1) * (size_t)P.width + (size_t)min(px, P.cover_w - 1);
            v.rad = mk(demodulated(g[3 * qc + 0], G.albedo[3 * p + 0], P.demodulate),
                       demodulated(g[3 * qc + 1], G.albedo[3 * p + 1], P.demodulate),
                       demodulated(g[3 * qc + 2], G.albedo[3 * p + 2], P.demodulate));
        }
        v.m1 = luminance(v.rad);
        v.m2 = v.m1 * v.m1;
        v.len = 0.0;
    }
    store_history(out, p, v, np, xp, id);
}

} // namespace RT_KNS

// ------------------------------------------------------------------------------------------------------------ host side
using rtapi::fail;

namespace {

int check_phase(const rtapi::PreviewGrid &g, int32_t jx, int32_t jy) {
    if (jx < 0 || jx >= g.step_x || jy < 0 || jy >= g.step_y)
        return fail(RT_ERR_INVALID_ARGUMENT, "the phase (jx, jy) must lie inside the preview's block: 0 <= jx < step_x, 0 <= jy < step_y");
    return RT_OK;
}

int preview_phase(const RtRenderParams *p, int64_t frame_index, int32_t *jx, int32_t *jy) {
    if (!jx || !jy) return fail(RT_ERR_INVALID_ARGUMENT, "jx/jy is NULL");
    int32_t grid[4];
    int rc = rt_preview_grid(p, &grid[0], &grid[1], &grid[2], &grid[3]); // its refusals about params are this call's
    if (rc != RT_OK) return rc;
    if (frame_index < 0) return fail(RT_ERR_INVALID_ARGUMENT, "frame_index must not be negative");
    const rtapi::PreviewPhase ph = rtapi::preview_phase(rtapi::preview_grid(p), frame_index);
    *jx = ph.jx;
    *jy = ph.jy;
    return RT_OK;
}

int preview_phase_camera(const RtCamera *camera, const RtRenderParams *p, int32_t jx, int32_t jy, RtCamera *out) {
    if (!camera || !out) return fail(RT_ERR_INVALID_ARGUMENT, "camera/out is NULL");
    int32_t grid[4];
    int rc = rt_preview_grid(p, &grid[0], &grid[1], &grid[2], &grid[3]);
    if (rc != RT_OK) return rc;
    if ((rc = check_phase(rtapi::preview_grid(p), jx, jy)) != RT_OK) return rc;
    *out = rtapi::preview_phase_camera(*camera, p->width, p->height, jx, jy);
    return RT_OK;
}

int enqueue_preview_accumulate(const RtRenderParams *p, const RtTemporalParams *t, const RtDenoiseParams *d, int jx, int jy,
                               const double *rgb, const RtGuides *g, const RtCamera *prev_camera, const RtHistory *prev,
                               const RtHistory *out, hipStream_t stream) {
    const rtapi::PreviewGrid pg = rtapi::preview_grid(p);
    RT_KNS::PreviewAccumulateArgs a;
    memset(&a, 0, sizeof a);
    rtapi::fill_upsample_args(a, p, d);
    rtapi::fill_history_args(a, t, prev_camera);
    a.cover_w = pg.cover_w;
    a.cover_h = pg.cover_h;
    a.jx = jx;
    a.jy = jy;
    hipLaunchKernelGGL(RT_KNS::k_preview_accumulate, rtapi::pixel_grid(p->width, p->height), dim3(256), 0, stream, a, rgb, *g,
                       prev ? *prev : *out, *out);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// What both accumulating entry points refuse about params, denoise and temporal; `full` as check_upsample's.
int check_preview_temporal(const RtRenderParams *p, const RtTemporalParams *t, const RtDenoiseParams *d, RtRenderParams &full) {
    int rc = rtapi::check_upsample(p, d, full);
    if (rc != RT_OK) return rc;
    return rtapi::check_temporal(t);
}

int preview_accumulate_device(RtScene *s, const RtRenderParams *p, const RtTemporalParams *t, const RtDenoiseParams *d, int32_t jx,
                              int32_t jy, const double *rgb, const RtGuides *g, const RtCamera *prev_camera, const RtHistory *prev,
                              const RtHistory *out, void *stream) {
    RtRenderParams full;
    int rc = check_preview_temporal(p, t, d, full);
    if (rc != RT_OK) return rc;
    if ((rc = check_phase(rtapi::preview_grid(p), jx, jy)) != RT_OK) return rc;
    if ((rc = rtapi::check_accumulate_buffers(rgb, g, prev_camera, prev, out)) != RT_OK) return rc;
    if ((rc = rtapi::use_scene_device(s)) != RT_OK) return rc;
    return enqueue_preview_accumulate(p, t, d, jx, jy, rgb, g, prev_camera, prev, out, (hipStream_t)stream);
}

int render_preview_temporal(RtScene *s, RtTemporal *t, const RtCamera *camera, const RtRenderParams *p, const RtTemporalParams *tp,
                            const RtDenoiseParams *d, int64_t frame_index, double *out_rgb, double *out_length) {
    RtRenderParams full;
    int rc = check_preview_temporal(p, tp, d, full);
    if (rc != RT_OK) return rc;
    if ((rc = rtapi::check_params(camera, p)) != RT_OK) return rc;
    if (frame_index < 0) return fail(RT_ERR_INVALID_ARGUMENT, "frame_index must not be negative");
    // the frame of the phase camera at the preview's params; the guides and the levels of the caller's camera at scale 0
    const rtapi::PreviewPhase ph = rtapi::preview_phase(rtapi::preview_grid(p), frame_index);
    const RtCamera shifted = rtapi::preview_phase_camera(*camera, p->width, p->height, ph.jx, ph.jy);
    const auto accumulate = [&](const double *frame, const RtGuides *g, const RtCamera *prev_camera, const RtHistory *prev,
                                const RtHistory *out, hipStream_t stream) {
        return enqueue_preview_accumulate(p, tp, d, ph.jx, ph.jy, frame, g, prev_camera, prev, out, stream);
    };
    return rtapi::render_into_state(s, t, "rt_render_preview_temporal needs the pooled kernel: the v1 kernel has no preview mode",
                                    camera, &shifted, p, &full, tp, d, accumulate, out_rgb, out_length);
}

} // namespace

extern "C" {

int rt_preview_phase(const RtRenderParams *p, int64_t frame_index, int32_t *jx, int32_t *jy) {
    return rtapi::guarded("rt_preview_phase", [&] { return preview_phase(p, frame_index, jx, jy); });
}

int rt_preview_phase_camera(const RtCamera *camera, const RtRenderParams *p, int32_t jx, int32_t jy, RtCamera *out) {
    return rtapi::guarded("rt_preview_phase_camera", [&] { return preview_phase_camera(camera, p, jx, jy, out); });
}

int rt_preview_accumulate_device(RtScene *s, const RtRenderParams *p, const RtTemporalParams *t, const RtDenoiseParams *d, int32_t jx,
                                 int32_t jy, const double *rgb_device, const RtGuides *guides_device, const RtCamera *prev_camera,
                                 const RtHistory *prev_history, const RtHistory *out_history, void *hip_stream) {
    return rtapi::guarded("rt_preview_accumulate_device", [&] {
        return preview_accumulate_device(s, p, t, d, jx, jy, rgb_device, guides_device, prev_camera, prev_history, out_history,
                                         hip_stream);
    });
}

int rt_render_preview_temporal(RtScene *s, RtTemporal *t, const RtCamera *camera, const RtRenderParams *p, const RtTemporalParams *tp,
                               const RtDenoiseParams *d, int64_t frame_index, double *out_rgb_host, double *out_length_host) {
    return rtapi::guarded("rt_render_preview_temporal",
                          [&] { return render_preview_temporal(s, t, camera, p, tp, d, frame_index, out_rgb_host, out_length_host); });
}

} // extern "C"
