// rt_preview_temporal.hip — jittered preview frames accumulated into a full-resolution history, behind rt_preview_phase,
// rt_preview_phase_camera, rt_preview_accumulate_device and rt_render_preview_temporal (include/rt_preview_temporal.h).
// DESIGN.md section 4.14:
//   phase    the pixel (jx, jy) of its block that this frame's preview traced (rt_plan.h: preview_phase; the shift is a
//            camera's, preview_phase_camera); sampled(p): p inside the cover with x mod step_x == jx, y mod step_y == jy;
//   history  k_temporal_accumulate's re-projection and taps (restated in history_value), and a tap's length must be > 0;
//   pixel    sampled with history: 4.11's blend; sampled without: fresh, length 1; not sampled with history: carried,
//            value, moments and length as the taps give them; neither: a FILL, 4.13's blend of the four anchors around p
//            on the grid shifted by the phase (guides read at the anchors' own pixels, colour at their blocks' top-left
//            pixels), stored before its re-modulation, with moments (l, l^2) and length exactly 0.
// Everything is f64, lane = pixel, 16x16 pixels per block as the other filter kernels; taps are read straight from global
// memory.  tests/preview_temporal_model.py restates it in this order.
//
// Compiled once, with the fast arithmetic, like rt_denoise.hip.
#include "rt_filter_taps.h"
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

__device__ __forceinline__ d3 cross3(d3 a, d3 b) {
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// the taps' weighted sums and 1 / their weight: a value is sum * inv, formed where it is used, as the twin forms it
struct HistorySums {
    d3 c;          // radiance
    double m1, m2; // luminance moments
    double len;    // history length
    double inv;
    double len_rn, w_rn; // the length's sum and the weight again, every product and sum rounded on its own (exact_tap)
};

// One tap's share of a CARRIED length.  The twin's sums above may be contracted into fused multiply-adds as the compiler
// sees fit (sum(w L) and sum(w) then round differently, and a pixel whose taps all have length L would carry L only to
// rounding); these are not: w = round(a b), len_rn += round(w L), w_rn += w.  Where the taps share one length L that is a
// power of two every product is exact, len_rn == L w_rn, and the quotient is L itself whatever the weights' last bits are.
__device__ __forceinline__ void exact_tap(double a, double b, double lq, double &len_rn, double &w_rn) {
#pragma clang fp contract(off)
    const double w = a * b;
    len_rn = len_rn + w * lq;
    w_rn = w_rn + w;
}

// The history value of one pixel.  TWIN of the re-projection and tap loop of k_temporal_accumulate (rt_temporal.hip),
// statement for statement, with one more condition on a tap: its length must be > 0, so that a fill is never read as
// history.  The loop is stated twice because moving it into a function shared by both kernels did not leave
// k_temporal_accumulate's instructions as they were (profiles/preview_temporal_shared_loop_counts.txt); identity (b) of
// DESIGN.md 4.14, tested on the device bit for bit, pins the two together.  As there, whether a tap exists is decided on
// doubles: no index is formed, and nothing of the previous history is loaded, before the re-projected position is known to
// be finite and within one pixel of the previous image, and every tap is bounds-checked on its own.
// false: the hit point is behind or outside the previous image, or the taps that agree weigh less than 1e-3.
__device__ __forceinline__ bool history_value(const PreviewAccumulateArgs &P, const RtGuides &G, const RtHistory &prev, size_t p,
                                              int id, d3 np, d3 xp, HistorySums &h) {
    // ulc + u hor - v ver - o = s (x - o): columns hor, -ver, -(x - o) against o - ulc
    const d3 o = ld3(P.o);
    const d3 a = ld3(P.hor), b = -ld3(P.ver), cc = -(xp - o), r = o - ld3(P.ulc);
    const d3 bxc = cross3(b, cc);
    const double det = dot(a, bxc);
    const double u = dot(r, bxc) / det;
    const double v = dot(a, cross3(r, cc)) / det;
    const double s = dot(a, cross3(b, r)) / det;
    const double fx = u * (double)(P.width - 1) - 0.5;
    const double fy = v * (double)(P.height - 1) - 0.5;
    // (a NaN fails every comparison below)
    const bool inside = det != 0.0 && s > 0.0 && fx >= -1.0 && fx <= (double)P.width && fy >= -1.0 && fy <= (double)P.height;
    if (!inside) return false;
    const double flx = floor(fx), fly = floor(fy);
    const int x0 = (int)flx, y0 = (int)fly; // in [-1, W] and [-1, H]
    const double tx = fx - flx, ty = fy - fly;
    const double fp = G.footprint[p];
    d3 ch = mk(0.0, 0.0, 0.0);
    double mh1 = 0.0, mh2 = 0.0, lh = 0.0, wsum = 0.0;
    h.len_rn = h.w_rn = 0.0;
    for (int j = 0; j < 2; ++j) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= P.height) continue;
        for (int i = 0; i < 2; ++i) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= P.width) continue;
            const size_t q = (size_t)qy * (size_t)P.width + (size_t)qx;
            if (prev.obj_id[q] != id) continue;
            const d3 dn = np - ld3(prev.normal + 3 * q);
            if (!(len2(dn) <= P.normal_tol2)) continue;
            const double dist = dot(np, ld3(prev.position + 3 * q) - xp);
            if (!(fabs(dist) <= P.plane_tol * fp)) continue;
            const double lq = prev.length[q];
            if (!(lq > 0.0)) continue; // a fill
            const double w = (i ? tx : 1.0 - tx) * (j ? ty : 1.0 - ty);
            ch = ch + w * ld3(prev.radiance + 3 * q);
            mh1 += w * prev.moments[2 * q + 0];
            mh2 += w * prev.moments[2 * q + 1];
            lh += w * lq;
            wsum += w;
            exact_tap(i ? tx : 1.0 - tx, j ? ty : 1.0 - ty, lq, h.len_rn, h.w_rn);
        }
    }
    if (!(wsum >= 1e-3)) return false;
    h.c = ch;
    h.m1 = mh1;
    h.m2 = mh2;
    h.len = lh;
    h.inv = 1.0 / wsum;
    return true;
}

// (i0, i1, t) of one axis of the shifted grid: the anchors of column i sit at x = i step + j
__device__ __forceinline__ void shifted_axis(int x, int j, int step, int count, int &i0, int &i1, double &t) {
    const int xs = x - j;
    i0 = xs < 0 ? 0 : min(xs / step, count - 1);
    i1 = min(i0 + 1, count - 1);
    t = (xs < 0 || i1 == i0) ? 0.0 : (double)(xs - i0 * step) / (double)step;
}

// One pixel of the accumulation.  Every index into the frame, the guides and the output is that of a pixel of the image:
// p itself, an anchor's own pixel (i step_x + jx, j step_y + jy) < cover, its block's top-left pixel, or p clamped into the
// cover.  Indices into the previous history are formed in history_value, after its range tests on doubles.
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
    const bool has_h = P.has_prev && id >= 0 && history_value(P, G, prev, p, id, np, xp, h);

    d3 rad = cp;
    double m1 = lp, m2 = lp * lp, len = 1.0;
    if (sampled) { // k_temporal_accumulate's pixel
        if (has_h) {
            const double inv = h.inv;
            const double N = h.len * inv + 1.0;
            const double al = fmax(1.0 / N, P.alpha), am = fmax(1.0 / N, P.alpha_moments);
            rad = (1.0 - al) * (h.c * inv) + al * cp;
            m1 = (1.0 - am) * (h.m1 * inv) + am * lp;
            m2 = (1.0 - am) * (h.m2 * inv) + am * (lp * lp);
            len = fmin(N, P.max_history);
        }
    } else if (has_h) { // carried; the length by a division of sums of its own: taps that share a length carry exactly it
        rad = h.c * h.inv;
        m1 = h.m1 * h.inv;
        m2 = h.m2 * h.inv;
        len = h.len_rn / h.w_rn;
    } else { // a fill: k_upsample_preview's blend on the shifted grid, before its re-modulation and square root
        int i0, i1, j0, j1;
        double tx, ty;
        shifted_axis(px, P.jx, P.step_x, P.gx, i0, i1, tx);
        shifted_axis(py, P.jy, P.step_y, P.gy, j0, j1, ty);
        const int qi[2] = {i0, i1}, qj[2] = {j0, j1};
        const double bx[2] = {1.0 - tx, tx}, by[2] = {1.0 - ty, ty};
        const double inv_fx = P.inv_sx / G.footprint[p]; // a miss has footprint inf: 0
        d3 acc = mk(0.0, 0.0, 0.0);
        double wsum = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double b = by[k >> 1] * bx[k & 1];
            if (b == 0.0) continue;
            const int ay = qj[k >> 1] * P.step_y, ax = qi[k & 1] * P.step_x; // the block's top-left pixel: the colour
            const size_t qc = (size_t)ay * (size_t)P.width + (size_t)ax;
            const size_t q = (size_t)(ay + P.jy) * (size_t)P.width + (size_t)(ax + P.jx); // the pixel it traced: the guides
            if (G.obj_id[q] != id) continue; // (-1 == -1: sky interpolates between sky anchors)
            const double w = guide_stops(b, P.inv_sn2, P.inv_sx, inv_fx, np, xp, G, q);
            const d3 v = mk(demodulated(g[3 * qc + 0], G.albedo[3 * q + 0], P.demodulate),
                            demodulated(g[3 * qc + 1], G.albedo[3 * q + 1], P.demodulate),
                            demodulated(g[3 * qc + 2], G.albedo[3 * q + 2], P.demodulate));
            acc = acc + w * v;
            wsum += w;
        }
        if (wsum > 0.0) {
            rad = mk(acc.x / wsum, acc.y / wsum, acc.z / wsum);
        } else { // no anchor qualifies: the frame at p, or where p is outside the cover (the frame holds 0 there) at the
                 // nearest covered pixel, demodulated by p's own albedo
            const size_t qc = (size_t)min(py, P.cover_h - 1) * (size_t)P.width + (size_t)min(px, P.cover_w - 1);
            rad = mk(demodulated(g[3 * qc + 0], G.albedo[3 * p + 0], P.demodulate),
                     demodulated(g[3 * qc + 1], G.albedo[3 * p + 1], P.demodulate),
                     demodulated(g[3 * qc + 2], G.albedo[3 * p + 2], P.demodulate));
        }
        m1 = luminance(rad);
        m2 = m1 * m1;
        len = 0.0;
    }
    out.radiance[3 * p + 0] = rad.x;
    out.radiance[3 * p + 1] = rad.y;
    out.radiance[3 * p + 2] = rad.z;
    out.moments[2 * p + 0] = m1;
    out.moments[2 * p + 1] = m2;
    out.length[p] = len;
    out.normal[3 * p + 0] = np.x;
    out.normal[3 * p + 1] = np.y;
    out.normal[3 * p + 2] = np.z;
    out.position[3 * p + 0] = xp.x;
    out.position[3 * p + 1] = xp.y;
    out.position[3 * p + 2] = xp.z;
    out.obj_id[p] = id;
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
    const rtapi::FilterStops st = rtapi::filter_stops(d);
    RT_KNS::PreviewAccumulateArgs a;
    memset(&a, 0, sizeof a);
    a.width = p->width;
    a.height = p->height;
    a.step_x = pg.step_x;
    a.step_y = pg.step_y;
    a.gx = p->width / pg.step_x;
    a.gy = p->height / pg.step_y;
    a.cover_w = pg.cover_w;
    a.cover_h = pg.cover_h;
    a.jx = jx;
    a.jy = jy;
    a.has_prev = prev != nullptr;
    a.demodulate = (d->flags & RT_DENOISE_DEMODULATE) != 0;
    if (prev_camera) {
        memcpy(a.o, prev_camera->origin, sizeof a.o);
        memcpy(a.ulc, prev_camera->upper_left_corner, sizeof a.ulc);
        memcpy(a.hor, prev_camera->horizontal, sizeof a.hor);
        memcpy(a.ver, prev_camera->vertical, sizeof a.ver);
    }
    a.alpha = t->alpha;
    a.alpha_moments = t->alpha_moments;
    a.max_history = t->max_history;
    a.normal_tol2 = t->normal_tolerance * t->normal_tolerance;
    a.plane_tol = t->plane_tolerance;
    a.inv_sn2 = st.inv_sn2;
    a.inv_sx = d->sigma_plane > 0.0 ? 1.0 / (d->sigma_plane * (double)(pg.step_x > pg.step_y ? pg.step_x : pg.step_y)) : 0.0;
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
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    RT_HIP(hipSetDevice(s->device));
    return enqueue_preview_accumulate(p, t, d, jx, jy, rgb, g, prev_camera, prev, out, (hipStream_t)stream);
}

int render_preview_temporal(RtScene *s, RtTemporal *t, const RtCamera *camera, const RtRenderParams *p, const RtTemporalParams *tp,
                            const RtDenoiseParams *d, int64_t frame_index, double *out_rgb, double *out_length) {
    RtRenderParams full;
    int rc = check_preview_temporal(p, tp, d, full);
    if (rc != RT_OK) return rc;
    if ((rc = rtapi::check_params(camera, p)) != RT_OK) return rc;
    if (frame_index < 0) return fail(RT_ERR_INVALID_ARGUMENT, "frame_index must not be negative");
    if (!out_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgb_host is NULL");
    if (!t) return fail(RT_ERR_INVALID_ARGUMENT, "temporal_state is NULL");
    if (p->width != t->width || p->height != t->height)
        return fail(RT_ERR_INVALID_ARGUMENT, "params->width and height must be the RtTemporal's");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (s->device != t->device) return fail(RT_ERR_INVALID_ARGUMENT, "the scene and the RtTemporal must be on the same device");
    if (s->use_v1) return fail(RT_ERR_UNSUPPORTED, "rt_render_preview_temporal needs the pooled kernel: the v1 kernel has no preview mode");
    RT_HIP(hipSetDevice(s->device));
    const size_t pixels = (size_t)p->width * (size_t)p->height, n = 3 * pixels;
    const hipStream_t stream = s->buf.stream;
    const rtapi::PreviewPhase ph = rtapi::preview_phase(rtapi::preview_grid(p), frame_index);
    const RtCamera shifted = rtapi::preview_phase_camera(*camera, p->width, p->height, ph.jx, ph.jy);
    double *frame = rtapi::state_frame(t), *filtered = frame + n;
    const RtGuides g = rtapi::state_guides(t);
    const RtHistory prev = rtapi::state_history(t, t->current), next = rtapi::state_history(t, t->current ^ 1);
    if ((rc = rtapi::enqueue_render(s, &shifted, p, frame, stream, 0, rtapi::Cancel())) != RT_OK) return rc;
    if ((rc = rtapi::enqueue_guides(s, camera, &full, g, stream)) != RT_OK) return rc;
    if ((rc = enqueue_preview_accumulate(p, tp, d, ph.jx, ph.jy, frame, &g, t->has_prev ? &t->camera : nullptr,
                                         t->has_prev ? &prev : nullptr, &next, stream)) != RT_OK)
        return rc;
    if ((rc = rtapi::enqueue_denoise_history(s, &full, d, tp, &next, &g, filtered, stream)) != RT_OK) return rc;
    RT_HIP(hipMemcpyAsync(out_rgb, filtered, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (out_length) RT_HIP(hipMemcpyAsync(t->host_length, next.length, pixels * sizeof(double), hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    if (out_length) memcpy(out_length, t->host_length, pixels * sizeof(double));
    t->current ^= 1;
    t->has_prev = true;
    t->camera = *camera;
    return RT_OK;
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
