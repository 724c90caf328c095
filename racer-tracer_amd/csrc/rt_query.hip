// rt_query.hip — the host side of every query on caller rays: closest / any hit (include/rt_rays.h),
// occlusion (include/rt_occlusion.h; 4.16), multi-hit (include/rt_multihit.h; 4.17) and, on caller points, ambient
// occlusion with its frame (include/rt_ambient.h; 4.18).  Each entry point states its own refusals and its launch
// (rt_rays_kernel.hip, rt_occlusion_kernel.hip, rt_multihit_kernel.hip, rt_ambient_kernel.hip); the refusals they share,
// the steps before a launch and the chunked host form (rt_query_stage.h) are stated once.
//
// Host code only (HIP runtime calls).  A query takes every scene rt_render_guides_device takes and follows its rules: the
// caller's stream, the tree when the scene walks one (use_bvh), and for a tree that renders keep in LDS its global copy,
// in whichever child order the last camera left it (a walk is correct in any order: rt_bvh_any.h, rt_bvh_kbest.h).
#include "rt_query_stage.h"

#include <cmath>
#include <cstring>

using rtapi::fail;

// The scene part of the render's argument block: fill_trace_args with a zeroed camera and 2 x 2 one-sample params, as
// enqueue_guides fills it with the caller's (the camera and the pixel grid are read by nothing in the three query kernels).
int rtapi::query_args(const RtScene *s, rtdev::TraceArgs &a) {
    RtCamera none;
    memset(&none, 0, sizeof none);
    RtRenderParams one;
    memset(&one, 0, sizeof one);
    one.width = one.height = 2;
    one.samples = one.max_depth = 1;
    one.tiles_w = one.tiles_h = 1;
    const int rc = rtapi::fill_trace_args(s, &none, &one, a);
    if (rc != RT_OK) return rc;
    if (!s->use_bvh) a.n_bvh_nodes = 0;
    return RT_OK;
}

// The device copy of RtScene.table_order, made by the scene's first query that names primitives.  A plain (synchronous)
// copy, once: a later query on another stream must not overtake it.
int rtapi::ensure_order(RtScene *s) {
    if (s->rays_order.count == s->table_order.size()) return RT_OK;
    RT_HIP(s->rays_order.alloc(s->table_order.size()));
    RT_HIP(hipMemcpy(s->rays_order.ptr, s->table_order.data(), s->table_order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return RT_OK;
}

namespace {

// What every query refuses behind its own refusals, without a device, the scene last so that each refusal names its own
// cause.  `either`: one message for a missing origin or direction (rt_trace_rays'), not one each.
int check_batch(const RtScene *s, const RtRays *rays, int64_t n, const char *either = nullptr) {
    if (n < 0 || n > (int64_t)INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "n must be in 0..INT32_MAX");
    // (an empty batch has no planes to look at: an empty tensor's address is NULL)
    if (n > 0 && either && (!rays->origin || !rays->direction)) return fail(RT_ERR_INVALID_ARGUMENT, either);
    if (n > 0 && !rays->origin) return fail(RT_ERR_INVALID_ARGUMENT, "rays->origin is NULL");
    if (n > 0 && !rays->direction) return fail(RT_ERR_INVALID_ARGUMENT, "rays->direction is NULL");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    return RT_OK;
}

int check_closest(const RtScene *s, const RtRays *rays, int64_t n, const RtRayQueryParams *q, const RtRayHits *hits) {
    if (!rays || !hits || !q) return fail(RT_ERR_INVALID_ARGUMENT, "rays/hits/query is NULL");
    if (q->mode != RT_RAYS_CLOSEST && q->mode != RT_RAYS_ANY) return fail(RT_ERR_INVALID_ARGUMENT, "query->mode must be RT_RAYS_CLOSEST or RT_RAYS_ANY");
    if (q->_reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, "query->_reserved must be 0");
    return check_batch(s, rays, n, "rays->origin/direction is NULL");
}

int check_occlusion(const RtScene *s, const RtRays *rays, int64_t n, const int32_t *occluded) {
    if (!rays) return fail(RT_ERR_INVALID_ARGUMENT, "rays is NULL");
    if (!occluded) return fail(RT_ERR_INVALID_ARGUMENT, "occluded is NULL");
    return check_batch(s, rays, n);
}

int check_multi(const RtScene *s, const RtRays *rays, int64_t n, const RtMultiHitParams *p, const RtRayHits *hits) {
    if (!rays) return fail(RT_ERR_INVALID_ARGUMENT, "rays is NULL");
    if (!p) return fail(RT_ERR_INVALID_ARGUMENT, "params is NULL");
    if (!hits) return fail(RT_ERR_INVALID_ARGUMENT, "hits is NULL");
    if (p->k < 1 || p->k > RT_MULTIHIT_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "params->k must be in 1..RT_MULTIHIT_MAX");
    if (p->_reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, "params->_reserved must be 0");
    return check_batch(s, rays, n);
}

// The ambient query's params, and the batch against them (index_base + n): every cause with its own message.
int check_ambient_params(const RtAmbientParams *p, int64_t n) {
    if (!p) return fail(RT_ERR_INVALID_ARGUMENT, "the ambient params are NULL");
    if (p->samples < 1 || p->samples > RT_AMBIENT_MAX_SAMPLES || (p->samples & (p->samples - 1)) != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "params->samples must be a power of two in 1..RT_AMBIENT_MAX_SAMPLES");
    if (p->_reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, "params->_reserved must be 0");
    if (!(p->bias >= 0.0) || !std::isfinite(p->bias)) return fail(RT_ERR_INVALID_ARGUMENT, "params->bias must be finite and not negative");
    if (!(p->radius >= p->bias)) return fail(RT_ERR_INVALID_ARGUMENT, "params->radius must not be NaN or below params->bias");
    if (p->index_base < 0 || p->index_base > ((int64_t)1 << 32) || (n > 0 && p->index_base + n > ((int64_t)1 << 32)))
        return fail(RT_ERR_INVALID_ARGUMENT, "params->index_base must be at least 0 and index_base + n at most 2^32");
    return RT_OK;
}

int check_ambient(const RtScene *s, const RtRays *points, int64_t n, const RtAmbientParams *p, const int32_t *open) {
    if (!points) return fail(RT_ERR_INVALID_ARGUMENT, "points is NULL");
    if (!open) return fail(RT_ERR_INVALID_ARGUMENT, "open is NULL");
    if (n < 0 || n > (int64_t)INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "n must be in 0..INT32_MAX");
    const int rc = check_ambient_params(p, n);
    if (rc != RT_OK) return rc;
    if (n > 0 && !points->origin) return fail(RT_ERR_INVALID_ARGUMENT, "points->origin is NULL");
    if (n > 0 && !points->direction) return fail(RT_ERR_INVALID_ARGUMENT, "points->direction (the normals) is NULL");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    return RT_OK;
}

// The frame forms: rt_render_guides_device's refusals (rt_denoise.hip), the ambient params for W * H points from index 0,
// the scene last.  `guides`: the caller's, or NULL for the host-output form, which brings the scene's own.
int check_ambient_frame(const RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtAmbientParams *ap, const RtGuides *guides,
                        bool own_guides, const double *out) {
    RtDenoiseParams none;
    rt_denoise_params_default(&none);
    int rc = rtapi::check_denoise(p, &none);
    if (rc != RT_OK) return rc;
    if (!own_guides && !rtapi::guides_complete(guides)) return fail(RT_ERR_INVALID_ARGUMENT, "guides_device or one of its planes is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    if ((rc = check_ambient_params(ap, (int64_t)p->width * (int64_t)p->height)) != RT_OK) return rc;
    if (ap->index_base != 0) return fail(RT_ERR_INVALID_ARGUMENT, "ambient->index_base must be 0 for a frame: pixel p is point p");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    return rtapi::check_params(camera, p);
}

// Behind an entry point's checks (`checked`: what they said) and before its launches: nothing for a refused or an empty
// batch — the caller returns `checked`, or RT_OK for n == 0, before a device is touched — else the scene's device, the
// argument block and, for a kernel that names primitives, the device copy of the table's order (so a scene's first
// occlusion call uploads nothing).
int begin_query(RtScene *s, int checked, int64_t n, bool names_prims, rtdev::TraceArgs &a) {
    if (checked != RT_OK || n == 0) return checked;
    RT_HIP(hipSetDevice(s->device));
    const int rc = rtapi::query_args(s, a);
    if (rc != RT_OK || !names_prims) return rc;
    return rtapi::ensure_order(s);
}

// the planes' entries per chunk of the host forms; a multi-hit ray takes up to RT_MULTIHIT_MAX of them
const size_t kPlane = (size_t)RT_RAYS_HOST_CHUNK;
static_assert(RT_RAYS_HOST_CHUNK % RT_MULTIHIT_MAX == 0, "a chunk of rt_trace_rays holds a whole number of multi-hit rays");

int trace_rays_device(RtScene *s, const RtRays *rays, int64_t n, const RtRayQueryParams *q, const RtRayHits *hits, void *stream) {
    rtdev::TraceArgs a;
    const int rc = begin_query(s, check_closest(s, rays, n, q, hits), n, true, a);
    if (rc != RT_OK || n == 0) return rc;
    RT_HIP(s->kernels->trace_rays(&a, rays, hits, s->rays_order.ptr, (int)n, q->mode == RT_RAYS_ANY, (hipStream_t)stream));
    return RT_OK;
}

int trace_rays_host(RtScene *s, const RtRays *rays, int64_t n, const RtRayQueryParams *q, const RtRayHits *hits) {
    rtdev::TraceArgs a;
    const int rc = begin_query(s, check_closest(s, rays, n, q, hits), n, true, a);
    if (rc != RT_OK || n == 0) return rc;
    return rtapi::stage_query(s->buf, kPlane, rays, (size_t)n, hits, 1, 1, nullptr, [&](const RtRays &dr, const RtRayHits &dh, int32_t *, int m) {
        return s->kernels->trace_rays(&a, &dr, &dh, s->rays_order.ptr, m, q->mode == RT_RAYS_ANY, s->buf.stream);
    });
}

int occlusion_device(RtScene *s, const RtRays *rays, int64_t n, int32_t *occluded, void *stream) {
    rtdev::TraceArgs a;
    const int rc = begin_query(s, check_occlusion(s, rays, n, occluded), n, false, a);
    if (rc != RT_OK || n == 0) return rc;
    RT_HIP(s->kernels->occlusion(&a, rays, occluded, (int)n, (hipStream_t)stream));
    return RT_OK;
}

int occlusion_host(RtScene *s, const RtRays *rays, int64_t n, int32_t *occluded) {
    rtdev::TraceArgs a;
    const int rc = begin_query(s, check_occlusion(s, rays, n, occluded), n, false, a);
    if (rc != RT_OK || n == 0) return rc;
    return rtapi::stage_query(s->buf, kPlane, rays, (size_t)n, nullptr, 1, 1, occluded, [&](const RtRays &dr, const RtRayHits &, int32_t *answers, int m) {
        return s->kernels->occlusion(&a, &dr, answers, m, s->buf.stream);
    });
}

int multi_device(RtScene *s, const RtRays *rays, int64_t n, const RtMultiHitParams *p, const RtRayHits *hits, int32_t *count, void *stream) {
    rtdev::TraceArgs a;
    const int rc = begin_query(s, check_multi(s, rays, n, p, hits), n, true, a);
    if (rc != RT_OK || n == 0) return rc;
    RT_HIP(s->kernels->multihit(&a, rays, hits, count, s->rays_order.ptr, (int)n, p->k, (hipStream_t)stream));
    return RT_OK;
}

int multi_host(RtScene *s, const RtRays *rays, int64_t n, const RtMultiHitParams *p, const RtRayHits *hits, int32_t *count) {
    rtdev::TraceArgs a;
    const int rc = begin_query(s, check_multi(s, rays, n, p, hits), n, true, a);
    if (rc != RT_OK || n == 0) return rc;
    return rtapi::stage_query(s->buf, kPlane, rays, (size_t)n, hits, (size_t)p->k, RT_MULTIHIT_MAX, count,
                              [&](const RtRays &dr, const RtRayHits &dh, int32_t *counts, int m) {
                                  return s->kernels->multihit(&a, &dr, &dh, counts, s->rays_order.ptr, m, p->k, s->buf.stream);
                              });
}

// `walked`: the header's rays_out_device (here a ray plane by that name is the staging buffer's, rt_query_stage.h)
int ambient_device(RtScene *s, const RtRays *points, int64_t n, const RtAmbientParams *p, int32_t *open, const RtAmbientRays *walked,
                   void *stream) {
    rtdev::TraceArgs a;
    const int rc = begin_query(s, check_ambient(s, points, n, p, open), n, false, a);
    if (rc != RT_OK || n == 0) return rc;
    RT_HIP(s->kernels->ambient(&a, points, (int)n, p, 0.0, open, nullptr, nullptr, walked, (hipStream_t)stream));
    return RT_OK;
}

int ambient_host(RtScene *s, const RtRays *points, int64_t n, const RtAmbientParams *p, int32_t *open) {
    rtdev::TraceArgs a;
    const int rc = begin_query(s, check_ambient(s, points, n, p, open), n, false, a);
    if (rc != RT_OK || n == 0) return rc;
    RtAmbientParams chunk = *p; // every chunk's launch names the index of its first point: the answer is the whole batch's
    return rtapi::stage_query(s->buf, kPlane, points, (size_t)n, nullptr, 1, 1, open, [&](const RtRays &dp, const RtRayHits &, int32_t *answers, int m) {
        const hipError_t e = s->kernels->ambient(&a, &dp, m, &chunk, 0.0, answers, nullptr, nullptr, nullptr, s->buf.stream);
        chunk.index_base += m;
        return e;
    });
}

// The guides of (camera, p) into g, then the query at every pixel into `out` (both device memory), on `stream`.
int enqueue_ambient_frame(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtAmbientParams *ap, const RtGuides &g, double *out,
                          hipStream_t stream) {
    int rc = rtapi::enqueue_guides(s, camera, p, g, stream);
    if (rc != RT_OK) return rc;
    rtdev::TraceArgs a;
    if ((rc = rtapi::query_args(s, a)) != RT_OK) return rc;
    RtRays points;
    points.origin = g.position;
    points.direction = g.normal;
    points.t_min = points.t_max = points.time = nullptr;
    const double mid = (camera->time_a + camera->time_b) * 0.5; // the guides' own time (rt_abi.h)
    RT_HIP(s->kernels->ambient(&a, &points, p->width * p->height, ap, mid, nullptr, out, g.obj_id, nullptr, stream));
    return RT_OK;
}

int ambient_frame_device(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtAmbientParams *ap, const RtGuides *g, double *out,
                         void *stream) {
    const int rc = check_ambient_frame(s, camera, p, ap, g, false, out);
    if (rc != RT_OK) return rc;
    RT_HIP(hipSetDevice(s->device));
    return enqueue_ambient_frame(s, camera, p, ap, *g, out, (hipStream_t)stream);
}

int ambient_frame_host(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtAmbientParams *ap, double *out) {
    int rc = check_ambient_frame(s, camera, p, ap, nullptr, true, out);
    if (rc != RT_OK) return rc;
    RT_HIP(hipSetDevice(s->device));
    const size_t pixels = (size_t)p->width * (size_t)p->height, n = 3 * pixels;
    rtapi::RenderBuffers &b = s->buf;
    if ((rc = rtapi::reserve_denoise(s, pixels, true)) != RT_OK) return rc;
    RT_HIP(b.frame.reserve(n));
    if ((rc = enqueue_ambient_frame(s, camera, p, ap, rtapi::scene_guides(s, pixels), b.frame.ptr, b.stream)) != RT_OK) return rc;
    RT_HIP(hipStreamSynchronize(b.stream));
    RT_HIP(hipMemcpy(out, b.frame.ptr, n * sizeof(double), hipMemcpyDeviceToHost)); // (a frame, not ray planes: those are rt_query_stage.h's)
    return RT_OK;
}

} // namespace

extern "C" {

void rt_ray_query_params_default(RtRayQueryParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->mode = RT_RAYS_CLOSEST;
}

int rt_trace_rays_device(RtScene *s, const RtRays *rays_device, int64_t n, const RtRayQueryParams *query, const RtRayHits *hits_device,
                         void *hip_stream) {
    return rtapi::guarded("rt_trace_rays_device", [&] { return trace_rays_device(s, rays_device, n, query, hits_device, hip_stream); });
}

int rt_trace_rays(RtScene *s, const RtRays *rays_host, int64_t n, const RtRayQueryParams *query, const RtRayHits *hits_host) {
    return rtapi::guarded("rt_trace_rays", [&] { return trace_rays_host(s, rays_host, n, query, hits_host); });
}

int rt_trace_occlusion_device(RtScene *s, const RtRays *rays_device, int64_t n, int32_t *occluded_device, void *hip_stream) {
    return rtapi::guarded("rt_trace_occlusion_device", [&] { return occlusion_device(s, rays_device, n, occluded_device, hip_stream); });
}

int rt_trace_occlusion(RtScene *s, const RtRays *rays_host, int64_t n, int32_t *occluded_host) {
    return rtapi::guarded("rt_trace_occlusion", [&] { return occlusion_host(s, rays_host, n, occluded_host); });
}

void rt_multihit_params_default(RtMultiHitParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->k = 4;
}

int rt_trace_rays_multi_device(RtScene *s, const RtRays *rays_device, int64_t n, const RtMultiHitParams *params, const RtRayHits *hits_device,
                               int32_t *count_device, void *hip_stream) {
    return rtapi::guarded("rt_trace_rays_multi_device",
                          [&] { return multi_device(s, rays_device, n, params, hits_device, count_device, hip_stream); });
}

int rt_trace_rays_multi(RtScene *s, const RtRays *rays_host, int64_t n, const RtMultiHitParams *params, const RtRayHits *hits_host,
                        int32_t *count_host) {
    return rtapi::guarded("rt_trace_rays_multi", [&] { return multi_host(s, rays_host, n, params, hits_host, count_host); });
}

void rt_ambient_params_default(RtAmbientParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->samples = 16;
    out->bias = 1e-3;
    out->radius = __builtin_inf();
}

int rt_trace_ambient_device(RtScene *s, const RtRays *points_device, int64_t n, const RtAmbientParams *params, int32_t *open_device,
                            const RtAmbientRays *walked_device, void *hip_stream) {
    return rtapi::guarded("rt_trace_ambient_device",
                          [&] { return ambient_device(s, points_device, n, params, open_device, walked_device, hip_stream); });
}

int rt_trace_ambient(RtScene *s, const RtRays *points_host, int64_t n, const RtAmbientParams *params, int32_t *open_host) {
    return rtapi::guarded("rt_trace_ambient", [&] { return ambient_host(s, points_host, n, params, open_host); });
}

int rt_render_ambient_device(RtScene *s, const RtCamera *camera, const RtRenderParams *params, const RtAmbientParams *ambient,
                             const RtGuides *guides_device, double *out_device, void *hip_stream) {
    return rtapi::guarded("rt_render_ambient_device",
                          [&] { return ambient_frame_device(s, camera, params, ambient, guides_device, out_device, hip_stream); });
}

int rt_render_ambient(RtScene *s, const RtCamera *camera, const RtRenderParams *params, const RtAmbientParams *ambient, double *out_host) {
    return rtapi::guarded("rt_render_ambient", [&] { return ambient_frame_host(s, camera, params, ambient, out_host); });
}

} // extern "C"
