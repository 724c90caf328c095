// rt_rays.hip — the host side of the ray query (include/rt_rays.h): the argument checks, the
// argument block, the device copy of the table's order, the launch (rt_rays_kernel.hip) and the chunked host form.
//
// Host code only (HIP runtime calls).  A query takes every scene rt_render_guides_device takes and follows its rules: the
// caller's stream, the tree when the scene walks one (use_bvh), and for a tree that renders keep in LDS its global copy,
// in whichever child order the last camera left it (a walk is correct in any order).
#include "rt_scene.h"

#include <cstring>

using rtapi::fail;

namespace {

// Everything that can be refused without a device, the scene last so that each refusal names its own cause.
int check_query(const RtScene *s, const RtRays *rays, int64_t n, const RtRayQueryParams *q, const RtRayHits *hits) {
    if (!rays || !hits || !q) return fail(RT_ERR_INVALID_ARGUMENT, "rays/hits/query is NULL");
    if (q->mode != RT_RAYS_CLOSEST && q->mode != RT_RAYS_ANY) return fail(RT_ERR_INVALID_ARGUMENT, "query->mode must be RT_RAYS_CLOSEST or RT_RAYS_ANY");
    if (q->_reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, "query->_reserved must be 0");
    if (n < 0 || n > (int64_t)INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "n must be in 0..INT32_MAX");
    // (an empty batch has no planes to look at: an empty tensor's address is NULL)
    if (n > 0 && (!rays->origin || !rays->direction)) return fail(RT_ERR_INVALID_ARGUMENT, "rays->origin/direction is NULL");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    return RT_OK;
}

} // namespace

// The scene part of the render's argument block: fill_trace_args with a zeroed camera and 2 x 2 one-sample params, as
// enqueue_guides fills it with the caller's (the camera and the pixel grid are read by nothing in k_trace_rays_f64, nor
// in rt_occlusion.hip's kernel, which takes the same block).
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

// The device copy of RtScene.table_order, made by the scene's first query (this one's or rt_multihit.hip's).  A plain
// (synchronous) copy, once: a later query on another stream must not overtake it.
int rtapi::ensure_order(RtScene *s) {
    if (s->rays_order.count == s->table_order.size()) return RT_OK;
    RT_HIP(s->rays_order.alloc(s->table_order.size()));
    RT_HIP(hipMemcpy(s->rays_order.ptr, s->table_order.data(), s->table_order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return RT_OK;
}

namespace {

using rtapi::ensure_order;
using rtapi::query_args;

int enqueue_rays(RtScene *s, const rtdev::TraceArgs &a, const RtRays &rays, int n, const RtRayQueryParams *q, const RtRayHits &hits,
                 hipStream_t stream) {
    RT_HIP(s->kernels->trace_rays(&a, &rays, &hits, s->rays_order.ptr, n, q->mode == RT_RAYS_ANY, stream));
    return RT_OK;
}

int trace_rays_device(RtScene *s, const RtRays *rays, int64_t n, const RtRayQueryParams *q, const RtRayHits *hits, void *stream) {
    int rc = check_query(s, rays, n, q, hits);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    if ((rc = query_args(s, a)) != RT_OK) return rc;
    if ((rc = ensure_order(s)) != RT_OK) return rc;
    return enqueue_rays(s, a, *rays, (int)n, q, *hits, (hipStream_t)stream);
}

int trace_rays_host(RtScene *s, const RtRays *rays, int64_t n, const RtRayQueryParams *q, const RtRayHits *hits) {
    int rc = check_query(s, rays, n, q, hits);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    if ((rc = query_args(s, a)) != RT_OK) return rc;
    if ((rc = ensure_order(s)) != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    const size_t chunk = (size_t)RT_RAYS_HOST_CHUNK;
    RT_HIP(b.rays_in.reserve(9 * chunk));
    RT_HIP(b.rays_out.reserve(9 * chunk));
    RT_HIP(b.rays_ids.reserve(3 * chunk));
    const hipStream_t stream = b.stream;
    // the chunk's planes on the device; a plane the caller leaves out is left out there too
    double *in = b.rays_in.ptr, *out = b.rays_out.ptr;
    int32_t *ids = b.rays_ids.ptr;
    RtRays dr;
    dr.origin = in;
    dr.direction = in + 3 * chunk;
    dr.t_min = rays->t_min ? in + 6 * chunk : nullptr;
    dr.t_max = rays->t_max ? in + 7 * chunk : nullptr;
    dr.time = rays->time ? in + 8 * chunk : nullptr;
    RtRayHits dh;
    dh.t = hits->t ? out : nullptr;
    dh.point = hits->point ? out + chunk : nullptr;
    dh.normal = hits->normal ? out + 4 * chunk : nullptr;
    dh.uv = hits->uv ? out + 7 * chunk : nullptr;
    dh.prim = hits->prim ? ids : nullptr;
    dh.obj_id = hits->obj_id ? ids + chunk : nullptr;
    dh.front_face = hits->front_face ? ids + 2 * chunk : nullptr;
    for (size_t at = 0; at < (size_t)n; at += chunk) {
        const size_t m = (size_t)n - at < chunk ? (size_t)n - at : chunk;
        auto up = [&](const double *dst, const double *src, size_t width) {
            return src ? hipMemcpyAsync((void *)dst, src + width * at, width * m * sizeof(double), hipMemcpyHostToDevice, stream) : hipSuccess;
        };
        RT_HIP(up(dr.origin, rays->origin, 3));
        RT_HIP(up(dr.direction, rays->direction, 3));
        RT_HIP(up(dr.t_min, rays->t_min, 1));
        RT_HIP(up(dr.t_max, rays->t_max, 1));
        RT_HIP(up(dr.time, rays->time, 1));
        if ((rc = enqueue_rays(s, a, dr, (int)m, q, dh, stream)) != RT_OK) return rc;
        auto down = [&](void *dst, const void *src, size_t width, size_t elem) {
            return dst ? hipMemcpyAsync((char *)dst + width * at * elem, src, width * m * elem, hipMemcpyDeviceToHost, stream) : hipSuccess;
        };
        RT_HIP(down(hits->t, dh.t, 1, sizeof(double)));
        RT_HIP(down(hits->point, dh.point, 3, sizeof(double)));
        RT_HIP(down(hits->normal, dh.normal, 3, sizeof(double)));
        RT_HIP(down(hits->uv, dh.uv, 2, sizeof(double)));
        RT_HIP(down(hits->prim, dh.prim, 1, sizeof(int32_t)));
        RT_HIP(down(hits->obj_id, dh.obj_id, 1, sizeof(int32_t)));
        RT_HIP(down(hits->front_face, dh.front_face, 1, sizeof(int32_t)));
        // (the next chunk's uploads reuse the buffers: stream order keeps them behind this chunk's launch and downloads)
    }
    RT_HIP(hipStreamSynchronize(stream));
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

} // extern "C"
