// rt_multihit.hip — the host side of the multi-hit query (include/rt_multihit.h): the argument
// checks, the argument block, the launch (rt_multihit_kernel.hip) and the chunked host form.
//
// Host code only (HIP runtime calls).  A query takes every scene rt_trace_rays_device takes, under its rules (rt_rays.hip:
// query_args, ensure_order): the caller's stream, the tree when the scene walks one (use_bvh), for a tree that renders keep
// in LDS its global copy, in whichever child order the last camera left it (rt_bvh_kbest.h: any order is correct), and the
// device copy of the table's order that the scene's first query of either kind uploads.
#include "rt_scene.h"

#include <cstring>

using rtapi::fail;

namespace {

// Everything that can be refused without a device, the scene last so that each refusal names its own cause.
int check_multi(const RtScene *s, const RtRays *rays, int64_t n, const RtMultiHitParams *p, const RtRayHits *hits) {
    if (!rays) return fail(RT_ERR_INVALID_ARGUMENT, "rays is NULL");
    if (!p) return fail(RT_ERR_INVALID_ARGUMENT, "params is NULL");
    if (!hits) return fail(RT_ERR_INVALID_ARGUMENT, "hits is NULL");
    if (p->k < 1 || p->k > RT_MULTIHIT_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "params->k must be in 1..RT_MULTIHIT_MAX");
    if (p->_reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, "params->_reserved must be 0");
    if (n < 0 || n > (int64_t)INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "n must be in 0..INT32_MAX");
    // (an empty batch has no planes to look at: an empty tensor's address is NULL)
    if (n > 0 && !rays->origin) return fail(RT_ERR_INVALID_ARGUMENT, "rays->origin is NULL");
    if (n > 0 && !rays->direction) return fail(RT_ERR_INVALID_ARGUMENT, "rays->direction is NULL");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    return RT_OK;
}

int multi_device(RtScene *s, const RtRays *rays, int64_t n, const RtMultiHitParams *p, const RtRayHits *hits, int32_t *count, void *stream) {
    int rc = check_multi(s, rays, n, p, hits);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    if ((rc = rtapi::query_args(s, a)) != RT_OK) return rc;
    if ((rc = rtapi::ensure_order(s)) != RT_OK) return rc;
    RT_HIP(s->kernels->multihit(&a, rays, hits, count, s->rays_order.ptr, (int)n, p->k, (hipStream_t)stream));
    return RT_OK;
}

int multi_host(RtScene *s, const RtRays *rays, int64_t n, const RtMultiHitParams *p, const RtRayHits *hits, int32_t *count) {
    int rc = check_multi(s, rays, n, p, hits);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    if ((rc = rtapi::query_args(s, a)) != RT_OK) return rc;
    if ((rc = rtapi::ensure_order(s)) != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    // rt_trace_rays' sizes and not a byte more (whichever runs first on a scene allocates for both).  A chunk here is an
    // eighth of that call's: `rays` rays with up to RT_MULTIHIT_MAX slots each fill at most `plane` = rays x 8 entries of an
    // answer plane, the room one plane of rt_trace_rays has.  The rays' own planes then take an eighth of rays_in; the
    // counts go behind them.
    const size_t plane = (size_t)RT_RAYS_HOST_CHUNK, chunk = plane / RT_MULTIHIT_MAX;
    static_assert(RT_RAYS_HOST_CHUNK % RT_MULTIHIT_MAX == 0, "a chunk of rt_trace_rays holds a whole number of multi-hit rays");
    RT_HIP(b.rays_in.reserve(9 * plane));
    RT_HIP(b.rays_out.reserve(9 * plane));
    RT_HIP(b.rays_ids.reserve(3 * plane));
    const hipStream_t stream = b.stream;
    const size_t k = (size_t)p->k;
    double *in = b.rays_in.ptr, *out = b.rays_out.ptr;
    int32_t *ids = b.rays_ids.ptr;
    int32_t *counts = reinterpret_cast<int32_t *>(in + 9 * chunk); // (9 * chunk doubles in: 8-byte aligned, 1/8 of the buffer used)
    RtRays dr;
    dr.origin = in;
    dr.direction = in + 3 * chunk;
    dr.t_min = rays->t_min ? in + 6 * chunk : nullptr;
    dr.t_max = rays->t_max ? in + 7 * chunk : nullptr;
    dr.time = rays->time ? in + 8 * chunk : nullptr;
    // the chunk's planes on the device, slot-major over the chunk's own m rays; a plane the caller leaves out is left out
    RtRayHits dh;
    dh.t = hits->t ? out : nullptr;
    dh.point = hits->point ? out + plane : nullptr;
    dh.normal = hits->normal ? out + 4 * plane : nullptr;
    dh.uv = hits->uv ? out + 7 * plane : nullptr;
    dh.prim = hits->prim ? ids : nullptr;
    dh.obj_id = hits->obj_id ? ids + plane : nullptr;
    dh.front_face = hits->front_face ? ids + 2 * plane : nullptr;
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
        RT_HIP(s->kernels->multihit(&a, &dr, &dh, count ? counts : nullptr, s->rays_order.ptr, (int)m, p->k, stream));
        // slot j of the chunk, m entries from j * m on the device, goes to entries j * n + at of the caller's plane
        auto down = [&](void *dst, const void *src, size_t width, size_t elem) {
            if (!dst) return hipSuccess;
            for (size_t j = 0; j < k; ++j) {
                const hipError_t e = hipMemcpyAsync((char *)dst + width * (j * (size_t)n + at) * elem, (const char *)src + width * j * m * elem,
                                                    width * m * elem, hipMemcpyDeviceToHost, stream);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        };
        RT_HIP(down(hits->t, dh.t, 1, sizeof(double)));
        RT_HIP(down(hits->point, dh.point, 3, sizeof(double)));
        RT_HIP(down(hits->normal, dh.normal, 3, sizeof(double)));
        RT_HIP(down(hits->uv, dh.uv, 2, sizeof(double)));
        RT_HIP(down(hits->prim, dh.prim, 1, sizeof(int32_t)));
        RT_HIP(down(hits->obj_id, dh.obj_id, 1, sizeof(int32_t)));
        RT_HIP(down(hits->front_face, dh.front_face, 1, sizeof(int32_t)));
        if (count) RT_HIP(hipMemcpyAsync(count + at, counts, m * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        // (the next chunk's uploads reuse the buffers: stream order keeps them behind this chunk's launch and downloads)
    }
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

} // namespace

extern "C" {

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

} // extern "C"
