// rt_occlusion.hip — the host side of the occlusion query (include/rt_occlusion.h): the argument
// checks, the argument block, the launch (rt_occlusion_kernel.hip) and the chunked host form.
//
// Host code only (HIP runtime calls).  A query takes every scene rt_trace_rays_device takes, under its rules
// (rt_rays.hip: query_args): the caller's stream, the tree when the scene walks one (use_bvh), and for a tree that renders
// keep in LDS its global copy, in whichever child order the last camera left it (a yes or no is the same in any order).
// There is no `order` table here, so a scene's first call uploads nothing.
#include "rt_scene.h"

using rtapi::fail;

namespace {

// Everything that can be refused without a device, the scene last so that each refusal names its own cause.
int check_occlusion(const RtScene *s, const RtRays *rays, int64_t n, const int32_t *occluded) {
    if (!rays) return fail(RT_ERR_INVALID_ARGUMENT, "rays is NULL");
    if (!occluded) return fail(RT_ERR_INVALID_ARGUMENT, "occluded is NULL");
    if (n < 0 || n > (int64_t)INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "n must be in 0..INT32_MAX");
    // (an empty batch has no planes to look at: an empty tensor's address is NULL)
    if (n > 0 && !rays->origin) return fail(RT_ERR_INVALID_ARGUMENT, "rays->origin is NULL");
    if (n > 0 && !rays->direction) return fail(RT_ERR_INVALID_ARGUMENT, "rays->direction is NULL");
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    return RT_OK;
}

int occlusion_device(RtScene *s, const RtRays *rays, int64_t n, int32_t *occluded, void *stream) {
    int rc = check_occlusion(s, rays, n, occluded);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    if ((rc = rtapi::query_args(s, a)) != RT_OK) return rc;
    RT_HIP(s->kernels->occlusion(&a, rays, occluded, (int)n, (hipStream_t)stream));
    return RT_OK;
}

int occlusion_host(RtScene *s, const RtRays *rays, int64_t n, int32_t *occluded) {
    int rc = check_occlusion(s, rays, n, occluded);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    if ((rc = rtapi::query_args(s, a)) != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    const size_t chunk = (size_t)RT_RAYS_HOST_CHUNK;
    // (rt_trace_rays' sizes: whichever of the two runs first on a scene allocates for both)
    RT_HIP(b.rays_in.reserve(9 * chunk));
    RT_HIP(b.rays_ids.reserve(3 * chunk));
    const hipStream_t stream = b.stream;
    // the chunk's planes on the device; a plane the caller leaves out is left out there too
    double *in = b.rays_in.ptr;
    int32_t *answers = b.rays_ids.ptr;
    RtRays dr;
    dr.origin = in;
    dr.direction = in + 3 * chunk;
    dr.t_min = rays->t_min ? in + 6 * chunk : nullptr;
    dr.t_max = rays->t_max ? in + 7 * chunk : nullptr;
    dr.time = rays->time ? in + 8 * chunk : nullptr;
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
        RT_HIP(s->kernels->occlusion(&a, &dr, answers, (int)m, stream));
        RT_HIP(hipMemcpyAsync(occluded + at, answers, m * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        // (the next chunk's uploads reuse the buffers: stream order keeps them behind this chunk's launch and download)
    }
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_trace_occlusion_device(RtScene *s, const RtRays *rays_device, int64_t n, int32_t *occluded_device, void *hip_stream) {
    return rtapi::guarded("rt_trace_occlusion_device", [&] { return occlusion_device(s, rays_device, n, occluded_device, hip_stream); });
}

int rt_trace_occlusion(RtScene *s, const RtRays *rays_host, int64_t n, int32_t *occluded_host) {
    return rtapi::guarded("rt_trace_occlusion", [&] { return occlusion_host(s, rays_host, n, occluded_host); });
}

} // extern "C"
