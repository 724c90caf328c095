// rt_query_stage.h — the chunked host form of every query on caller rays (rt_query.hip: rt_trace_rays, rt_trace_occlusion,
// rt_trace_rays_multi; rt_trace_ambient's points are staged as rays are), ONCE: the caller's host planes go through the scene's three staging buffers a chunk at a time, a
// launch per chunk, the answers back behind it.  Runtime calls only (reserve, hipMemcpyAsync, hipStreamSynchronize), no
// kernel and no launcher of its own: it compiles with a plain host compiler against a fake runtime
// (tests/query_stage_driver.cpp).  Private to the library.
#pragma once
#include "rt_scene.h"

namespace rtapi {

// n > 0 rays of `rays` (host planes) through launch(device RtRays, device RtRayHits, device int32 plane, m) for every chunk
// of m rays, the answers into `hits` (NULL: the query has no hit planes) and `per_ray` (NULL: no int32 per ray), then ONE
// synchronisation of b.stream.  A plane the caller leaves out is neither staged nor passed: it arrives as NULL.
//   plane: entries of one staging plane (the entry points pass RT_RAYS_HOST_CHUNK).  The buffers are what rt_trace_rays
//     made them, whichever query runs first on a scene: rays_in [origin 3 | direction 3 | t_min | t_max | time] x plane
//     doubles, rays_out [t | point 3 | normal 3 | uv 2] x plane doubles (only where there are hit planes), rays_ids
//     [prim | obj_id | front_face] x plane.
//   k, slots: a ray answers with k <= slots entries per hit plane, so a chunk is plane / slots rays.  On the device a hit
//     plane is slot-major over the chunk's own m rays (slot j from entry j * m on); it goes to entries j * n + at of the
//     caller's plane, which for k = 1 is the plain plane.
//   The int32 plane takes the first plane of rays_ids where no hit plane does; else it goes behind the rays' own planes in
//     rays_in, where slots >= 2 leave seven eighths and more unused (and a query with slots = 1 would grow the buffer).
template <class Launch>
int stage_query(RenderBuffers &b, size_t plane, const RtRays *rays, size_t n, const RtRayHits *hits, size_t k, size_t slots,
                int32_t *per_ray, Launch launch) {
    const size_t chunk = plane / slots;
    const size_t with_ints = 9 * chunk + (hits && per_ray ? (chunk + 1) / 2 : 0);
    RT_HIP(b.rays_in.reserve(with_ints > 9 * plane ? with_ints : 9 * plane));
    if (hits) RT_HIP(b.rays_out.reserve(9 * plane));
    RT_HIP(b.rays_ids.reserve(3 * plane));
    const hipStream_t stream = b.stream;
    double *in = b.rays_in.ptr, *out = b.rays_out.ptr;
    int32_t *ids = b.rays_ids.ptr;
    RtRays dr;
    dr.origin = in;
    dr.direction = in + 3 * chunk;
    dr.t_min = rays->t_min ? in + 6 * chunk : nullptr;
    dr.t_max = rays->t_max ? in + 7 * chunk : nullptr;
    dr.time = rays->time ? in + 8 * chunk : nullptr;
    const RtRayHits none = {};
    const RtRayHits &h = hits ? *hits : none;
    RtRayHits dh;
    dh.t = h.t ? out : nullptr;
    dh.point = h.point ? out + plane : nullptr;
    dh.normal = h.normal ? out + 4 * plane : nullptr;
    dh.uv = h.uv ? out + 7 * plane : nullptr;
    dh.prim = h.prim ? ids : nullptr;
    dh.obj_id = h.obj_id ? ids + plane : nullptr;
    dh.front_face = h.front_face ? ids + 2 * plane : nullptr;
    int32_t *const ints = !per_ray ? nullptr : hits ? reinterpret_cast<int32_t *>(in + 9 * chunk) : ids;
    for (size_t at = 0; at < n; at += chunk) {
        const size_t m = n - at < chunk ? n - at : chunk;
        auto up = [&](const double *dst, const double *src, size_t width) {
            return src ? hipMemcpyAsync((void *)dst, src + width * at, width * m * sizeof(double), hipMemcpyHostToDevice, stream) : hipSuccess;
        };
        RT_HIP(up(dr.origin, rays->origin, 3));
        RT_HIP(up(dr.direction, rays->direction, 3));
        RT_HIP(up(dr.t_min, rays->t_min, 1));
        RT_HIP(up(dr.t_max, rays->t_max, 1));
        RT_HIP(up(dr.time, rays->time, 1));
        RT_HIP(launch(dr, dh, ints, (int)m));
        auto down = [&](void *dst, const void *src, size_t width, size_t elem, size_t rows) {
            for (size_t j = 0; dst && j < rows; ++j) {
                const hipError_t e = hipMemcpyAsync((char *)dst + width * (j * n + at) * elem, (const char *)src + width * j * m * elem,
                                                    width * m * elem, hipMemcpyDeviceToHost, stream);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        };
        RT_HIP(down(h.t, dh.t, 1, sizeof(double), k));
        RT_HIP(down(h.point, dh.point, 3, sizeof(double), k));
        RT_HIP(down(h.normal, dh.normal, 3, sizeof(double), k));
        RT_HIP(down(h.uv, dh.uv, 2, sizeof(double), k));
        RT_HIP(down(h.prim, dh.prim, 1, sizeof(int32_t), k));
        RT_HIP(down(h.obj_id, dh.obj_id, 1, sizeof(int32_t), k));
        RT_HIP(down(h.front_face, dh.front_face, 1, sizeof(int32_t), k));
        RT_HIP(down(per_ray, ints, 1, sizeof(int32_t), 1));
        // (the next chunk's uploads reuse the buffers: stream order keeps them behind this chunk's launch and downloads)
    }
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

} // namespace rtapi
