/* rt_occlusion.h — occlusion queries: one yes or no per ray of a batch the caller brings.  Plain C; RtRays, its defaults
 * and RT_RAY_INVALID are rt_rays.h's.  DESIGN.md section 4.16 has the definition and the walk.
 *
 * A ray is occluded iff RT_RAYS_CLOSEST (rt_rays.h) over the same window would report a hit.  Both window ends are
 * inclusive, the defaults are [0.001, inf), and t is in units of the direction.  A segment from a to b is the ray
 * (a, b - a) with a window inside [0, 1] — however close a and b lie: the direction's scale is rt_rays.h's (THE
 * DIRECTION'S SCALE: normalised by a power of two before the walk, tested for a largest component within 2^+-300).
 *
 * The answer is one int32_t per ray: 1 occluded, 0 not, RT_RAY_INVALID for an invalid ray (rt_rays.h's rule: a non-finite
 * origin, direction, time or t_min, t_min < 0, a t_max that is NaN or below t_min, a direction of all zeros), which is
 * answered in its lane and never an error of the call.  On a scene with a tree the walk leaves at the first accepted
 * primitive instead of looking for the nearest one.
 *
 * Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: a NULL scene, rays or output, n < 0, n > INT32_MAX, a
 * NULL origin or direction when n > 0.  n == 0 is RT_OK and enqueues nothing.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
#ifndef RT_OCCLUSION_H
#define RT_OCCLUSION_H

#include "rt_rays.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n rays whose planes, and the n answers, are device memory of the scene's device, enqueued on `hip_stream` (NULL =
 * default stream) without synchronising, and without an upload on a scene's first call.  The RtRays struct itself is host
 * memory, read before the call returns. */
int rt_trace_occlusion_device(RtScene *scene, const RtRays *rays_device, int64_t n, int32_t *occluded_device,
                              void *hip_stream);

/* Host-memory convenience, synchronous: the rays are staged through the scene's own device buffers in chunks of
 * RT_RAYS_HOST_CHUNK (a call of any n allocates the same), the answers copied back chunk by chunk. */
int rt_trace_occlusion(RtScene *scene, const RtRays *rays_host, int64_t n, int32_t *occluded_host);

#ifdef __cplusplus
}
#endif

#endif /* RT_OCCLUSION_H */
