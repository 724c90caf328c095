/* rt_rays.h — ray queries: the scene's closest hit, or any hit, for a batch of rays the caller brings.  Plain C; the
 * types are rt_abi.h's.  DESIGN.md section 4.15 has the definition, tests/ray_query_model.py restates it with the oracle.
 *
 * A ray is (origin, direction, [t_min, t_max], time).  The direction has any length: t is in units of it (ray.rs:30-32).
 * THE DIRECTION'S SCALE.  A direction whose largest component lies outside 2^-32 .. 2^33 in magnitude is walked as
 * d 2^-E over the window [t_min, t_max] 2^E, E the binary exponent of that component, and t is handed back times 2^-E
 * (csrc/rt_query_ray.h): exact products, so the answer does not depend on the unit the direction is measured in — bit
 * for bit in the RT_ARITH_REFERENCE flavour, and one answer for every scale outside that band in the fast one.  Held by
 * the tests for a largest component within 2^-300 .. 2^300.  The same code serves every largest component that is a
 * normal double, untested beyond that range; what then limits a ray is the range of a double alone: a window end whose
 * scaled value overflows or underflows acts as +inf or 0, and a t that leaves the range in the caller's units is reported
 * as it rounds there.  The record is formed from the caller's own o and d and the reported t (point = o + t d).
 * Directions of subnormal components are scaled by 2^1022 and no further.
 * RT_RAYS_CLOSEST answers with the scene's own closest-hit rule over the ray's window — the rule a render applies over
 * [0.001, inf): both ends inclusive, in the linear loop a later primitive wins an exact tie, through the tree only exact
 * ties may differ, and a box's side on an edge is open.  The record is the render's hit record: point, the face normal
 * (against the ray), u / v in f64, front_face, with every wrapper quirk the render has (translate.rs:36).
 * RT_RAYS_ANY answers with SOME primitive that has a hit inside the window (which one is unspecified), and the record of
 * that hit.
 *
 * A ray that lies EXACTLY in the plane of a rect or of a box's side meets the reference's own 0 / 0 there: as in the
 * reference that primitive then answers with t = NaN, and which primitive the query names is unspecified.
 *
 * The planes of RtRays must not be written to while a query that reads them is in flight: a kernel may read a ray's
 * entries more than once.
 *
 * A miss is t = +inf, prim = obj_id = RT_RAY_MISS and zeros elsewhere.  An INVALID ray — a non-finite origin, direction,
 * time or t_min, t_min < 0, a t_max that is NaN or below t_min, a direction of all zeros — is answered in its lane with
 * prim = RT_RAY_INVALID and a miss's values elsewhere; it is never an error of the call.
 *
 * Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: a NULL scene, rays, hits, query, origin or direction,
 * n < 0, n > INT32_MAX, an unknown mode, a non-zero _reserved.  n == 0 is RT_OK and enqueues nothing (the planes of an
 * empty batch are not looked at).
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
#ifndef RT_RAYS_H
#define RT_RAYS_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rays per staging chunk of rt_trace_rays: 172 B of device memory per ray of it, whatever n is */
#define RT_RAYS_HOST_CHUNK 262144

enum { RT_RAY_MISS = -1, RT_RAY_INVALID = -2 };
enum RtRayQueryMode { RT_RAYS_CLOSEST = 0, RT_RAYS_ANY = 1 };

typedef struct RtRays {          /* n rays as planes */
    const double *origin;        /* 3n, required */
    const double *direction;     /* 3n, required; any length: t is in units of it (ray.rs:30-32) */
    const double *t_min;         /* n, or NULL: 0.001 for every ray (renderer.rs:58) */
    const double *t_max;         /* n, or NULL: +inf */
    const double *time;          /* n, or NULL: 0 (only MovingSphere reads it) */
} RtRays;

typedef struct RtRayHits {       /* every plane may be NULL: then it is not written */
    double  *t;                  /* n   */
    double  *point;              /* 3n  */
    double  *normal;             /* 3n  the face normal, against the ray */
    double  *uv;                 /* 2n  */
    int32_t *prim;               /* n   index into RtSceneDesc.primitives, or RT_RAY_MISS / RT_RAY_INVALID */
    int32_t *obj_id;             /* n   that primitive's RtPrimitive.obj_id */
    int32_t *front_face;         /* n   */
} RtRayHits;

typedef struct RtRayQueryParams { int32_t mode; int32_t _reserved; } RtRayQueryParams;

void rt_ray_query_params_default(RtRayQueryParams *out);     /* RT_RAYS_CLOSEST */

/* n rays whose planes (and the planes of the answer) are device memory of the scene's device, enqueued on `hip_stream`
 * (NULL = default stream) without synchronising (a scene's FIRST query of either form uploads the table's order with one
 * synchronous copy of 4 B per primitive).  The structs themselves are host memory, read before the call returns. */
int rt_trace_rays_device(RtScene *scene, const RtRays *rays_device, int64_t n, const RtRayQueryParams *query,
                         const RtRayHits *hits_device, void *hip_stream);

/* Host-memory convenience, synchronous: the rays are staged through the scene's own device buffers in chunks of a bounded
 * size (a call of any n allocates the same), the answers copied back chunk by chunk. */
int rt_trace_rays(RtScene *scene, const RtRays *rays_host, int64_t n, const RtRayQueryParams *query,
                  const RtRayHits *hits_host);

#ifdef __cplusplus
}
#endif

#endif /* RT_RAYS_H */
