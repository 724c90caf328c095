/* rt_multihit.h — multi-hit ray queries: the first k primitives along each ray of a batch the caller brings.  Plain C;
 * RtRays, RtRayHits, their defaults, RT_RAY_MISS and RT_RAY_INVALID are rt_rays.h's.  DESIGN.md section 4.17 has the
 * definition and the walk, tests/multihit_model.py restates it with the oracle.
 *
 * THE RULE.  Take a ray with window [t_min, t_max] and a time.  Every primitive of the scene has at most one hit: the hit
 * the render's own test for that primitive alone reports over the window (for a sphere, the nearer root inside the window,
 * else the farther).  The answer is those hits sorted by ascending t, the first k of them.  Slot 0 is therefore what
 * RT_RAYS_CLOSEST reports, slot j what RT_RAYS_CLOSEST would report with the primitives of slots 0..j-1 removed from the
 * scene, and one primitive never fills two slots.  Among hits with exactly equal t the order is unspecified; if such a
 * tie straddles slot k-1 and the first hit left out, which of the two is kept is unspecified.  Both window ends are
 * inclusive, and the fast flavour's open box edges are rt_rays.h's.  So is the direction's scale (rt_rays.h: THE
 * DIRECTION'S SCALE): the direction is normalised by a power of two before the walk and every slot's t handed back in the
 * caller's units; tested for a largest component within 2^+-300.
 *
 * count is the number of filled slots, 0..k.  There is no "more than k" flag: computing one would forbid the shrinking far
 * end that makes the walk cheap (once k hits are held, nothing beyond the k-th is looked at).  Unfilled slots hold a miss's
 * values: t = +inf, prim = obj_id = RT_RAY_MISS, zeros elsewhere.  An INVALID ray (rt_rays.h's rule) has
 * count = RT_RAY_INVALID, prim = RT_RAY_INVALID in every slot and a miss's values elsewhere; it is never an error of the
 * call.
 *
 * LAYOUT.  The planes of RtRayHits are slot-major: element (slot j, ray r) of a plane with c components starts at
 * c * (j * n + r), so a plane holds k * n entries, and slot 0's part of every plane is laid out exactly as rt_trace_rays
 * lays out its answer.  Every plane, and count, may be NULL: a NULL plane is not written.  uv is computed only when asked
 * for.
 *
 * Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: a NULL scene, rays, params or hits, a NULL origin or
 * direction when n > 0, n < 0, n > INT32_MAX, k < 1 or k > RT_MULTIHIT_MAX, a non-zero _reserved.  n == 0 is RT_OK and
 * enqueues nothing.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
#ifndef RT_MULTIHIT_H
#define RT_MULTIHIT_H

#include "rt_rays.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_MULTIHIT_MAX 8

typedef struct RtMultiHitParams { int32_t k; int32_t _reserved; } RtMultiHitParams;

void rt_multihit_params_default(RtMultiHitParams *out);              /* k = 4 */

/* n rays whose planes, the k * n entries of every answer plane and the n counts are device memory of the scene's device,
 * enqueued on `hip_stream` (NULL = default stream) without synchronising (a scene's FIRST query of rt_rays.h or of this
 * header uploads the table's order with one synchronous copy of 4 B per primitive).  The structs themselves are host
 * memory, read before the call returns. */
int rt_trace_rays_multi_device(RtScene *scene, const RtRays *rays_device, int64_t n, const RtMultiHitParams *params,
                               const RtRayHits *hits_device, int32_t *count_device, void *hip_stream);

/* Host-memory convenience, synchronous: the rays are staged through the device buffers rt_trace_rays stages through, in
 * chunks of RT_RAYS_HOST_CHUNK / RT_MULTIHIT_MAX rays (a call of any n and k allocates what rt_trace_rays allocates), and
 * each chunk's slots are copied into the caller's slot-major planes of k * n entries. */
int rt_trace_rays_multi(RtScene *scene, const RtRays *rays_host, int64_t n, const RtMultiHitParams *params,
                        const RtRayHits *hits_host, int32_t *count_host);

#ifdef __cplusplus
}
#endif

#endif /* RT_MULTIHIT_H */
