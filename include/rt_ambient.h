/* rt_ambient.h — ambient-occlusion queries: how much of the cosine-weighted hemisphere above a point is open.  Plain C;
 * RtRays and RT_RAY_INVALID are rt_rays.h's, "open" is rt_occlusion.h's answer 0.  DESIGN.md section 4.18 has the
 * definition, the lane mapping and the cost.
 *
 * INPUT.  An RtRays read as n POINTS: `origin` is the point, `direction` its surface normal (any non-zero length: it is
 * normalised here), `t_min` / `t_max` the point's bias and radius in world units (a NULL plane: the params' values for
 * every point), `time` as in rt_rays.h.
 *
 * SAMPLE s of point p (global index g = index_base + p), in this order of operations:
 *   1. n' = normal * 2^-E, E = rt_rays.h's exponent of THE DIRECTION'S SCALE (0 for a largest |component| within
 *      2^+-32: n' = normal), an exact product; nhat = unit(n').
 *   2. u = random_in_unit_sphere under rt_rng.h's contract with purpose RT_RNG_AMBIENT: candidates are blocks i = 0, 1, ...
 *      of counter {pixel = (uint32)g, sample = s, (0 << 8) | RT_RNG_AMBIENT, block = i} under key `seed`, three 42-bit
 *      coordinates c_j = -1 + 2 e_j per block as RT_RNG_SCATTER packs them; the first candidate with |c|^2 < 1 is u.
 *      (A candidate of exactly (0, 0, 0), one in 2^126, would leave a NaN direction: such a sample is never open.)
 *   3. dir = nhat + unit(u), component by component: the render's Lambertian direction (lambertian.rs:27).
 *   4. If every |component| of dir is below 1e-8 (near_zero), dir = nhat.
 *   5. dhat = unit(dir).
 *   6. The ray is (point, dhat, [bias_p, radius_p], time_p); the sample is OPEN iff rt_trace_occlusion answers 0 for it.
 * unit(a) is the flavour's own.  RT_ARITH_REFERENCE: l2 = (a.x * a.x + a.y * a.y) + a.z * a.z, l = sqrt(l2), then
 * (a.x / l, a.y / l, a.z / l) — five roundings before the square root's, no contraction anywhere.  RT_ARITH_FAST:
 * r = 1 / sqrt(l2) from the hardware seed and one third-order step (at most 1 ulp), then (a.x * r, a.y * r, a.z * r), and
 * a product may be contracted into the sum that takes it (l2's, step 3's); dhat's own three products are rounded.
 * |c|^2 is the same sum as l2.
 *
 * ANSWER.  int32_t open[n]: the number of open samples of a valid point, 0 .. samples; RT_RAY_INVALID for an invalid
 * point — a non-finite point, normal or time, a normal of all zeros, a bias that is negative or non-finite, a radius
 * that is NaN or below the bias — which is answered in its lane and never an error of the call.  The cosine-weighted
 * ambient-occlusion value of a point is open / samples.  Because g addresses the draws, a batch may be cut anywhere:
 * the second part passes index_base + (points before it).
 *
 * EXPORT (device form only).  The rays the kernel walked, ray j = p * samples + s, into the planes of an RtAmbientRays
 * that are not NULL: exactly the values the walk saw, so rt_trace_occlusion_device on them answers what was counted.
 * An invalid point's rays carry the point's own origin, window and time and a direction of zeros: invalid rays.
 *
 * Refused with RT_ERR_INVALID_ARGUMENT before a device is touched, each with its own message: a NULL scene, points,
 * params or output; samples not a power of two in 1..1024; a non-zero _reserved; a bias that is negative or non-finite;
 * a radius that is NaN or below the bias; index_base < 0 or index_base + n > 2^32; a NULL origin or direction when
 * n > 0; n < 0 or n > INT32_MAX.  The frame forms also refuse what rt_render_guides_device refuses, guides with a NULL
 * plane and a non-zero index_base.  n == 0 is RT_OK and enqueues nothing.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
#ifndef RT_AMBIENT_H
#define RT_AMBIENT_H

#include "rt_occlusion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_RNG_AMBIENT 9          /* rt_rng.h's purposes end at 8: block i = candidate i of sample s of point g */
#define RT_AMBIENT_MAX_SAMPLES 1024

typedef struct RtAmbientParams {
    int32_t samples;      /* S: a power of two in 1..RT_AMBIENT_MAX_SAMPLES */
    int32_t _reserved;    /* must be 0 */
    double  bias;         /* near end of every sample's window where the points bring no t_min plane; default 1e-3 */
    double  radius;       /* far end where they bring no t_max plane; default +inf */
    uint64_t seed;
    int64_t  index_base;  /* the RNG index of point 0; 0 <= index_base, index_base + n <= 2^32 */
} RtAmbientParams;

typedef struct RtAmbientRays {    /* n * samples rays as planes; any plane may be NULL */
    double *origin;       /* 3 per ray */
    double *direction;    /* 3 per ray: dhat */
    double *t_min;
    double *t_max;
    double *time;
} RtAmbientRays;

/* samples 16, bias 1e-3, radius +inf, seed 0, index_base 0. */
void rt_ambient_params_default(RtAmbientParams *out);

/* n points whose planes, the n answers and the export's planes are device memory of the scene's device, enqueued on
 * `hip_stream` (NULL = default stream) without synchronising, and without an upload on a scene's first call.  The structs
 * themselves are host memory, read before the call returns.  rays_out_device may be NULL: nothing is exported. */
int rt_trace_ambient_device(RtScene *scene, const RtRays *points_device, int64_t n, const RtAmbientParams *params,
                            int32_t *open_device, const RtAmbientRays *rays_out_device, void *hip_stream);

/* Host-memory convenience, synchronous: staged in chunks of RT_RAYS_HOST_CHUNK points like rt_trace_occlusion; the answer
 * does not depend on the chunking. */
int rt_trace_ambient(RtScene *scene, const RtRays *points_host, int64_t n, const RtAmbientParams *params,
                     int32_t *open_host);

/* The ambient-occlusion FRAME of (camera, params): rt_render_guides_device's guides into the caller's complete
 * guides_device, then the query at every pixel p = y * W + x — point = the guide position, normal = the guide normal,
 * time = (time_a + time_b) / 2, ambient->index_base == 0 — and sqrt(open / samples) into all three channels of
 * out_device (W*H*3 f64): gamma-encoded like rt_render_frame_device's frame, so rt_post_rgba8_device and
 * rt_denoise_device take it as it is.  A pixel whose guide ray misses (obj_id == -1) gets 1.  Enqueued on `hip_stream`
 * without synchronising. */
int rt_render_ambient_device(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                             const RtAmbientParams *ambient, const RtGuides *guides_device, double *out_device,
                             void *hip_stream);

/* Host-output convenience, synchronous: the guides are the scene's own, out_host is W*H*3 f64. */
int rt_render_ambient(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                      const RtAmbientParams *ambient, double *out_host);

#ifdef __cplusplus
}
#endif

#endif /* RT_AMBIENT_H */
