// rt_scene.h — what the host-side translation units of the library share: the RtScene object
// behind include/rt_abi.h's opaque handle, the RT_HIP check of a runtime call and the one function
// that enqueues a render (rt_api.hip), with the render buffers a scene carries (RenderBuffers).  The
// error helpers are rt_error.h's, the rules that need no device rt_plan.h's, the types that own device
// memory, pinned memory, streams and events rt_resources.h's: nothing here frees by hand.  Holds no
// kernel and compiles with a plain host compiler (tests/resources_driver.cpp).  Private to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>
#include <string>
#include <vector>
#include "rt_device_types.h"
#include "rt_bvh.h"
#include "rt_error.h"
#include "rt_plan.h"
#include "rt_resources.h"
#include "../../include/rt_abi.h"
#include "../../include/rt_rays.h"
#include "../../include/rt_occlusion.h"
#include "../../include/rt_multihit.h"
#include "../../include/rt_ambient.h"

// The trace kernels exist twice (rt_trace_common.h: ARITHMETIC): RT_ARITH_FAST, and RT_ARITH_REFERENCE behind *_exact.
// Every launcher that has both flavours, ONCE: X(member of rtapi::Launchers, exported name, return type, parameters).  The
// declarations of both flavours, the struct and its two tables (rt_scene_create.hip) are all expanded from this list.
//   trace (rt_trace_kernel.hip): the v1 kernel.
//   pool_*, trace_pool (rt_trace_pool_kernel.hip): the pooled kernel, the variant's resident blocks per CU and static LDS.
//   resolve, resolve_chunks, fold_* (rt_frame_kernels.hip): the resolve pass over per-pixel sums, the resolve and fold
//     passes over the pooled kernel's slices (fold_adaptive with the tiles' decisions, rt_tile_decide.h).
//   nee (rt_nee_kernel.hip): the whole frame's NEE samples into args->accum.
//   nee_pass, nee_chunk, nee_decide (rt_nee_pass_kernel.hip): one chunk of the NEE estimator over listed tiles on top of
//     args->accum, the batch-means update behind it and the decision step behind a pass (rt_tile_decide.h).
//   nee_stream* (rt_nee_stream_kernel.hip): the NEE estimator as ONE persistent launch of `blocks` blocks over args'
//     region-ordered tile queue, every tile delivered into args->deliver_out; the variant's resident blocks per CU (the
//     runtime's occupancy query); the chunk length the flavour was compiled with.
//   nee_lights* (rt_nee_lights_kernel.hip, rt_nee_lights_pass_kernel.hip, rt_nee_lights_stream_kernel.hip): nee, nee_pass,
//     nee_stream and its blocks per CU with the extended light code (rt_nee_lights.h), which exist for PRIMS_ANY only.
//   trace_rays (rt_rays_kernel.hip): n caller rays of device planes against args' scene, closest or any hit; `order` is
//     the device copy of the table's description indices.
//   occlusion (rt_occlusion_kernel.hip): n caller rays of device planes against args' scene, one int32 per ray: is there
//     a hit inside the ray's window (include/rt_occlusion.h).
//   multihit (rt_multihit_kernel.hip): n caller rays of device planes against args' scene, the first k primitives
//     along each ray into slot-major planes and a count per ray (include/rt_multihit.h); `order` as for trace_rays.
//   ambient (rt_ambient_kernel.hip): n caller points of device planes against args' scene, params' hemisphere samples of
//     each formed, walked and counted (include/rt_ambient.h): the count into `open`, or its frame value into `frame` beside
//     the guides' obj_id; the rays it walked into `walked`'s planes where there are some.
#define RT_LAUNCHER_LIST(X)                                                                                                \
    X(trace, rtdev_launch_trace, hipError_t,                                                                               \
      (const rtdev::TraceArgs *args, int prims_class, int textured, int specular, hipStream_t stream))                     \
    X(resolve, rtdev_launch_resolve, hipError_t,                                                                           \
      (const double *accum, double *out, int width, int height, int strip_rows, int strip_count, int strip_index,         \
       int samples, hipStream_t stream))                                                                                   \
    X(pool_blocks_per_cu, rtdev_pool_blocks_per_cu, int,                                                                   \
      (int prims_class, int textured, int specular, int bvh, size_t dyn_lds))                                              \
    X(pool_static_lds, rtdev_pool_static_lds, int, (int prims_class, int textured, int specular, int bvh))                 \
    X(trace_pool, rtdev_launch_trace_pool, hipError_t,                                                                     \
      (const rtdev::TraceArgs *args, const rtdev::PrimaryRects *rects, int prims_class, int textured, int specular,       \
       int bvh, unsigned blocks, hipStream_t stream))                                                                      \
    X(resolve_chunks, rtdev_launch_resolve_chunks, hipError_t,                                                             \
      (const double *partial, double *out, int width, int height, int n_chunks, int slice_rows, int strip_rows,           \
       int strip_count, int strip_index, int step_x, int step_y, int cover_w, int cover_h, int out_col_step, int out_cols, \
       int samples, hipStream_t stream))                                                                                   \
    X(fold_chunks, rtdev_launch_fold_chunks, hipError_t,                                                                   \
      (const double *partial, double *running, double *out, size_t n, int c0, int c1, int samples_done,                   \
       hipStream_t stream))                                                                                                \
    X(fold_adaptive, rtdev_launch_fold_adaptive, hipError_t, (const rtdev::AdaptiveFold *f, hipStream_t stream))           \
    X(nee, rtdev_launch_nee, hipError_t,                                                                                   \
      (const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee, int prims_class, int textured, int specular, int bvh,     \
       hipStream_t stream))                                                                                                \
    X(nee_pass, rtdev_launch_nee_pass, hipError_t,                                                                         \
      (const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee, int prims_class, int textured, int specular, int bvh,     \
       hipStream_t stream))                                                                                                \
    X(nee_chunk, rtdev_launch_nee_chunk, hipError_t,                                                                       \
      (const double *running, double *boundary, double *squares, size_t n, int samples, hipStream_t stream))              \
    X(nee_decide, rtdev_launch_nee_decide, hipError_t, (const rtdev::NeeDecide *f, hipStream_t stream))                    \
    X(nee_stream, rtdev_launch_nee_stream, hipError_t,                                                                     \
      (const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee, int prims_class, int textured, int specular, int bvh,     \
       unsigned blocks, hipStream_t stream))                                                                               \
    X(nee_stream_blocks_per_cu, rtdev_nee_stream_blocks_per_cu, int,                                                       \
      (int prims_class, int textured, int specular, int bvh))                                                              \
    X(nee_stream_chunk, rtdev_nee_stream_chunk, int, (void))                                                               \
    X(nee_lights, rtdev_launch_nee_lights, hipError_t,                                                                     \
      (const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee, const rtdev::NeeLightArgs *lights, int textured,          \
       int specular, int bvh, hipStream_t stream))                                                                         \
    X(nee_lights_pass, rtdev_launch_nee_lights_pass, hipError_t,                                                           \
      (const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee, const rtdev::NeeLightArgs *lights, int textured,          \
       int specular, int bvh, hipStream_t stream))                                                                         \
    X(nee_lights_stream, rtdev_launch_nee_lights_stream, hipError_t,                                                       \
      (const rtdev::TraceArgs *args, const rtdev::NeeArgs *nee, const rtdev::NeeLightArgs *lights, int textured,          \
       int specular, int bvh, unsigned blocks, hipStream_t stream))                                                        \
    X(nee_lights_stream_blocks_per_cu, rtdev_nee_lights_stream_blocks_per_cu, int, (int textured, int specular, int bvh)) \
    X(trace_rays, rtdev_launch_trace_rays, hipError_t,                                                                     \
      (const rtdev::TraceArgs *args, const RtRays *rays, const RtRayHits *hits, const int32_t *order, int n, int any_hit, \
       hipStream_t stream))                                                                                                \
    X(occlusion, rtdev_launch_occlusion, hipError_t,                                                                       \
      (const rtdev::TraceArgs *args, const RtRays *rays, int32_t *occluded, int n, hipStream_t stream))                    \
    X(multihit, rtdev_launch_multihit, hipError_t,                                                                         \
      (const rtdev::TraceArgs *args, const RtRays *rays, const RtRayHits *hits, int32_t *count, const int32_t *order,     \
       int n, int k, hipStream_t stream))                                                                                  \
    X(ambient, rtdev_launch_ambient, hipError_t,                                                                           \
      (const rtdev::TraceArgs *args, const RtRays *points, int n, const RtAmbientParams *params, double default_time,      \
       int32_t *open, double *frame, const int32_t *obj_id, const RtAmbientRays *walked, hipStream_t stream))
#define RT_DECLARE_LAUNCHER(member, name, ret, params) \
    extern "C" ret name params;                        \
    extern "C" ret name##_exact params;
RT_LAUNCHER_LIST(RT_DECLARE_LAUNCHER)
#undef RT_DECLARE_LAUNCHER

namespace rtapi {

// The launchers of one arithmetic flavour (rt_scene_create.hip: kFastLaunchers, kExactLaunchers); a scene points to its own.
struct Launchers {
#define RT_LAUNCHER_MEMBER(member, name, ret, params) ret(*member) params;
    RT_LAUNCHER_LIST(RT_LAUNCHER_MEMBER)
#undef RT_LAUNCHER_MEMBER
};

#define RT_HIP(call)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return rtapi::fail(RT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));  \
    } while (0)

// How a caller asks for cancellation: the flag of rt_render, the callback of rt_render_ex, or neither.
// Polled by the calling thread only.
struct Cancel {
    const volatile int *flag = nullptr;
    int (*fn)(void *) = nullptr;
    void *user = nullptr;
    bool armed() const { return flag != nullptr || fn != nullptr; }
    bool raised() const { return (flag && *flag) || (fn && fn(user) != 0); }
};

// Where a launch's finished pixels go when the launch delivers them itself (TraceArgs.deliver_*; rt_deliver.hip).
struct Delivery {
    double *out = nullptr;              // device-visible address of the output (pinned host memory or HBM)
    int col_step = 0, cols = 1;         // tile-column layout; cols == 1: plain [H][W][3] with col_step == width
    std::vector<rtdev::Region> regions; // rt_plan.h: frame_bands / stream_windows, in queue order (queue_order fills item_begin in)
    uint32_t serial = 0;                // value published in the scene's host_flags[region]
    bool cancellable = false;           // the caller polls a cancel hook while this launch runs: the waves read the scene's cancel word
    // rt_render_nee: the launch is k_nee_stream_f64's with this light sampling (rt_nee.hip: enqueue_nee_stream), not the pooled kernel's
    const RtLightSamplingParams *nee = nullptr;
};

// Everything a render allocates on first use — slices, the v1 accumulator, frames, the packed RGBA, counters, the pinned
// frame and flags, streams, events — kept per device across rt_scene_destroy / rt_scene_create (rt_render_cache.h), which
// move the whole set.  Every resource is an owner of rt_resources.h: the set frees itself, on its own device, and a member
// added here needs no other line anywhere.  The members are declared streams, events, memory, so that they go in the
// reverse order: memory, then events, then streams.
struct RenderBuffers {
    OwnersDevice device;                // the scene's; made current (and left current) before the members are freed
    Stream stream;                      // used by the host-output entry points
    // cancel: the stream whose command processor overwrites the launches' item counters (rt_api.hip: poison_queue)
    Stream stream_ctl;
    // rt_render_progressive (rt_progressive.hip), made on its first call: the stream that copies a pass's frame to the host
    // and, per frame slot (two; three for rt_render_adaptive), the pass's trace span, the end of its fold, the end of the
    // copy of its running-tile count (adaptive) and the end of its frame's copy
    Stream stream_copy;
    Event ev_begin, ev_traced, ev_resolved;
    Event ev_pass_begin[3], ev_pass_traced[3];
    Event ev_folded[3], ev_counted[3], ev_copied[3];

    DevBuf<double> partial;             // [chunks][owned rows][W][3] per-chunk sums (pooled kernel)
    DevBuf<unsigned int> queue;         // one item counter per launch of a render call
    DevBuf<double> accum;               // running sums, W*H*3 (v1 kernel; the passes of rt_render_progressive)
    DevBuf<double> frame;               // resolved frame for the host-output entry points (two of them for rt_render_progressive)
    // rt_render_adaptive (rt_progressive.hip), on first use: the running sums of squares (W*H*3), per tile its stop, its
    // scale and its error in three pass slots, two tile lists and one running-tile count per pass (+ their pinned copies)
    DevBuf<double> squares, tile_scale, tile_err;
    DevBuf<int32_t> tile_stop;
    DevBuf<uint32_t> tile_lists, tile_counts;
    PinnedBuf<uint32_t> host_counts;    // [RT_MAX_CHUNKS]
    DevBuf<uint8_t> rgba;               // packed frame of rt_render_frame_rgba8
    DevBuf<unsigned long long> segments; // rt_device_types.h: RT_STAT_*
    // Delivery (rt_deliver.hip): the launch writes finished pixels straight into `host_frame` — pinned, portable host
    // memory mapped into every device, so several scenes (devices) can fill one frame — and publishes finished regions
    // in `host_flags`; tile_done / region_done are the device counters behind that (zero between launches).
    PinnedBuf<double> host_frame;
    PinnedBuf<unsigned int> host_flags; // [RT_MAX_REGIONS] published regions + [1] the cancel word the waves read (TraceArgs.cancel_flag)
    DevBuf<unsigned int> tile_done, region_done;
    uint32_t deliver_serial = 0; // the flags still hold the serials this set published: the counter moves on with the set
    bool deliver_dirty = false;  // a delivering launch was cut short: the counters must be cleared before the next one
    // denoising (rt_denoise.hip), made on first use: the guides of rt_denoise_frame and rt_render_progressive_denoised —
    // planes [normal 3 | position 3 | albedo 3 | footprint 1] x W*H doubles and obj_id x W*H — and the filter's two
    // ping-pong buffers of W*H*3 doubles each
    DevBuf<double> guide_planes, denoise_scratch;
    DevBuf<int32_t> guide_ids;
    // rt_render_adaptive_filtered (rt_variance_filter.hip), on first use: every pixel's samples and chunks, W*H each
    DevBuf<int32_t> batch_counts;
    // the host forms of the ray queries (rt_query_stage.h), on first use: one chunk of rays — planes [origin 3 | direction 3 |
    // t_min | t_max | time] x RT_RAYS_HOST_CHUNK doubles — and of answers — [t | point 3 | normal 3 | uv 2] doubles, [prim |
    // obj_id | front_face] (rt_trace_occlusion stages through rays_in and the first plane of rays_ids; rt_trace_rays_multi
    // through all three, an eighth of a chunk's rays at a time with up to eight slots each)
    DevBuf<double> rays_in, rays_out;
    DevBuf<int32_t> rays_ids;

    RenderBuffers() = default;
    RenderBuffers(RenderBuffers &&) = default;
    // what the target held is freed as a whole set — on ITS device, in the order above — before it takes the other over
    RenderBuffers &operator=(RenderBuffers &&o) noexcept {
        if (this != &o) {
            this->~RenderBuffers();
            new (this) RenderBuffers(std::move(o));
        }
        return *this;
    }
    ~RenderBuffers() { device.make_current(); }

    // what rt_scene_create makes when it takes no set over: only such a set is worth caching
    bool complete() const {
        return stream && stream_ctl && ev_begin && ev_traced && ev_resolved && host_flags.ptr && segments.ptr;
    }
};

} // namespace rtapi

// The device launchers of rt_denoise.hip (compiled once, RT_ARITH_FAST): guide rays of a whole frame, and one step of the
// filter — demodulation (`step` < 0), a-trous iteration `step` (0-based), remodulation (`step` == iterations).
extern "C" hipError_t rtdev_launch_guides(const rtdev::TraceArgs *args, const RtGuides *guides, hipStream_t stream);
extern "C" hipError_t rtdev_launch_denoise_step(const RtDenoiseParams *d, int step, int width, int height, const double *in,
                                                const RtGuides *guides, double *out, hipStream_t stream);
// ... of rt_temporal.hip (compiled once, RT_ARITH_FAST): the launcher of level `step` of the variance-guided filter
// (k_temporal_atrous) — rtdev_launch_denoise_step's parameters, the luminance stop sigma_l > 0 and the variance planes
// beside the colour ones.  Linked inside the library only: rtapi::enqueue_levels (rt_denoise.hip) runs these levels for
// rt_temporal.hip and rt_variance_filter.hip alike.
extern "C" __attribute__((visibility("hidden"))) hipError_t rtdev_launch_atrous_var(
    const RtDenoiseParams *d, double sigma_l, int step, int width, int height, const double *in, const double *var,
    const RtGuides *guides, double *out, double *var_out, hipStream_t stream);

struct RtScene {
    int device = 0;
    rtapi::DevBuf<rtdev::Prim> prims;
    rtapi::DevBuf<rtdev::Texture> textures;
    rtapi::DevBuf<rtdev::Image> images;
    rtapi::DevBuf<rtdev::Perlin> perlins;
    std::vector<rtapi::DevBuf<uint8_t>> image_pixels; // device copies of the RGBA8 texels
    int n_prims = 0, n_materials = 0, n_textures = 0, n_images = 0, n_perlins = 0;
    int perlin_identity = 1; // all permutation tables are the identity (noise.rs:121-130 never shuffles them)
    rtdev::Background bg;
    // kernel specialisation of both trace kernels (rt_trace_kernel.hip, rt_trace_pool_kernel.hip; rtdev::PRIMS_*):
    // 0 rects only, 1 spheres only, 2 anything
    int prims_class = 2;
    int rect_end[3] = {0, 0, 0}; // linear loop: ends of the XY / XZ / YZ rect groups of the (grouped) device table
    int sphere_end = 0;          // ... and of the plain-sphere group behind them
    int box_end = 0;             // ... and of the boxes (wrapped or not) behind those
    int textured = 0; // some material's texture is not a plain SolidColor
    // upper bound of a finished sample's radiance (every attenuation in [0, 1]; emission, background and the depth-0 white
    // below it), or 0 when the scene has none (rt_plan.cpp: scene_radiance_bound): what sizes the pooled kernel's fixed-point sums
    double radiance_bound = 0.0;
    int specular = 0; // some material is Metal or Dielectric
    int has_moving = 0; // some primitive is a MovingSphere (the only reader of a ray's time)
    // union of the primitives' bounds (rt_bvh.h: primitive_bounds), for the pixel rectangle camera rays can hit anything
    // in (rt_primary_bounds.h); empty (mn > mx) for a scene without primitives
    double box_mn[3] = {1.0, 1.0, 1.0}, box_mx[3] = {-1.0, -1.0, -1.0};
    // the records of a linear table of plain rects only, in device table order, for their own pixel rectangles
    // (rt_primary_bounds.h: primary_rects); empty for every other table and for one of more than RT_PRIMARY_RECTS records
    std::vector<rtdev::RectGeo> primary_rect_geo;

    // closest hit: linear loop for small scenes, skip-link BVH (rt_bvh.h) above kBvhThreshold primitives
    int use_bvh = 0;
    rtapi::DevBuf<rtdev::BvhNode> bvh_nodes;
    rtapi::DevBuf<rtdev::BvhNode> bvh_nodes_ordered; // eight direction-ordered copies (trees that do not fit LDS)
    rtapi::DevBuf<int32_t> bvh_prim_index;
    rtapi::DevBuf<rtdev::LeafGeo> leaf_geo; // what a leaf test reads (rt_device_types.h)
    double leaf_time_a = 0.0, leaf_inv_dt = 1.0;
    int n_bvh_nodes = 0;
    double bvh_root_mn[3] = {0, 0, 0}, bvh_root_mx[3] = {0, 0, 0}, bvh_center[3] = {0, 0, 0};
    bool bvh_nodes_in_lds = false; // node array (32 B each) staged in dynamic LDS when <= 32 KiB
    // the tree on the host, for trees that live in LDS: before a launch the node array is re-emitted with every node's
    // children nearest-to-the-camera first (rt_bvh.h: order_bvh_for_origin) whenever the camera has moved
    rtdev::BvhBuild bvh_host;
    double bvh_ordered_for[3] = {0, 0, 0};
    bool bvh_is_ordered = false;
    std::vector<rtdev::BvhNode> bvh_ordered_nodes[2]; // host copies of the array last uploaded and the one before
    int bvh_upload_slot = 0;

    // pooled kernel (default): persistent grid = CUs x resident blocks of the variant
    bool use_v1 = false;   // RtSceneOptions.kernel == RT_KERNEL_V1: the lane-per-pixel kernel
    bool exact = false;    // RtSceneOptions.arithmetic == RT_ARITH_REFERENCE: the *_exact copy of the trace kernels
    const rtapi::Launchers *kernels = nullptr; // ... and their launchers (rt_scene_create.hip: scene_create)
    bool gather_staged = false; // RtSceneOptions.gather == RT_GATHER_STAGED (rt_multi.hip)
    // RtSceneOptions.launch_blocks: 0, or the most blocks a persistent launch of this scene gets (cap_blocks below), and
    // what the most recent such launch got: its blocks and its items (rtdev_scene_variant)
    int launch_blocks = 0;
    int last_launch_blocks = 0, last_launch_items = 0;
    int num_cus = 0, pool_blocks_per_cu = 1;
    int pool_blocks_per_cu_lens = 1; // ... when the camera has an aperture (its lens samples take dynamic LDS)
    int pool_static_lds = 0;         // static LDS of the variant's kernel (hipFuncGetAttributes)
    size_t pool_dyn_lds = 0, pool_dyn_lds_lens = 0; // its dynamic LDS without / with lens samples (rt_device_types.h: pool_lds_layout)

    // next-event estimation (rt_nee.hip): the listed lights as description indices, in table order (at most 64), and on
    // the device rtdev::NeeArgs' slot per device primitive and device primitive per light
    std::vector<int32_t> lights;
    rtapi::DevBuf<int32_t> nee_slot, nee_prim;
    // the extended list (rt_scene_set_lights): what is needed to list again — the facts of every primitive and the
    // description index of every device record —, the params in force (all zero: rt_scene_create's list), whether the
    // launches take the extended-light kernels (the list holds a wrapped, box or moving light, or the pick is by power),
    // and the pick of every cap: for n = 1 .. count lights in play, row n - 1 of nee_pick holds p_0 .. p_{count-1} and
    // cdf_0 .. cdf_{count-1} (2 * count doubles a row; entries >= n unused), pick_uniform[n - 1] whether that cap's pick
    // is the uniform one
    std::vector<rtapi::LightFact> light_facts;
    std::vector<int32_t> table_order;
    RtLightListParams light_params = {};
    bool lights_extended = false;
    rtapi::DevBuf<double> nee_pick;
    std::vector<char> pick_uniform;
    std::vector<double> pick_weights; // p_k of the uncapped list (rt_scene_light_weights)
    // ray queries (rt_query.hip): table_order on the device, made by the scene's first query that names primitives
    rtapi::DevBuf<int32_t> rays_order;

    rtapi::RenderBuffers buf;
    bool has_stats = false;
    int last_launches = 0;
    // rt_render_progressive: the call's kernel and fold times, summed over its passes, stand in for the event spans
    bool summed_times = false;
    double summed_kernel_ms = 0.0, summed_resolve_ms = 0.0;
};

namespace rtapi {
// A launch whose waves read the scene's cancel word (the slot behind the region flags): lowered, and named in its arguments
inline void arm_cancel_word(RtScene *s, rtdev::TraceArgs &a) {
    s->buf.host_flags.ptr[rtdev::RT_MAX_REGIONS] = 0u;
    a.cancel_flag = s->buf.host_flags.ptr + rtdev::RT_MAX_REGIONS;
}
// The resident blocks of a persistent kernel on the device, under the scene's launch_blocks cap (0: none).  A cap only
// lowers the count: every block of the launch stays co-resident.
inline unsigned cap_blocks(const RtScene *s, unsigned resident) {
    return s->launch_blocks > 0 && (unsigned)s->launch_blocks < resident ? (unsigned)s->launch_blocks : resident;
}
// The grid of a persistent launch, where it is computed: kept for rtdev_scene_variant
inline void note_grid(RtScene *s, unsigned blocks, uint32_t n_items) {
    s->last_launch_blocks = (int)blocks;
    s->last_launch_items = (int)n_items;
}
// A call has enqueued its (first) launches: rt_scene_last_stats reads the counters and the event spans of this call
inline void note_launches(RtScene *s, int launches) {
    s->has_stats = true;
    s->last_launches = launches;
    s->summed_times = false;
}
// The last check of a device-side entry point and its first step: there is a scene, and its device is the current one
inline int use_scene_device(const RtScene *s) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    RT_HIP(hipSetDevice(s->device));
    return RT_OK;
}
} // namespace rtapi

// Internal exports for the tests (not part of rt_abi.h; the ABI version does not cover them).
//   rtdev_progressive_passes: the samples_done of every pass of rt_render_progressive(samples, pass_samples), in order, into
//     out (at most n_out of them), and their number into n_passes.  No device needed.
//   rtdev_scene_variant: what rt_scene_create_ex chose for a scene, RTDEV_VARIANT_FIELDS values in this order:
//     kernel (0 pool, 1 v1), prims_class (rtdev::PRIMS_*), textured, specular, use_bvh, exact (RT_ARITH_REFERENCE kernels),
//     bvh_nodes_in_lds, has_moving, perlin_in_lds, static LDS of the pool variant, its dynamic LDS without and with lens
//     samples (bytes; 0 for v1), resident blocks per CU without and with lens samples, last_launch_blocks and
//     last_launch_items: the block count and n_items of the scene's most recent persistent launch (pooled kernel, NEE
//     stream kernels; 0 before the first), which is how a test sees that RtSceneOptions.launch_blocks took effect.
//     Writes min(n_out, fields) values.
//   rtdev_scene_classify: the selection rule of rt_scene_create_ex on a description alone (no device): prims_class, textured,
//     specular, has_moving.  Returns the description's validation error, if any.
//   rtdev_scene_radiance_bound: the bound on a finished sample's radiance that rt_scene_create_ex gives a description
//     (RtScene.radiance_bound), or 0: none (f64 sums).  Returns the description's validation error, if any.
//   rtdev_sum_exponent: the exponent e of the fixed-point sums (TraceArgs.sum_scale = 2^(52-e)) that a render of `samples`
//     samples per pixel gets from a radiance bound, or e = 0: f64 sums; RT_ERR_UNSUPPORTED where the render is refused
//     (rt_plan.cpp: sum_exponent).
#define RTDEV_VARIANT_FIELDS 16
extern "C" int rtdev_scene_variant(const RtScene *s, int32_t *out, int32_t n_out);
extern "C" int rtdev_scene_classify(const RtSceneDesc *d, int32_t out[4]);
extern "C" int rtdev_scene_radiance_bound(const RtSceneDesc *d, double *bound);
extern "C" int rtdev_sum_exponent(double bound, int32_t samples, int32_t *e);
extern "C" int rtdev_progressive_passes(int32_t samples, int32_t pass_samples, int32_t *out, int32_t n_out, int32_t *n_passes);

namespace rtapi {
// Enqueue trace + resolve on `stream` (two-pass path: the resolve kernel writes out_device), or — with a Delivery —
// ONE delivering launch that finishes its own pixels (out_device is ignored).  `cancel` is polled before every launch:
// between the sample batches of the v1 kernel, between the chunk batches of the pooled one (whose waves also read the
// scene's cancel word while `cancel` is armed).  Returns RT_ERR_CANCEL_EVENT when cancelled (callers map that to RT_OK).
// out_col_step / out_cols: layout the RESOLVE pass of the two-pass path writes (rt_frame_kernels.hip:
// k_resolve_chunks_f64): the plain frame, or the tile stream's column layout.
int enqueue_render(RtScene *s, const RtCamera *camera, const RtRenderParams *p, double *out_device,
                   hipStream_t stream, int batch, const Cancel &cancel, const Delivery *delivery = nullptr,
                   int out_col_step = 0, int out_cols = 1);
// Allocate now what enqueue_render would allocate for these parameters (calls over several shares: before the first launch).
int reserve_render_buffers(RtScene *s, const RtRenderParams *p, bool delivering);
// Block until `ev` has happened, polling `cancel` meanwhile (RT_ERR_CANCEL_EVENT as soon as it is raised).
int wait_event(hipEvent_t ev, const Cancel &cancel);
// Ends the pool launches in flight on `s` early: every item counter becomes 2^31 (rt_api.hip).
int poison_queue(RtScene *s);
// The same without waiting for the write to land: several shares are poisoned side by side (rt_deliver.hip: abort_shares) —
// a share whose launch still waits behind another share's on the SAME device only reaches its ev_begin when that one ends,
// and waiting for it before poisoning the next would let the next run to its end.
int poison_queue_begin(RtScene *s);
// A whole-frame render of the pooled kernel enqueued chunk range by chunk range (rt_progressive.hip): begin_passes checks the
// render as enqueue_render does and enqueues what precedes its first launch — counters cleared (one item counter per
// launch, max_launches of them), the cancel word armed when `cancellable`, the tree ordered for the camera, ev_begin —
// and enqueue_chunks launches chunks [c0, c1) of every tile into their slices.  The launches share one set of segment
// counters, so rt_scene_last_stats counts the whole call.  Buffers must be reserved first (reserve_render_buffers).
struct PoolPasses {
    rtdev::TraceArgs args;
    std::vector<int> starts; // chunk_plan(samples)
    unsigned max_blocks = 0; // resident blocks of the variant on the device
    int launches = 0, max_launches = 0;
};
int begin_passes(RtScene *s, const RtCamera *camera, const RtRenderParams *p, hipStream_t stream, int max_launches,
                 bool cancellable, PoolPasses &pp);
// tile_list: NULL (every tile) or n_list tiles of the grid in device memory (TraceArgs.tile_list).
int enqueue_chunks(RtScene *s, PoolPasses &pp, int c0, int c1, hipStream_t stream, const uint32_t *tile_list = nullptr,
                   uint32_t n_list = 0);
// Denoising (rt_denoise.hip).  check_denoise: the filter's parameters (NULL, iterations, sigmas, _reserved) and a whole
// frame's size (strips and scale > 1 refused).  reserve_denoise: the filter's scratch (with `variance_planes`, that of
// enqueue_levels) and, with `own_guides`, the scene's guide planes for a W*H frame, before the first launch.
// scene_guides: those planes as an RtGuides.  enqueue_guides / enqueue_denoise: the guide launch and the filter's
// launches on `stream` (arguments checked by the caller).
int check_denoise(const RtRenderParams *p, const RtDenoiseParams *d);
// What the three filter units (rt_denoise.hip, rt_temporal.hip, rt_variance_filter.hip) share on the host.
// guides_complete: no NULL among a caller's guide planes.  pixel_grid: 16x16 pixels per block of 256 lanes.
// filter_stops: the inverse sigmas of a-trous level `level` (step 2^level) as the kernels take them, 0 where a stop is
// off; level 0 is also the 7x7 variance windows' (step 1; they have no colour stop).
bool guides_complete(const RtGuides *g);
dim3 pixel_grid(int width, int height);
struct FilterStops {
    double inv_sn2; // 1 / sigma_n^2
    double inv_sx;  // 1 / (sigma_x * 2^level)
    double inv_sc2; // 1 / (sigma_c * 2^-level)^2
};
FilterStops filter_stops(const RtDenoiseParams *d, int level = 0);
// What the entry points that take a preview frame (rt_upsample.hip, rt_preview_temporal.hip) refuse about params and
// denoise; `full` becomes params at full resolution (scale 0), what the guides and the filter's levels take.
int check_upsample(const RtRenderParams *p, const RtDenoiseParams *d, RtRenderParams &full);
// ... and what their kernels' argument blocks (UpsampleArgs, PreviewAccumulateArgs) say about such a frame: the image, the
// preview's grid with its anchors per row and column, and the blend's stops
template <class Args> void fill_upsample_args(Args &a, const RtRenderParams *p, const RtDenoiseParams *d) {
    const PreviewGrid pg = preview_grid(p);
    a.width = p->width;
    a.height = p->height;
    a.step_x = pg.step_x;
    a.step_y = pg.step_y;
    a.gx = p->width / pg.step_x;
    a.gy = p->height / pg.step_y;
    a.demodulate = (d->flags & RT_DENOISE_DEMODULATE) != 0;
    a.inv_sn2 = filter_stops(d).inv_sn2;
    a.inv_sx = d->sigma_plane > 0.0 ? 1.0 / (d->sigma_plane * (double)(pg.step_x > pg.step_y ? pg.step_x : pg.step_y)) : 0.0;
}
// The levels of a demodulated frame and its re-modulation into `out`: plain levels (rt_denoise_device's) with
// sigma_l <= 0, else variance-guided ones over `variance` (W*H).  The scene's scratch holds two colour buffers and, behind
// them, two variance planes (8 W*H doubles, reserved here); `variance` may be the SECOND of those planes — level 0 reads
// it and writes the first, level 1 swaps them — or the caller's own.
int enqueue_levels(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, double sigma_l, const double *radiance,
                   const double *variance, const RtGuides &g, double *out, hipStream_t stream);
// The trace kernels' argument block of a render (rt_api.hip: fill_args), for launches of other kernels that trace rays.
int fill_trace_args(const RtScene *s, const RtCamera *camera, const RtRenderParams *p, rtdev::TraceArgs &a);
// ... its scene part alone, for the kernels that take caller rays (rt_query.hip): the tree when the scene
// walks one (use_bvh), and of a tree that renders keep in LDS its global copy.
int query_args(const RtScene *s, rtdev::TraceArgs &a);
// The device copy of RtScene.table_order in s->rays_order, made by the scene's first query that names primitives
// (rt_query.hip), with one synchronous copy.
int ensure_order(RtScene *s);
int reserve_denoise(RtScene *s, size_t pixels, bool own_guides, bool variance_planes = false);
RtGuides scene_guides(RtScene *s, size_t pixels);
int enqueue_guides(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtGuides &g, hipStream_t stream);
int enqueue_denoise(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const double *rgb, const RtGuides &g,
                    double *out, hipStream_t stream);
// The scene's light list (rt_nee.hip) on the device, made by rt_scene_create once the device table's order is final
// (rt_plan.h: light_tables).
int build_light_list(RtScene *s, const LightTables &t);
// ... listed again from the scene's own facts with these (checked) params, the pick tables with it (rt_scene_set_lights).
int set_light_list(RtScene *s, const RtLightListParams &lp);
// What every NEE entry point refuses before a device is touched (rt_nee.hip), the scene last so that each refusal names
// its own cause; `what` is the entry point's name in the messages about whole frames.
// `strips`: params->strip_count > 1 is not refused (rt_render_frame_nee_strips_device; check_params holds the strip values).
int check_nee(const RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
              const char *what = "rt_render_frame_nee", bool strips = false);
// ... the part about camera, params and light sampling alone, short of check_params (the several-scene calls, rt_deliver.hip
// and rt_multi.hip, check their scene list next).
int check_nee_args(const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls, const char *what,
                   bool strips = false);
// rt_render_frame_nee_device's launches for the rows `p` owns (rt_nee.hip): k_nee_f64 into the scene's full-frame
// accumulator, then the resolve pass of the owned rows into out_device (a full frame; rows not owned are not written), on
// `stream`, not synchronised.  A share that owns no rows launches nothing (note_idle_share).  reserve_nee_buffers
// allocates now what enqueue_nee (`delivering` false) or enqueue_nee_stream (true) would allocate for these parameters: a
// call over several shares reserves for all of them before its first launch.  note_idle_share gives a share that launched
// nothing the statistics of an empty call (no sample, no segment, kernel_launches 0).
int enqueue_nee(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls, double *out_device,
                hipStream_t stream);
int reserve_nee_buffers(RtScene *s, const RtRenderParams *p, bool delivering);
int note_idle_share(RtScene *s, hipStream_t stream);
// The counters of a delivering launch over `n_tiles` item tiles (rt_api.hip; zero between launches).
int reserve_delivery_counters(RtScene *s, size_t n_tiles);
// A whole NEE frame enqueued pass by pass (rt_progressive.hip), the NEE form of begin_passes / enqueue_chunks:
// begin_nee_passes fills the argument blocks and enqueues what precedes the first launch — statistics cleared, the cancel
// word armed when `cancellable`, ev_begin — and enqueue_nee_pass launches, chunk by chunk of [c0, c1), k_nee_pass_f64 for
// the listed tiles on top of the scene's running sums and k_nee_chunk_f64 behind it (RenderBuffers.accum, .squares and
// .partial — here the sums at the last chunk boundary, W*H*3 —, all cleared by the caller before pass 0).
struct NeePasses {
    rtdev::TraceArgs args;
    rtdev::NeeArgs nee;
    rtdev::NeeLightArgs lights; // read by the extended-light kernels only (RtScene.lights_extended)
    std::vector<int> starts; // chunk_plan(samples)
};
int begin_nee_passes(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                     hipStream_t stream, bool cancellable, NeePasses &np);
int enqueue_nee_pass(RtScene *s, NeePasses &np, int c0, int c1, hipStream_t stream, const uint32_t *tile_list = nullptr,
                     uint32_t n_list = 0);
// rt_render_nee's delivering launch (rt_nee.hip): k_nee_stream_f64 as one persistent grid over delivery.regions (one item per
// tile), finishing its own pixels in delivery.out; everything it needs is allocated first, ev_begin / ev_traced /
// ev_resolved span it.  ... and the frame behind its fallback: rt_render_frame_nee's launch and resolve into the scene's
// device frame, copied into `out` (host memory, W*H*3), arguments checked by the caller.
int enqueue_nee_stream(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                       const Delivery &delivery);
int nee_frame_to_host(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls, double *out);
// A delivering launch's regions and counters in its argument block (rt_api.hip): the regions in queue order for
// `chunks_per_tile` items per tile (rt_plan.h: queue_order, which refuses a list that does not fit the tile grid), the
// counters cleared where a launch was cut short, TraceArgs.deliver_*.
int setup_delivery(RtScene *s, rtdev::TraceArgs &a, const Delivery &delivery, int chunks_per_tile, hipStream_t stream);
// The pinned host frame of the host-output entry points, at least `doubles` long (rt_deliver.hip).
int ensure_host_frame(RtScene *s, size_t doubles);
// The several-device calls (rt_deliver.hip, rt_multi.hip): a non-empty list of distinct, non-NULL scenes.
int check_scenes(RtScene *const *scenes, int n);
// ... of the NEE forms (rt_deliver.hip): check_nee_args, check_scenes, strip_rows >= 0, check_params — no device touched.
int check_nee_shares(RtScene *const *scenes, int n, const RtCamera *camera, const RtRenderParams *p,
                     const RtLightSamplingParams *ls, int strip_rows, const char *what);
// ... and, behind every other refusal of the entry point: the scenes carry the same light list params (rt_scene_set_lights).
int check_same_light_lists(RtScene *const *scenes, int n, const char *what);
} // namespace rtapi
