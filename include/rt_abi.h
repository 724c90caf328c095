/* rt_abi.h — C ABI of the MI355X render path (libracer_tracer_amd.so).
 *
 * This is the drop-in boundary for racer-tracer's renderer: everything the
 * reference does between `Renderer::render` being called and the
 * `ImageBufferEvent::BufferUpdate` tiles coming out
 * (racer-tracer/src/renderer.rs:101-107, renderer/cpu.rs:26-131) happens
 * behind the functions declared here.  The signatures use plain C types
 * only (pointers, sizes, PODs) so that a Rust `impl Renderer` can bind them
 * with `extern "C"` unchanged; INTEGRATION.md shows that binding.
 *
 * Every struct is a flattened ("described") form of a reference trait
 * object; the comment on each one names the Rust type it replaces.
 * All floating point is f64 like the reference (vec3.rs:13-16).
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 5

/* ------------------------------------------------------------------ errors
 * 0 = Ok.  1..22 are exactly the reference's exit codes
 * (racer-tracer/src/error.rs:71-97).  Codes >= 100 are new, GPU-side. */
enum RtError {
    RT_OK = 0,
    RT_ERR_FAILED_TO_CREATE_WINDOW = 1,
    RT_ERR_FAILED_TO_UPDATE_WINDOW = 2,
    RT_ERR_CONFIGURATION = 3,
    RT_ERR_UNKNOWN_MATERIAL = 4,
    RT_ERR_FAILED_TO_ACQUIRE_LOCK = 5,
    RT_ERR_EXIT_EVENT = 6,
    RT_ERR_CANCEL_EVENT = 7,
    RT_ERR_IMAGE_SAVE = 8,
    RT_ERR_SCENE_LOAD = 9,
    RT_ERR_ARGUMENT_PARSING = 10,
    RT_ERR_KEY = 11,
    RT_ERR_CREATE_LOG = 12,
    RT_ERR_RECEIVE = 13,
    RT_ERR_SEND = 14,
    RT_ERR_ACTION_PROTOCOL = 15,
    RT_ERR_BUS_WRITE = 16,
    RT_ERR_BUS_READ = 17,
    RT_ERR_BUS_UPDATE = 18,
    RT_ERR_BUS_TIMEOUT = 19,
    RT_ERR_NO_OBJECT_WITH_ID = 20,
    RT_ERR_FAILED_TO_OPEN_IMAGE = 21,
    RT_ERR_FAILED_TO_PARSE = 22,
    /* new */
    RT_ERR_NO_DEVICE = 100,      /* no HIP device / runtime unusable */
    RT_ERR_HIP = 101,            /* a HIP call failed; see rt_last_error_message */
    RT_ERR_INVALID_ARGUMENT = 102,
    RT_ERR_UNSUPPORTED = 103,    /* scene uses something the device path lacks */
    RT_ERR_OUT_OF_MEMORY = 104
};

/* ---------------------------------------------------------------- textures
 * Flattened `dyn Texture` (texture.rs:8-10). */
enum RtTextureKind {
    RT_TEX_SOLID_COLOR = 0, /* texture/solid_color.rs:24-28  : color            */
    RT_TEX_CHECKERED = 1,   /* texture/checkered.rs:32-42    : tex_even, tex_odd */
    RT_TEX_IMAGE = 2,       /* texture/image.rs:28-51        : image            */
    RT_TEX_NOISE = 3        /* texture/noise.rs:26-33        : color, scale, depth, perlin */
};

typedef struct RtTexture {
    int32_t kind;
    int32_t tex_even; /* Checkered: index of `texture_a` (used when sines >= 0) */
    int32_t tex_odd;  /* Checkered: index of `texture_b` (used when sines <  0) */
    int32_t image;    /* Image: index into RtSceneDesc.images                   */
    int32_t perlin;   /* Noise: index into RtSceneDesc.perlins                  */
    int32_t depth;    /* Noise: turbulence octaves                              */
    double color[3];  /* SolidColor / Noise colour                              */
    double scale;     /* Noise scale                                            */
} RtTexture;

/* Decoded image of a TextureImage: RGBA8, row-major, row 0 = top
 * (what `image::open(..).into_rgba8()` yields, texture/image.rs:18-24). */
typedef struct RtImage {
    const uint8_t *rgba;
    int32_t width;
    int32_t height;
} RtImage;

/* One `Perlin` (texture/noise.rs:36-55): 256 unit gradient vectors and the
 * three permutation tables (identity in the reference, noise.rs:121-130). */
typedef struct RtPerlin {
    double ranvec[256][3];
    int32_t perm_x[256];
    int32_t perm_y[256];
    int32_t perm_z[256];
} RtPerlin;

/* --------------------------------------------------------------- materials
 * Flattened `dyn Material` (material.rs:10-15). */
enum RtMaterialKind {
    RT_MAT_LAMBERTIAN = 0,   /* material/lambertian.rs:26-38   */
    RT_MAT_METAL = 1,        /* material/metal.rs:26-43        */
    RT_MAT_DIELECTRIC = 2,   /* material/dialectric.rs:25-55   */
    RT_MAT_DIFFUSE_LIGHT = 3 /* material/diffuse_light.rs:25-37 */
};

typedef struct RtMaterial {
    int32_t kind;
    int32_t texture;         /* index into textures (unused for Dielectric) */
    double fuzz;             /* Metal                                       */
    double refraction_index; /* Dielectric                                  */
} RtMaterial;

/* --------------------------------------------------------------- primitives
 * Flattened `SceneObject` + `dyn HittableSceneObject` (scene.rs:24-49).
 * The YAML loader can wrap an object in at most one RotateY and then at
 * most one Translate (scene/yml.rs:401-439), so the instance chain is two
 * optional fields instead of a tree. */
enum RtPrimitiveKind {
    RT_PRIM_SPHERE = 0,  /* geometry/sphere.rs  : p = cx, cy, cz, radius        */
    RT_PRIM_XY_RECT = 1, /* geometry/xy_rect.rs : p = x0, x1, y0, y1, k         */
    RT_PRIM_XZ_RECT = 2, /* geometry/xz_rect.rs : p = x0, x1, z0, z1, k         */
    RT_PRIM_YZ_RECT = 3, /* geometry/yz_rect.rs : p = y0, y1, z0, z1, k         */
    RT_PRIM_BOX = 4,     /* geometry/box.rs     : p = min xyz, max xyz          */
    RT_PRIM_MOVING_SPHERE = 5 /* geometry/moving_sphere.rs : p = cx, cy, cz (at time_a), radius;
                                 center_b = centre at time_b; linear in ray.time()      */
};

enum RtPrimitiveFlags {
    RT_PRIM_HAS_ROTATE_Y = 1, /* geometry/rotate_y.rs, applied first (inner) */
    RT_PRIM_HAS_TRANSLATE = 2 /* geometry/translate.rs, applied second (outer) */
};

typedef struct RtPrimitive {
    int32_t kind;
    int32_t material;
    int32_t flags;
    int32_t obj_id;      /* scene.rs:51,60 (informational; not read by the path) */
    double p[6];
    double rot_sin;      /* sin/cos of radians(degrees), rotate_y.rs:19-28 */
    double rot_cos;
    double translate[3]; /* translate.rs:13-16 */
    double center_b[3];  /* MovingSphere.pos_b (moving_sphere.rs:20-25) */
    double time_a;       /* MovingSphere.time_a / time_b: 0 and 1 in the reference */
    double time_b;       /*   (scene/random.rs:55)                                 */
} RtPrimitive;

/* -------------------------------------------------------------- background
 * Flattened `dyn BackgroundColor` (background_color.rs:3-5). */
enum RtBackgroundKind {
    RT_BG_SKY = 0,  /* background_color.rs:27-33: (1-t)*top + t*bottom */
    RT_BG_SOLID = 1 /* background_color.rs:45-48: `top` holds the colour */
};

typedef struct RtBackground {
    int32_t kind;
    int32_t _pad;
    double top[3];
    double bottom[3];
} RtBackground;

/* ------------------------------------------------------------------- scene
 * `SceneLoadData.objects` + `.background` (scene.rs:109-114) in POD form.
 * The library copies everything it needs in rt_scene_create; the caller
 * may free the arrays afterwards. */
typedef struct RtSceneDesc {
    const RtPrimitive *primitives;
    int32_t n_primitives;
    const RtMaterial *materials;
    int32_t n_materials;
    const RtTexture *textures;
    int32_t n_textures;
    const RtImage *images;
    int32_t n_images;
    const RtPerlin *perlins;
    int32_t n_perlins;
    RtBackground background;
} RtSceneDesc;

/* ------------------------------------------------------------------ camera
 * The 14 fields of `CameraSharedData` (camera.rs:56-72), passed per call
 * because the camera changes between renders (main.rs:178-189). */
typedef struct RtCamera {
    double origin[3];
    double upper_left_corner[3];
    double forward[3];
    double right[3];
    double up[3];
    double horizontal[3];
    double vertical[3];
    double vfov;
    double viewport_width;
    double viewport_height;
    double lens_radius;
    double focus_distance;
    double time_a;
    double time_b;
} RtCamera;

/* ------------------------------------------------------------------ params
 * `Image` (image.rs:3-8) + `RenderConfig` (config.rs:75-82) + the seed the
 * reference does not have (util.rs:9-23 is OS-seeded). */
typedef struct RtRenderParams {
    int32_t width;      /* screen.width  (>= 2: cpu.rs:36 divides by width - 1;   */
    int32_t height;     /* screen.height  >= 2: cpu.rs:40 divides by height - 1)  */
    int32_t samples;    /* render.samples   */
    int32_t max_depth;  /* render.max_depth */
    int32_t tiles_w;    /* render.num_threads_width  (tile grid of rt_render) */
    int32_t tiles_h;    /* render.num_threads_height */
    uint64_t seed;      /* key of the counter-based RNG (rt_rng.h) */
    /* Row ownership for multi-GPU renders: this call renders the image rows
     * r with (r / strip_rows) % strip_count == strip_index and leaves the
     * others untouched.  strip_count <= 1 means "all rows". */
    int32_t strip_rows;
    int32_t strip_count;
    int32_t strip_index;
    /* `scale` of the preview renderer (config.rs:81, renderer/cpu_scaled.rs): 0 or 1
     * = every pixel (CpuRenderer).  scale > 1 = CpuRendererScaled: only the top-left
     * pixel of each scale_w x scale_h block is traced and the block is filled with it,
     * where scale_w = largest divisor <= scale of (width / tiles_w) and likewise for
     * rows (cpu_scaled.rs:18-41); what is left over at the right/bottom edge stays
     * (0,0,0) (cpu_scaled.rs:50-52).  Not combinable with strips. */
    int32_t scale;
} RtRenderParams;

/* ---------------------------------------------------------------- tone map
 * Flattened `dyn ToneMap` (tone_map.rs:14-16) with the parameters its factory
 * resolves (tone_map.rs:18-66); matrices are row-major. */
enum RtToneMapKind {
    RT_TM_NONE = 0,     /* tone_map/none.rs     */
    RT_TM_REINHARD = 1, /* tone_map/reinhard.rs : max_white                       */
    RT_TM_HABLE = 2,    /* tone_map/hable.rs    : hable[6], exposure_bias, linear_white */
    RT_TM_ACES = 3      /* tone_map/aces.rs     : aces_in, aces_out               */
};

typedef struct RtToneMap {
    int32_t kind;
    int32_t _pad;
    double max_white;
    double hable[6]; /* shoulder_strength, linear_strength, linear_angle, toe_strength, toe_numerator, toe_denominator */
    double exposure_bias;
    double linear_white;
    double aces_in[9];
    double aces_out[9];
} RtToneMap;

typedef struct RtScene RtScene; /* opaque; owned by the library */

/* ------------------------------------------------------------ scene options
 * Implementation choices rt_scene_create makes by itself, exposed so that a
 * caller (the parity tests above all) can pin them.  Every combination renders
 * the same picture: closest-hit semantics are those of bvh_node.rs:112-132 in
 * all of them and the pooled and v1 kernels implement the same contract.  The
 * library reads NO environment variable (developer builds with
 * -DRT_DEVELOPER_KNOBS aside). */
enum RtClosestHit {
    RT_HIT_AUTO = 0,   /* linear loop up to 48 primitives, BVH above */
    RT_HIT_LINEAR = 1, /* brute force over the primitive table (it lives in LDS: a few hundred primitives at most) */
    RT_HIT_BVH = 2     /* skip-link BVH */
};
enum RtTraceKernel {
    RT_KERNEL_POOL = 0, /* k_trace_pool_f64: persistent waves over a pool of paths (default) */
    RT_KERNEL_V1 = 1    /* k_trace_f64: lane = pixel; the simple second implementation */
};
/* Arithmetic of the trace kernels.  The reference divides (vec3.rs:79-85 unit_vector, sphere.rs:52,
 * xy_rect.rs:31) and multiplies by 1/x (vec3.rs:279-301) in IEEE f64 without FMA contraction.
 *   RT_ARITH_FAST (default): one reciprocal / reciprocal square root per ray from the hardware seed, refined to
 *     <= 1 ulp, FMA contraction on.  Against the reference's arithmetic (the oracle) the shipped scenes agree to
 *     ~1e-13 per channel; a scene that amplifies rounding (thousands of small mirrors: a bounce multiplies a
 *     direction error by distance / radius) can flip the odd hit, i.e. a few pixels in ten thousand beyond 1e-3.
 *     Scenes with boxes, wrappers, moving spheres or more than 48 primitives add their per-pixel sums in 64-bit fixed
 *     point, which makes the frame independent of how the GPU schedules the work.  That needs a bound E on a sample's
 *     radiance: the largest of 1, the emitted colours and the background's components, with every colour on a
 *     scattering material in [0, 1].  A sample is rounded to a multiple of 2^(e-52), where 2^e is the power of two
 *     above E (the next one when E is within 1e-6 below one) and e grows by one per halving that brings the longest
 *     sample chunk (about spp / 16) to at most 2048 samples; a pixel whose radiance is of that order, black for every
 *     purpose, comes out up to sqrt(2^(e-53)) from the f64 sum's value (4e-8 for E = 15).  Fixed-point sums are used
 *     exactly when E < 2^30 and e <= 31, which keeps that error below 4.9e-4.  A scene without such a bound (a colour
 *     above 1, below 0 or not finite on a scattering material, or E >= 2^30) is rendered as RT_ARITH_REFERENCE; a
 *     render whose sample count would take e past 31 (a bound near 2^30 and more than about 32 768 spp) returns
 *     RT_ERR_UNSUPPORTED — create the scene with RT_ARITH_REFERENCE to render it.
 *   RT_ARITH_REFERENCE: the reference's own operations (IEEE divisions, sqrt + three divisions, no contraction);
 *     holds the 1e-3 per-channel tolerance on such scenes too; ~25 % slower.  Same kernels, same draws, same
 *     closest-hit rule: only the last bits of the arithmetic differ. */
enum RtArithmetic {
    RT_ARITH_FAST = 0,
    RT_ARITH_REFERENCE = 1
};
/* How rt_render_frame_multi_device collects this scene's strips in the output buffer.
 *   RT_GATHER_AUTO (default): a scene on the output's device renders straight into the output; every other one
 *     renders into its own frame and sends its strips by peer copies.
 *   RT_GATHER_STAGED: this scene always takes the second road, also on the output's device — a switch for tests, so
 *     that ONE card executes the staging + strided-copy code that several cards run.  Same frame either way. */
enum RtGather {
    RT_GATHER_AUTO = 0,
    RT_GATHER_STAGED = 1
};
/* launch_blocks: a cap on the grid of this scene's persistent launches — the pooled trace kernel (whole frames, strips,
 * the preview scale, the delivering launch, the passes of rt_render_progressive / rt_render_adaptive with their tile
 * lists) and both NEE stream kernels.  Like RT_GATHER_STAGED a switch for tests: a launch has min(resident blocks,
 * (items + 3) / 4) blocks, so on a large card a wave takes a second work item only in frames of many thousands of items;
 * with launch_blocks = c > 0 a launch has min(that, c) blocks, and a SMALL frame executes the item-after-item code that
 * a full-size frame runs.  It changes no pixel: every sum is either per item (f64 slices) or fixed-point.  0 (default):
 * no cap.  Negative: RT_ERR_INVALID_ARGUMENT.  The v1 kernel and the lane-per-pixel NEE kernels are not persistent and
 * ignore it. */
typedef struct RtSceneOptions {
    int32_t closest_hit; /* RtClosestHit  */
    int32_t kernel;      /* RtTraceKernel */
    int32_t arithmetic;  /* RtArithmetic  */
    int32_t gather;      /* RtGather      */
    int32_t launch_blocks; /* 0: no cap; c > 0: at most c blocks per persistent launch */
    int32_t _reserved[3]; /* must be 0 */
} RtSceneOptions;

/* Statistics of the last render on a scene (path segments = ray_color
 * levels actually evaluated; feeds the roofline figure of bench.py). */
typedef struct RtRenderStats {
    uint64_t samples;        /* primary rays traced               */
    uint64_t segments;       /* sum over samples of path length   */
    double kernel_ms;        /* HIP-event time of the trace kernel(s), this call */
    double resolve_ms;       /* HIP-event time of the resolve kernel, this call  */
    int32_t kernel_launches; /* trace-kernel launches in this call */
    int32_t _pad;
} RtRenderStats;

/* Tile callback = one `ImageBufferEvent::BufferUpdate{rgb,r,c,width,height}`
 * (image_buffer.rs:62-71): `rgb` is width*height*3 f64, row-major, already
 * divided by samples and sqrt'd, NOT tone-mapped (cpu.rs:52,64-70).
 * `rgb` is only valid during the call. */
typedef void (*RtTileCallback)(void *user, const double *rgb, int32_t r, int32_t c,
                               int32_t width, int32_t height);

/* --------------------------------------------------------------- functions
 * Threading (renderer.rs:101: `trait Renderer: Send + Sync`, called from one rayon worker at a
 * time, main.rs:163-199): the library keeps no global state besides the thread-local error text.
 * Different RtScene objects may be used from different threads concurrently; calls on the SAME
 * RtScene must be serialised by the caller (the reference's render task does: one render at a
 * time, scene rebuilt between renders).  Callbacks run on the calling thread. */

/* ABI version of the loaded library (== RT_ABI_VERSION of its build). */
int rt_abi_version(void);

/* Number of usable HIP devices (0 when there is none or the runtime is
 * unusable).  Never fails. */
int rt_device_count(void);

/* Upload a scene to a device.  Replaces handing `&dyn Hittable` +
 * `&dyn BackgroundColor` to the renderer (renderer.rs:92-99); re-doable
 * because the reference rebuilds its BVH between renders (main.rs:178). */
int rt_scene_create(const RtSceneDesc *desc, int device, RtScene **out);
/* Same with explicit options (NULL = defaults = rt_scene_create). */
int rt_scene_create_ex(const RtSceneDesc *desc, int device, const RtSceneOptions *options, RtScene **out);
void rt_scene_destroy(RtScene *scene);
/* rt_scene_destroy keeps what a render allocated (slices, frames, pinned host memory, counters, streams, events) in a
 * per-device cache of at most two sets, and the next rt_scene_create on that device takes a set over: the reference
 * rebuilds its scene on every object event (main.rs:174-189), and a rebuilt scene's first render then costs what any
 * render costs (measured: 4.7 -> 1.6 ms for a 1080p preview, profiles/r04_scene_create.txt).  This gives the cached
 * memory back (e.g. before the process goes on to something else); scenes that are alive are not touched. */
void rt_release_cached_buffers(void);

/* Replaces `CpuRenderer::render` (renderer/cpu.rs:118-131) with the whole
 * frame as ONE BufferUpdate (legal: renderer/image.rs:56-62 does the same).
 * out_rgb: caller-owned HOST memory, width*height*3 f64, row-major, row 0 =
 * top; gamma-encoded (sqrt(sum/samples)), not tone-mapped, not clamped.
 * The launch writes finished pixels into pinned memory itself, band of rows by
 * band of rows, and the call copies a finished band into out_rgb while the GPU
 * renders the next: the frame is in out_rgb a fraction of a millisecond after
 * the last wave ends (no resolve launch, no device-to-host copy afterwards). */
int rt_render_frame(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                    double *out_rgb);

/* Same, but out_rgb_device is DEVICE memory of the scene's device and the
 * work is enqueued on `hip_stream` (a hipStream_t; NULL = default stream)
 * without synchronising: the caller (or a collective on the same stream)
 * orders against it.  Rows not owned under params->strip_* are not written. */
int rt_render_frame_device(RtScene *scene, const RtCamera *camera,
                           const RtRenderParams *params, double *out_rgb_device,
                           void *hip_stream);

/* Cancel hook of rt_render_ex / rt_render_multi = `do_cancel` (renderer.rs:25-30):
 * returns non-zero once the render should stop.  The reference's
 * `RenderData.cancel_event` is an `Option<&synchronoise::SignalEvent>` polled with
 * `wait_timeout(Duration::ZERO)`; a binding passes a function that does exactly
 * that.  Called on the calling thread only, between
 * launches, before every tile callback and every few tens of microseconds while
 * the call waits for the GPU. */
typedef int (*RtCancelCallback)(void *cancel_user);

/* Replaces `CpuRenderer::render` with the reference's own tile stream:
 * tiles_w x tiles_h tiles in column-major order with the last row/column
 * absorbing remainders (cpu.rs:73-115), one callback per tile — tiles_w *
 * tiles_h of them, an empty tile (more tile rows than image rows) included,
 * with width or height 0 — on the calling thread.  Delivery is progressive: ONE launch renders the frame tile
 * column by tile column and writes finished pixels straight into pinned host
 * memory; the callbacks of a finished column run while the GPU works on the
 * next, so tiles arrive during the render as the reference's do (cpu.rs:64-70);
 * their pixels are bit-identical to rt_render_frame's.  `cancel` (may be NULL)
 * is polled like `do_cancel` (renderer.rs:25-30) before every callback and
 * while the call waits for the GPU: once it is non-zero the waves in flight
 * stop at their next work item, the call returns RT_OK and emits nothing
 * further; tiles delivered before stay delivered (cpu.rs:55-62).  Passing a
 * flag costs nothing while it stays zero.  If it is already set on entry the
 * call returns RT_ERR_CANCEL_EVENT (cpu.rs:82-85).
 * params->strip_count > 1 is refused (RT_ERR_INVALID_ARGUMENT): tiles are finished pieces of the
 * frame.  rt_scene_last_stats after this call: kernel_ms spans the launch. */
int rt_render(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
              RtTileCallback callback, void *user, const volatile int *cancel);

/* rt_render with the cancel hook as a FUNCTION (NULL = never cancelled): the form a
 * binding of the reference uses, whose cancel event is an object, not an int in memory. */
int rt_render_ex(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                 RtTileCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user);

/* One whole-frame BufferUpdate per pass (renderer/denoised.rs:210-216, renderer/image.rs:56-62):
 * rgb = width*height*3 f64, row-major, sqrt(sum / samples_done), not tone-mapped; valid during the call only. */
typedef void (*RtFrameCallback)(void *user, const double *rgb, int32_t samples_done, int32_t samples_total);

/* The whole frame, converging: rendered in passes (renderer/denoised.rs:291-331) with one callback per pass on the
 * calling thread, the last of them carrying the frame of rt_render_frame.
 *  - params->samples (N) is the total.  The frame's samples are summed chunk by chunk in a chunk order that depends on N
 *    only; a pass runs from the current chunk boundary to the first boundary at least pass_samples further on, or to N.
 *    samples_done is always a chunk boundary; pass_samples >= N means one pass.  For N = 96 the boundaries are
 *    0, 24, 48, 72, 84, 92, 96, so pass_samples = 1 delivers at 24, 48, 72, 84, 92, 96; pass_samples = 30 at 48, 84, 96;
 *    pass_samples = 96 at 96.  samples_total is N in every callback.
 *  - The last callback's frame is bit-identical to rt_render_frame's for the same inputs.  The frame after s samples
 *    agrees with an s-spp render to the same tolerance as any two summation orders (the draws are the same).
 *  - Fixed-point sums (RtArithmetic) use the exponent of N, so the result is exact at N; a render that rt_render_frame
 *    refuses at N is refused here too.
 *  - `cancelled` (may be NULL) behaves as in rt_render_ex: raised on entry, the call returns RT_ERR_CANCEL_EVENT with no
 *    callback; raised later, the waves in flight stop at their next work item and the call returns RT_OK with no further
 *    callback.  Frames already delivered stay delivered.
 *  - Refused before anything is enqueued: RT_ERR_INVALID_ARGUMENT for params->strip_count > 1, params->scale > 1,
 *    pass_samples <= 0 or a NULL callback; RT_ERR_UNSUPPORTED for a scene on the v1 kernel (RT_KERNEL_V1).
 *  - rt_scene_last_stats afterwards describes the whole call: samples = W*H*N and segments as rt_render_frame's for the
 *    same inputs, kernel_ms summed over the passes' launches, resolve_ms over their fold passes, kernel_launches = passes.
 *  - The GPU works one pass ahead of the callback.  The callback must not call into the library with the same scene.
 * A binding detects this entry point by symbol lookup (RT_ABI_VERSION is unchanged by it). */
int rt_render_progressive(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                          int32_t pass_samples, RtFrameCallback callback, void *user,
                          RtCancelCallback cancelled, void *cancel_user);

/* ------------------------------------------------------------------ denoising
 * The reference's ray_color returns the first hit's normal, position, depth and obj_id beside the colour (renderer.rs:
 * RayImageData) and renderer/denoised.rs filters the frame pass by pass with them.  These entry points do that on the
 * device: first-hit GUIDE buffers, then an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with object,
 * normal and plane edge stops and an optional colour stop, in f64 throughout (DESIGN.md section 4.6 has the definition).
 *
 * Guides: one ray per pixel, get_ray with the lens offset at zero, u = (x + 0.5) / (W - 1), v = (y + 0.5) / (H - 1)
 * (row 0 = top), time (time_a + time_b) / 2, no random draw; the closest hit over [0.001, inf) under the scene's own
 * closest-hit rule.  Planes (structure of arrays, W*H pixels, row-major): normal (3 f64, after set_face_normal),
 * position (3 f64), albedo (3 f64: the texture value clamped to [0, 1] for Lambertian and Metal, 1 for Dielectric and
 * DiffuseLight), footprint (1 f64: t * |camera.vertical| / (H - 1), the world-space size of a pixel at the hit) and
 * obj_id (1 int32: RtPrimitive.obj_id).  A miss has obj_id -1, normal = position = 0, albedo = 1, footprint = +inf. */
enum RtDenoiseFlags {
    RT_DENOISE_DEMODULATE = 1 /* filter radiance / max(albedo, 1e-3) and multiply the albedo back afterwards */
};
typedef struct RtDenoiseParams {
    int32_t iterations;  /* a-trous levels, 0..10 (0: the output is an exact copy of the input) */
    int32_t flags;       /* RtDenoiseFlags */
    double sigma_color;  /* colour stop on sqrt(radiance); <= 0 switches it off */
    double sigma_normal; /* normal stop; <= 0 switches it off */
    double sigma_plane;  /* plane-distance stop in pixel footprints; <= 0 switches it off */
    int32_t _reserved[4]; /* must be 0 */
} RtDenoiseParams;
typedef struct RtGuides {
    double *normal;    /* W*H*3 */
    double *position;  /* W*H*3 */
    double *albedo;    /* W*H*3 */
    double *footprint; /* W*H   */
    int32_t *obj_id;   /* W*H   */
} RtGuides;

/* The defaults: 5 iterations, demodulation on, colour stop off, sigma_normal and sigma_plane as DESIGN.md records. */
void rt_denoise_params_default(RtDenoiseParams *out);
/* The guides of a whole frame (params->strip_count <= 1, params->scale <= 1) into DEVICE memory of the scene's device,
 * enqueued on `hip_stream` (NULL = default stream) without synchronising. */
int rt_render_guides_device(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                            const RtGuides *guides_device, void *hip_stream);
/* Filter a gamma-encoded device frame (what rt_render_frame_device writes) with device guides of the same size into
 * out_device (rgb_device != out_device), enqueued on `hip_stream` without synchronising.  Scratch memory is the scene's. */
int rt_denoise_device(RtScene *scene, const RtRenderParams *params, const RtDenoiseParams *denoise,
                      const double *rgb_device, const RtGuides *guides_device, double *out_device, void *hip_stream);
/* Host-memory convenience, synchronous: guides, upload of rgb_host, filter, download into out_host (rgb != out). */
int rt_denoise_frame(RtScene *scene, const RtCamera *camera, const RtRenderParams *params, const RtDenoiseParams *denoise,
                     const double *rgb_host, double *out_host);
/* rt_render_progressive whose every callback receives the denoised frame of its pass.  The guides are traced once before
 * pass 0; each pass's filter runs after its fold, into a device slot of its own, so the running sums are untouched.  The
 * last callback's frame equals rt_denoise_frame applied to rt_render_frame's frame, bit for bit.  Pass boundaries,
 * cancel, refusals and statistics are rt_render_progressive's (resolve_ms includes the filter). */
int rt_render_progressive_denoised(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                                   int32_t pass_samples, const RtDenoiseParams *denoise, RtFrameCallback callback,
                                   void *user, RtCancelCallback cancelled, void *cancel_user);
/* The four that return a code refuse, as far as they take them, NULL pointers, iterations outside 0..10, non-finite
 * sigmas, non-zero _reserved, strips, scale > 1 and rgb == out (RT_ERR_INVALID_ARGUMENT) before they touch a device.  A binding detects them by symbol lookup (RT_ABI_VERSION is
 * unchanged by them). */

/* ---------------------------------------------------------------- temporal accumulation
 * The history the reference's renderer/denoised.rs plans ("Implement SVGF", `temporal()`): radiance carried from one
 * camera to the next by re-projecting the first hits, per-pixel luminance moments, and an a-trous filter whose luminance
 * stop is scaled by the local standard deviation (Schied et al. 2017).  DESIGN.md section 4.11 has the definition; all of
 * it is f64 in linear (demodulated) radiance.
 *  - A history is six planes over W*H pixels in DEVICE memory: radiance (3 f64, accumulated and UNFILTERED), moments
 *    (2 f64: the running means of the luminance and of its square), length (1 f64), and the normal (3 f64), position
 *    (3 f64) and obj_id (int32) of the frame that wrote it.  The camera of that frame is kept by the caller.
 *  - rt_temporal_accumulate_device blends a gamma-encoded frame (what rt_render_frame_device writes) into out_history:
 *    each hit pixel's position is re-projected through prev_camera, the four bilinear taps of prev_history that agree in
 *    obj_id, normal (|n - n'|^2 <= normal_tolerance^2) and plane (|n . (x' - x)| <= plane_tolerance * footprint) are
 *    blended with a = max(1 / (length + 1), alpha); a pixel without a valid tap, a miss, or prev_history == NULL starts
 *    afresh with length 1.  prev_camera and prev_history are both NULL or neither is; out_history must not alias
 *    prev_history.  denoise->flags decides the demodulation, as in rt_denoise_device.  Enqueued on `hip_stream` without
 *    synchronising.
 *  - rt_denoise_history_device filters a history's radiance into out_device (gamma-encoded): the per-pixel variance of the
 *    luminance (from the moments where length >= 4, else from a 7x7 neighbourhood), denoise->iterations a-trous levels with
 *    the extra stop exp(-|l_p - l_q| / (sigma_luminance * sqrt(var) + 1e-10)), and the re-modulation
 *    sqrt(max(radiance * albedo, 0)), which is all that iterations == 0 does.  With sigma_luminance <= 0 the levels are
 *    rt_denoise_device's own.  guides_device are the guides of the frame that wrote the history.  The history is not
 *    written: no filtered colour is ever fed back.  Scratch memory is the scene's.
 *  - RtTemporal keeps two histories, the guides and the last camera for a W x H stream of frames on one device.
 *    rt_render_temporal does, in order: rt_render_frame_device's frame for (camera, params), its guides, the accumulation
 *    against the stored history and camera, the filter, the download into out_rgb_host (and of the history's length into
 *    out_length_host, W*H f64, when not NULL), and the swap of the histories.  The caller advances params->seed from frame
 *    to frame: equal seeds trace equal samples, and accumulating those adds nothing.  rt_temporal_reset forgets the
 *    history (a moved object keeps its obj_id, so the caller resets).  Calls on one RtTemporal, and on the scene it
 *    renders, are serialised by the caller.
 *  - Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: NULL pointers, what rt_denoise_device refuses about
 *    params and denoise, non-finite temporal parameters, an alpha outside [0, 1], max_history < 1, a non-zero _reserved;
 *    for rt_render_temporal also a width, height or device that is not the RtTemporal's.  RT_ERR_UNSUPPORTED for
 *    rt_render_temporal on a scene of the v1 kernel, as rt_render_progressive_denoised.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
typedef struct RtTemporalParams {
    double alpha;            /* floor of the radiance blend factor, 0..1 (0: the running mean up to max_history) */
    double alpha_moments;    /* ... of the moments' */
    double max_history;      /* the history length stops growing here (>= 1) */
    double normal_tolerance; /* a tap is valid while |n - n'| <= this */
    double plane_tolerance;  /* ... and its distance from the pixel's tangent plane <= this many pixel footprints */
    double sigma_luminance;  /* luminance stop in standard deviations; <= 0 switches it off */
    int32_t _reserved[4];    /* must be 0 */
} RtTemporalParams;
typedef struct RtHistory {
    double *radiance;  /* W*H*3 */
    double *moments;   /* W*H*2 */
    double *length;    /* W*H   */
    double *normal;    /* W*H*3 */
    double *position;  /* W*H*3 */
    int32_t *obj_id;   /* W*H   */
} RtHistory;
typedef struct RtTemporal RtTemporal; /* opaque; owned by the library */

/* The defaults: alpha = alpha_moments = 0.2, max_history 32, the tolerances and sigma_luminance as DESIGN.md 4.11
 * records.  A NULL is ignored. */
void rt_temporal_params_default(RtTemporalParams *out);
int rt_temporal_accumulate_device(RtScene *scene, const RtRenderParams *params, const RtTemporalParams *temporal,
                                  const RtDenoiseParams *denoise, const double *rgb_device, const RtGuides *guides_device,
                                  const RtCamera *prev_camera, const RtHistory *prev_history, const RtHistory *out_history,
                                  void *hip_stream);
int rt_denoise_history_device(RtScene *scene, const RtRenderParams *params, const RtDenoiseParams *denoise,
                              const RtTemporalParams *temporal, const RtHistory *history, const RtGuides *guides_device,
                              double *out_device, void *hip_stream);
int rt_temporal_create(int device, int32_t width, int32_t height, RtTemporal **out);
void rt_temporal_destroy(RtTemporal *temporal_state);
int rt_temporal_reset(RtTemporal *temporal_state);
int rt_render_temporal(RtScene *scene, RtTemporal *temporal_state, const RtCamera *camera, const RtRenderParams *params,
                       const RtTemporalParams *temporal, const RtDenoiseParams *denoise, double *out_rgb_host,
                       double *out_length_host /* may be NULL */);

/* ---------------------------------------------------------------- adaptive sampling
 * rt_render_progressive's passes, with the 8x8 tiles that have converged left out of the passes after it (DESIGN.md
 * section 4.7).
 *  - Passes and decisions.  The passes are rt_render_progressive's for (N = params->samples, pass_samples).  After each
 *    pass every tile still running is evaluated; let s be its samples done and k its chunks done.  It is eligible when
 *    k >= 4 and s >= min_samples, and it stops when it is eligible and its error is <= threshold.  A stopped tile traces
 *    nothing further.  The call ends after the last pass, or as soon as no tile is running.
 *  - Error of a tile.  Per pixel and channel, from the tile's chunk sums S_j over n_j samples (j = 1..k, s = sum n_j):
 *    m = S / s with S = sum S_j; V = max(0, sum S_j^2 / n_j - S m) / (k - 1) (batch means); sigma = sqrt(V / s);
 *    e = sigma / (sqrt(m + sigma) + sqrt(m)) — which is sqrt(m + sigma) - sqrt(m), how far one standard error moves the
 *    gamma-encoded value — and e = 0 where sigma = 0 (a black or constant pixel; no floor constant).  The tile's error is
 *    the largest e over its pixels inside the image and their three channels.  out_tile_error holds each tile's error at
 *    its last pass, or -1 if that pass ended with fewer than 2 chunks.
 *  - Frame.  Every pixel equals, bit for bit, rt_render_progressive's frame after out_samples[p] samples (same scene,
 *    camera, params and pass_samples).  out_samples is constant over each 8x8 tile and always a pass boundary.  With
 *    threshold <= 0 the frame is rt_render_frame's, bit for bit, and every count is N.
 *  - Callback (may be NULL).  One after every pass that traced a tile: running tiles at the pass boundary, stopped tiles
 *    frozen at their own; samples_done is the pass boundary, samples_total N.  The last callback's frame equals out_rgb.
 *    The GPU runs the next pass during the callback, which must not call into the library with the same scene.
 *  - Cancel behaves as in rt_render_progressive: raised on entry, RT_ERR_CANCEL_EVENT with no callback; raised later,
 *    RT_OK with nothing further delivered, and out_* hold the state of the last callback (untouched when none came).
 *  - Refused with RT_ERR_INVALID_ARGUMENT before the scene is looked at: NULL adaptive or out_rgb, a non-finite threshold,
 *    pass_samples <= 0, min_samples < 0, a non-zero _reserved, params->strip_count > 1 or params->scale > 1.  A scene on
 *    the v1 kernel gets RT_ERR_UNSUPPORTED, and what rt_render_frame refuses at N is refused here too (the fixed-point
 *    sums take N's exponent, as in rt_render_progressive).
 *  - rt_scene_last_stats afterwards: samples is the device's own count (= the sum of out_samples), segments the device's
 *    count, kernel_ms and resolve_ms summed over the passes, kernel_launches = the passes run.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
typedef struct RtAdaptiveParams {
    double threshold;     /* a tile stops once its error is <= threshold; <= 0: no tile ever stops */
    int32_t pass_samples; /* decisions at the ends of rt_render_progressive's passes for this value (> 0) */
    int32_t min_samples;  /* no tile stops before this many samples (>= 0) */
    int32_t _reserved[4]; /* must be 0 */
} RtAdaptiveParams;

/* The defaults: threshold 0.01, pass_samples 64, min_samples 0.  A NULL is ignored. */
void rt_adaptive_params_default(RtAdaptiveParams *out);
int rt_render_adaptive(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                       const RtAdaptiveParams *adaptive,
                       double *out_rgb,        /* HOST, W*H*3 f64, required */
                       int32_t *out_samples,   /* HOST, W*H: the samples each pixel received; may be NULL */
                       double *out_tile_error, /* HOST, ceil(W/8)*ceil(H/8), row-major tiles; may be NULL */
                       RtFrameCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user);

/* ---------------------------------------------------------------- next-event estimation
 * A second estimator for whole frames: the plain path of rt_render_frame with one light sample
 * at every Lambertian vertex whose bounce ray is traced (segment + 1 < max_depth), both terms weighted by multiple
 * importance sampling.  Its mean is the plain frame's mean: every draw of the plain estimator keeps its address
 * (rt_rng.h), so a sample's bounce path is the path rt_render_frame traces; the light sample draws from RT_RNG_LIGHT.
 *  - Lights are listed at rt_scene_create, in table order, at most 64: an unwrapped Sphere of positive radius or an
 *    unwrapped XY / XZ / YZ rect of non-zero area whose material is DiffuseLight.  Every other emitter is found by bounce
 *    rays only, with weight 1.  Any subset of the emitters gives an unbiased frame, so max_lights caps the list and 0
 *    lists none: the plain estimator.
 *  - Sums are per pixel in f64, in sample order: the frame does not depend on tiles, scheduling or a radiance bound.
 *    The output is sqrt(sum / samples), not tone-mapped, as rt_render_frame's.
 *  - Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: NULL pointers, an unknown heuristic, max_lights
 *    outside 0..64, a non-zero _reserved, params->strip_count > 1 and params->scale > 1.
 *  - rt_scene_last_stats afterwards: samples, path segments (shadow rays are not counted) and kernel_ms of the call.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
enum RtMisHeuristic {
    RT_MIS_POWER = 0,  /* w = p^2 / (p^2 + q^2) */
    RT_MIS_BALANCE = 1 /* w = p / (p + q)       */
};
typedef struct RtLightSamplingParams {
    int32_t heuristic;    /* RtMisHeuristic */
    int32_t max_lights;   /* 0..64; 0 = no light listed: the plain estimator's frame */
    int32_t _reserved[6]; /* must be 0 */
} RtLightSamplingParams;
/* The defaults: RT_MIS_POWER, 64 lights.  A NULL is ignored. */
void rt_light_sampling_params_default(RtLightSamplingParams *out);
/* The scene's listed lights as indices into RtSceneDesc.primitives, in table order, before any max_lights cap: the first
 * min(capacity, count) into out_prims (may be NULL when capacity is 0), their number into *out_count. */
int rt_scene_lights(RtScene *scene, int32_t *out_prims, int32_t capacity, int32_t *out_count);
/* out_rgb: HOST memory, width*height*3 f64.  Synchronous. */
int rt_render_frame_nee(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                        const RtLightSamplingParams *light_sampling, double *out_rgb);
/* rgb_device: DEVICE memory of the scene's device, enqueued on `hip_stream` (NULL = default stream) without
 * synchronising, e.g. ahead of rt_denoise_device. */
int rt_render_frame_nee_device(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                               const RtLightSamplingParams *light_sampling, double *rgb_device, void *hip_stream);

/* ---------------------------------------------------------------- the light list of a scene
 * rt_scene_create lists what the paragraph above says and picks among the listed lights uniformly: moving spheres, boxes
 * and wrapped primitives are never listed.  rt_scene_set_lights widens that per scene ("the
 * extended list"); until it is called a scene behaves as described above, and calling it with the defaults restores that
 * list exactly.
 *  - Listing.  Primitives are listed in table order, at most 64.  A primitive is listed when its material is
 *    DiffuseLight and it is a Sphere with r > 0 or a rect of non-zero area (inside Translate / RotateY only with
 *    RT_LIGHTS_WRAPPED), a Box of positive surface area with RT_LIGHTS_BOXES (a wrapped one needs RT_LIGHTS_WRAPPED too),
 *    or a MovingSphere with r > 0 with RT_LIGHTS_MOVING.  rt_scene_lights reports the new list.
 *  - Pick.  RT_PICK_UNIFORM: light k = min(floor(e0 n), n - 1) with probability 1 / n, n = min(max_lights, count).
 *    RT_PICK_POWER: w_k = A_k L_k, A the object-frame surface area (rect |da db|, sphere 4 pi r^2, box 2 (ab + bc + ca)),
 *    L the largest colour component of a SolidColor emitter (a negative or non-finite one counts as 0), else 1;
 *    p_k = w_k / sum_{j<n} w_j, the running sums formed in f64 in table order with the last one set to 1, k the first
 *    index with e0 < cdf_k.  A sum that is not positive and finite gives the uniform pick.  A light with p_k = 0 is never
 *    sampled, and a bounce that hits it keeps weight 1.
 *  - Kernels.  A scene whose list holds a wrapped, box or moving light, or whose pick is RT_PICK_POWER, is rendered by
 *    the extended-light forms of the NEE kernels, which exist for the "anything" primitive class only: a rects-only or
 *    spheres-only scene that asks for RT_PICK_POWER goes through that class's linear loop, whose primitive kinds are a
 *    superset (same hits, same frame up to the arithmetic of another closest-hit loop).
 *  - rt_scene_set_lights waits for the scene's own stream, replaces the device tables and may be called any number of
 *    times; the caller serialises it with renders on that scene, as every call on one RtScene.  Every NEE entry point uses
 *    the new list from then on.  The several-scene NEE calls refuse scenes that do not all carry the same list params.
 *  - rt_scene_light_weights: the pick probabilities p_k of the whole (uncapped) list, the first min(capacity, count) into
 *    out_p (may be NULL when capacity is 0), their number into *out_count.
 *  - Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: NULLs, kinds outside 0..7, an unknown pick, a
 *    non-zero _reserved. */
enum RtLightKinds {
    RT_LIGHTS_PLAIN = 0,   /* what rt_scene_create lists */
    RT_LIGHTS_WRAPPED = 1, /* ... inside Translate and / or RotateY too */
    RT_LIGHTS_BOXES = 2,   /* Box emitters */
    RT_LIGHTS_MOVING = 4,  /* MovingSphere emitters */
    RT_LIGHTS_ALL = 7
};
enum RtLightPick {
    RT_PICK_UNIFORM = 0,
    RT_PICK_POWER = 1
};
typedef struct RtLightListParams {
    int32_t kinds;        /* RtLightKinds, or-ed */
    int32_t pick;         /* RtLightPick */
    int32_t _reserved[6]; /* must be 0 */
} RtLightListParams;
/* The defaults: RT_LIGHTS_PLAIN, RT_PICK_UNIFORM — what rt_scene_create lists.  A NULL is ignored. */
void rt_light_list_params_default(RtLightListParams *out);
int rt_scene_set_lights(RtScene *scene, const RtLightListParams *p);
int rt_scene_light_weights(RtScene *scene, double *out_p, int32_t capacity, int32_t *out_count);

/* ---------------------------------------------------------------- next-event estimation in passes
 * rt_render_progressive and rt_render_adaptive with the next-event estimator: whole frames while
 * they converge, a cancel hook and the adaptive stop rule for rt_render_frame_nee's frames.
 *  - Passes.  The pass boundaries are exactly rt_render_progressive's for (N = params->samples, pass_samples): the chunk
 *    plan of N, a pass running to the first chunk boundary at least pass_samples further on.
 *  - Frames.  The NEE kernel sums each pixel in f64 in sample order and every draw is addressed by (pixel, sample, ...), so
 *    nothing a sample contributes depends on N, and the passes carry each pixel's running sum from one launch to the next.
 *    Therefore the frame a callback receives with samples_done = s is bit-identical to rt_render_frame_nee with
 *    params->samples = s and everything else equal — for EVERY pass, not only the last (rt_render_progressive promises
 *    that for its last frame only).
 *  - Adaptive.  Tiles, eligibility (k >= 4 chunks, s >= min_samples), the error formula, out_samples, out_tile_error (-1
 *    with fewer than 2 chunks), the callback, the early end when no tile runs and the statistics are rt_render_adaptive's,
 *    with S_j the NEE chunk sums of the tile's pixels (S_j is formed as the difference of the pixel's running sum at the
 *    chunk's two boundaries).  Every pixel of out_rgb and of every callback frame equals, bit for bit, rt_render_frame_nee
 *    at samples = out_samples[p] (in a callback: min(out_samples[p], samples_done)).  With threshold <= 0 the frame is
 *    rt_render_frame_nee's at N and every count is N.
 *  - Cancel as in rt_render_progressive / rt_render_adaptive: raised on entry, RT_ERR_CANCEL_EVENT and no callback; raised
 *    later, RT_OK, nothing further delivered, and out_* hold the state of the last callback (untouched when none came).
 *    The waves read the cancel word when they start and at every chunk boundary inside a pass.  A render on the same scene
 *    afterwards sees nothing stale.
 *  - Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: everything rt_render_frame_nee refuses (NULL
 *    pointers, an unknown heuristic, max_lights outside 0..64, a non-zero _reserved, params->strip_count > 1,
 *    params->scale > 1); pass_samples <= 0 and a NULL callback for the progressive form; everything rt_render_adaptive
 *    refuses about `adaptive` and out_rgb for the adaptive form.  The NEE kernel is a kernel of its own, so a scene created
 *    with RT_KERNEL_V1 is NOT refused (unlike rt_render_progressive and rt_render_adaptive).
 *  - No radiance bound and no fixed-point sums, as rt_render_frame_nee: a scene that rt_render_frame refuses at N for its
 *    exponent renders here.
 *  - max_lights = 0, or a scene without a listed light: the plain estimator in passes.
 *  - rt_scene_last_stats afterwards: samples is the device's own count (W*H*N progressive, the sum of out_samples adaptive),
 *    segments counts path segments only (shadow rays are not counted; progressive: exactly rt_render_frame_nee's count at
 *    N), kernel_ms and resolve_ms are summed over the passes, kernel_launches = the passes run.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
int rt_render_progressive_nee(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                              const RtLightSamplingParams *light_sampling, int32_t pass_samples,
                              RtFrameCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user);
int rt_render_adaptive_nee(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                           const RtLightSamplingParams *light_sampling, const RtAdaptiveParams *adaptive,
                           double *out_rgb,        /* HOST, W*H*3 f64, required */
                           int32_t *out_samples,   /* HOST, W*H: the samples each pixel received; may be NULL */
                           double *out_tile_error, /* HOST, ceil(W/8)*ceil(H/8), row-major tiles; may be NULL */
                           RtFrameCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user);

/* ---------------------------------------------------------------- variance-guided filter of an adaptive frame
 * rt_denoise_history_device's variance-guided levels for a STILL frame, the variance taken from the batch sums the adaptive
 * renderer keeps anyway (tests/variance_filter_model.py restates it).  After rt_render_adaptive or
 * rt_render_adaptive_nee a pixel of a tile with s samples and k chunks done has, per channel, the running sum S and
 * Q = sum_j S_j^2 / n_j (the adaptive paragraph above).  With a = max(albedo, 1e-3) under RT_DENOISE_DEMODULATE, else 1:
 *    m = S / s;  sigma = sqrt(max(0, Q - S m) / (k - 1) / s);  C = m / a;  sigma' = sigma / a;
 *    var = (0.2126 sigma'_r + 0.7152 sigma'_g + 0.0722 sigma'_b)^2          where k >= min_chunks
 * — the squared standard error of the luminance with the channels taken as fully correlated, an upper bound.  A guide miss
 * has var = 0.  Where k < min_chunks var is rt_denoise_history_device's 7x7 spatial estimate over C.  The filter is
 * denoise->iterations levels of that call's a-trous level over (C, var) with filter->sigma_luminance, then
 * sqrt(max(C albedo, 0)), which is all that iterations == 0 does; with sigma_luminance <= 0 the levels are
 * rt_denoise_device's.
 *  - rt_batch_variance_device: C into radiance_out_device (W*H*3 f64) and var into variance_out_device (W*H f64) from the
 *    planes of batch_planes (samples and chunks are per PIXEL, samples >= 1) and the guides' albedo, normal, position,
 *    footprint and obj_id.  Enqueued on `hip_stream` without synchronising.
 *  - rt_denoise_variance_device: the levels and the re-modulation of (radiance_device, variance_device) into out_device
 *    (gamma-encoded; out_device != radiance_device).  Neither input is written.  Scratch memory is the scene's.  Enqueued on
 *    `hip_stream` without synchronising.
 *  - rt_render_adaptive_filtered does, in order: rt_render_adaptive (light_sampling == NULL) or rt_render_adaptive_nee —
 *    the same passes, callbacks (unfiltered frames), cancel and refusals —, the guides of (camera, params), the two calls
 *    above on the scene's own sums, squares and tile state, and the download of the filtered frame into out_rgb.
 *    outputs->raw_rgb, samples and tile_error equal the adaptive call's out_rgb, out_samples and out_tile_error bit for bit;
 *    with adaptive->threshold <= 0 raw_rgb is rt_render_frame's frame (rt_render_frame_nee's): the still-frame case.
 *    outputs->sums and squares are S and Q, chunks the k of every pixel's tile, variance the var fed to the levels.  On a
 *    cancel nothing is filtered: the call returns what the adaptive call returns, out_rgb holds the last unfiltered frame as
 *    that call leaves it, and of `outputs` only samples and tile_error are written.
 *  - Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: NULL pointers (the fields of RtBatchOutputs aside),
 *    what rt_denoise_device refuses about params and denoise, a non-finite sigma_luminance, min_chunks < 2, a non-zero
 *    _reserved, out_device == radiance_device; for rt_render_adaptive_filtered everything the adaptive call it runs refuses.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
typedef struct RtVarianceFilterParams {
    double sigma_luminance; /* luminance stop in standard errors; <= 0: rt_denoise_device's levels */
    int32_t min_chunks;     /* the batch estimate is used from this many chunks on (>= 2) */
    int32_t _reserved[5];   /* must be 0 */
} RtVarianceFilterParams;
typedef struct RtBatchPlanes { /* DEVICE memory */
    const double *sums;     /* W*H*3: S */
    const double *squares;  /* W*H*3: Q */
    const int32_t *samples; /* W*H: s */
    const int32_t *chunks;  /* W*H: k */
} RtBatchPlanes;
typedef struct RtBatchOutputs { /* HOST memory; each field may be NULL */
    double *raw_rgb;     /* W*H*3 */
    double *sums;        /* W*H*3 */
    double *squares;     /* W*H*3 */
    int32_t *samples;    /* W*H */
    int32_t *chunks;     /* W*H */
    double *tile_error;  /* ceil(W/8)*ceil(H/8), as rt_render_adaptive's */
    double *variance;    /* W*H */
} RtBatchOutputs;

/* The defaults: sigma_luminance 4, min_chunks 4.  A NULL is ignored. */
void rt_variance_filter_params_default(RtVarianceFilterParams *out);
int rt_batch_variance_device(RtScene *scene, const RtRenderParams *params, const RtDenoiseParams *denoise,
                             const RtVarianceFilterParams *filter, const RtBatchPlanes *batch_planes,
                             const RtGuides *guides_device, double *radiance_out_device, double *variance_out_device,
                             void *hip_stream);
int rt_denoise_variance_device(RtScene *scene, const RtRenderParams *params, const RtDenoiseParams *denoise,
                               const RtVarianceFilterParams *filter, const double *radiance_device,
                               const double *variance_device, const RtGuides *guides_device, double *out_device,
                               void *hip_stream);
int rt_render_adaptive_filtered(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                                const RtLightSamplingParams *light_sampling /* NULL: the plain estimator */,
                                const RtAdaptiveParams *adaptive, const RtDenoiseParams *denoise,
                                const RtVarianceFilterParams *filter,
                                double *out_rgb /* HOST, W*H*3 f64, filtered, required */,
                                RtBatchOutputs *outputs /* may be NULL */,
                                RtFrameCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user);

/* rt_render_ex's contract with rt_render_frame_nee's estimator: the tile stream of ONE next-event-estimation frame, delivered
 * while it renders, with a cancel hook that stops it quickly.  One device (several: rt_render_nee_multi below); no `volatile int` form.
 *  - Tiles: the tiles_w x tiles_h grid, column-major, the last row / column absorbing the remainders, ONE callback per tile
 *    (an empty tile included), on the calling thread, while the launch is still running.  For the same `params` the sequence
 *    of (r, c, width, height) is exactly rt_render_ex's.
 *  - Pixels: every delivered pixel equals rt_render_frame_nee's pixel for the same scene, camera, params and
 *    light_sampling, bit for bit: a pixel's samples are added in sample order to an f64 sum that starts at +0.0, and the
 *    value written is sqrt((1 / samples) * sum) with the same reciprocal.  The tile grid changes no pixel.
 *  - One persistent launch traces 8x8 pixel tiles, queued tile column by tile column, and writes finished pixels straight
 *    into pinned host memory; no resolve launch.  Where that launch does not apply (a tile grid wider than the image) the
 *    frame is rt_render_frame_nee's launch and the tiles are cut from it: same pixels, same sequence.
 *  - cancelled / cancel_user as rt_render_ex's (polled on the calling thread; NULL: none).  Raised on entry:
 *    RT_ERR_CANCEL_EVENT, no callback.  Raised later: RT_OK, nothing further is delivered, tiles already delivered stay
 *    delivered.  On the device a wave reads the cancel word at every hand-out of a tile and between the sample chunks of
 *    its tile, so a cancel does not wait for a tile's full sample count.  A later render on the same scene, through any
 *    entry point, sees nothing stale.
 *  - Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: everything rt_render_frame_nee refuses (NULL scene,
 *    camera, params or light_sampling, an unknown heuristic, max_lights outside 0..64, a non-zero _reserved,
 *    params->strip_count > 1, params->scale > 1) and a NULL callback.  A scene created with RT_KERNEL_V1 is NOT refused
 *    (the NEE kernels are their own).  max_lights = 0, or a scene without a listed light: the plain estimator's paths.
 *  - rt_scene_last_stats afterwards: samples = W*H*N, segments exactly rt_render_frame_nee's count for the same inputs,
 *    kernel_ms spans the launch, kernel_launches = 1.
 * A binding detects this entry point by symbol lookup (RT_ABI_VERSION is unchanged by it). */
int rt_render_nee(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                  const RtLightSamplingParams *light_sampling,
                  RtTileCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user);

/* ---------------------------------------------------------------- next-event estimation on several devices
 * rt_render_frame_multi, rt_render_frame_multi_device and rt_render_multi with rt_render_frame_nee's estimator, and the
 * strip-owning form of rt_render_frame_nee_device that a multi-process gather would call.
 *  - Shares as in rt_render_frame_multi: scenes[i] are distinct RtScene objects of the SAME description, one per share (a
 *    device may carry several); the frame is cut into strips of strip_rows rows (0 = 8) and strip j belongs to
 *    scenes[j % n_scenes].  Every share traces its strips on its own stream at the same time.
 *  - Pixels: every pixel delivered or written equals rt_render_frame_nee's pixel for the same scene, camera, params and
 *    light_sampling, BIT FOR BIT, for every n_scenes >= 1 and every strip_rows >= 1, strips that cut 8x8 tiles included:
 *    a pixel's samples are added in sample order to an f64 sum of its own and every draw is addressed by the pixel's index
 *    in the whole image, so nothing depends on which share traces it or on how the rows are cut.  (The plain several-
 *    device calls promise this for strip heights that are multiples of 8 only.)  The value is sqrt((1 / samples) * sum).
 *  - rt_render_frame_nee_strips_device: rt_render_frame_nee_device honouring params->strip_*: the rows the share owns are
 *    rendered and written, every other row of rgb_device is left alone.  With strip_count <= 1 it IS
 *    rt_render_frame_nee_device; with strip_count > 1 the strip values are held to what rt_render_frame_device asks
 *    (strip_rows > 0, 0 <= strip_index < strip_count).  Enqueued on `hip_stream`, not synchronised.
 *  - rt_render_frame_nee_multi: out_rgb is HOST memory; every share writes its finished pixels into one pinned frame, which
 *    the call copies to out_rgb band by band.  rt_render_frame_nee_multi_device: out_rgb_device is memory of scenes[0]'s
 *    device, the strips are gathered as rt_render_frame_multi_device gathers them; synchronises before returning.
 *  - rt_render_nee_multi: rt_render_nee's contract over the shares.  The sequence of (r, c, width, height) is rt_render_nee's
 *    (and so rt_render_ex's); a tile column goes out once EVERY share has published it.  Cancel as in rt_render_multi and
 *    rt_render_nee: raised on entry, RT_ERR_CANCEL_EVENT and no callback; raised later, RT_OK, nothing further is delivered,
 *    every share's launch is ended, and a later render on any of the scenes sees nothing stale.  Where the delivering
 *    launch does not apply (a tile grid wider than the image) n_scenes == 1 falls back as rt_render_nee does and
 *    n_scenes > 1 returns RT_ERR_UNSUPPORTED, as rt_render_multi does for its non-delivering routes.
 *  - A share that owns no rows (more shares than strips; a strip_index whose first strip lies below the image) launches
 *    nothing and the call succeeds; rt_render_frame_nee_strips_device then writes nothing.
 *  - Refused with RT_ERR_INVALID_ARGUMENT before any device is touched: everything rt_render_frame_nee refuses about camera,
 *    params and light_sampling (NULLs, an unknown heuristic, max_lights outside 0..64, a non-zero _reserved,
 *    params->scale > 1); for the three several-scene forms a NULL or repeated scene, n_scenes <= 0, params->strip_count > 1
 *    (the call deals the strips) and a negative strip_rows; a NULL output or callback.  A scene created with RT_KERNEL_V1
 *    is NOT refused (the NEE kernels are their own).
 *  - rt_scene_last_stats(scenes[i]) afterwards gives share i's own counts: the samples add up to W*H*N, the segments to
 *    EXACTLY rt_render_frame_nee's count (a pixel's paths do not depend on its share), kernel_launches is 1 for a share
 *    that launched and 0 for one that owned nothing.
 * Nothing here has run on more than one physical device yet.  A binding detects these entry points by
 * symbol lookup (RT_ABI_VERSION is unchanged by them). */
int rt_render_frame_nee_strips_device(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                                      const RtLightSamplingParams *light_sampling, double *rgb_device, void *hip_stream);
int rt_render_frame_nee_multi(RtScene *const *scenes, int n_scenes, const RtCamera *camera, const RtRenderParams *params,
                              const RtLightSamplingParams *light_sampling, int strip_rows, double *out_rgb /* HOST */);
int rt_render_frame_nee_multi_device(RtScene *const *scenes, int n_scenes, const RtCamera *camera, const RtRenderParams *params,
                                     const RtLightSamplingParams *light_sampling, int strip_rows, double *out_rgb_device);
int rt_render_nee_multi(RtScene *const *scenes, int n_scenes, const RtCamera *camera, const RtRenderParams *params,
                        const RtLightSamplingParams *light_sampling, int strip_rows,
                        RtTileCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user);

/* What the reference does to a finished tile downstream of the renderer, on
 * the device: ScreenBuffer::update's tone map (image_buffer.rs:147-153) and
 * SavePng's packing `(c * 255.0) as u32 -> (r << 24 | g << 16 | b << 8 | 255)`
 * as big-endian bytes (image_action/png.rs:21-31), fused in one pass over a
 * frame produced by rt_render_frame_device.  rgb_device: n_pixels*3 f64;
 * rgba_device: n_pixels*4 bytes; mapped_device: n_pixels*3 f64 receiving the
 * tone-mapped floats, or NULL.  Enqueued on `hip_stream`, no synchronisation.
 * Arithmetic is unfused IEEE f64, so the bytes equal rth_tone_map +
 * rth_pack_rgba8 on the host. */
int rt_post_rgba8_device(RtScene *scene, const RtToneMap *tone_map, const double *rgb_device,
                         size_t n_pixels, uint8_t *rgba_device, double *mapped_device, void *hip_stream);

/* rt_render_frame + rt_post_rgba8_device + copy: out_rgba is HOST memory,
 * width*height*4 bytes (what SavePng hashes and encodes).  Whole frames only
 * (params->strip_count > 1 is refused): with several GPUs gather the strips of
 * rt_render_frame_device first and pack on the gathering rank with rt_post_rgba8_device. */
int rt_render_frame_rgba8(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                          const RtToneMap *tone_map, uint8_t *out_rgba);

/* ---------------------------------------------------------- several devices
 * The reference shards one frame over its rayon pool by tile inside ONE call
 * (renderer/cpu.rs:118-131); these do the same over the GPUs of one process.
 * scenes[i] are RtScene objects of the SAME description created on the devices
 * that should take part (a device may appear twice: two scenes on it share it).
 * The frame is cut into strips of `strip_rows` rows (0 = 8), strip j belongs to
 * scenes[j % n_scenes]; every device traces its strips concurrently on its own
 * stream and the finished pixels are collected
 *   - rt_render_frame_multi:        in out_rgb (HOST memory): every device writes
 *     its finished pixels over its own PCIe link into one pinned frame, which the
 *     call copies to out_rgb band by band while the devices render on;
 *   - rt_render_frame_multi_device: in out_rgb_device, memory of scenes[0]'s
 *     device, by peer copies over xGMI (one strided copy per device on the
 *     SOURCE device's stream behind its resolve pass; a single process needs no
 *     RCCL rendezvous for that — the multi-PROCESS path gathers with RCCL,
 *     racer-tracer_amd/strips.py).  Synchronises before returning;
 *   - rt_render_multi:              as rt_render_ex's tile stream: a tile column
 *     is handed to the callback as soon as EVERY device has finished its strips
 *     of it (same order, same tiles, same cancel behaviour as rt_render_ex), so
 *     a several-GPU `impl Renderer` keeps progressive delivery and cancel.
 * params->strip_* must be unset (the call sets them per device) and
 * params->scale <= 1.  The frame is bit-identical to rt_render_frame's for
 * every n_scenes when strip_rows is a multiple of 8 (the RNG is addressed by the
 * global pixel index and strips are then whole 8-row item tiles); other strip
 * heights regroup the pixels that share a tile's sums and agree to rounding.
 * rt_scene_last_stats(scenes[i]) afterwards gives device i's share. */
int rt_render_frame_multi(RtScene *const *scenes, int n_scenes, const RtCamera *camera,
                          const RtRenderParams *params, int strip_rows, double *out_rgb);
int rt_render_frame_multi_device(RtScene *const *scenes, int n_scenes, const RtCamera *camera,
                                 const RtRenderParams *params, int strip_rows, double *out_rgb_device);
int rt_render_multi(RtScene *const *scenes, int n_scenes, const RtCamera *camera, const RtRenderParams *params,
                    int strip_rows, RtTileCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user);

/* Stats of the most recent render call on this scene (synchronises the
 * stream of that call first). */
int rt_scene_last_stats(RtScene *scene, RtRenderStats *out);

/* Static description of an error code; never NULL. */
const char *rt_strerror(int code);
/* Thread-local detail of the last failure in this library ("" if none). */
const char *rt_last_error_message(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_ABI_H */
