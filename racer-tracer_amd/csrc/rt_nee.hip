// rt_nee.hip — next-event estimation: the upload of the scene's light list (rt_plan.cpp: light_tables) and
// the entry points rt_render_frame_nee, rt_render_frame_nee_device, rt_render_frame_nee_strips_device, rt_scene_lights and
// rt_light_sampling_params_default (include/rt_abi.h); the several-device forms live in rt_deliver.hip and rt_multi.hip.  The kernel is rt_nee_kernel.hip's k_nee_f64, compiled in both arithmetic flavours; a scene uses its
// own (RtScene.kernels).  rt_scene_set_lights, rt_scene_light_weights and rt_light_list_params_default list a scene's lights
// again (rt_plan.cpp: list_lights, light_pick); a scene whose list holds a wrapped, box or moving light, or picks by power,
// launches the k_nee_lights_* kernels (rt_nee_lights_kernel.hip and its two siblings) in place of the three above.
#include "rt_scene.h"

#include <algorithm>
#include <cstring>
#include <string>

using rtapi::fail;
using rtapi::kMaxLights;

// What every NEE entry point refuses about camera, params and light sampling, short of check_params
int rtapi::check_nee_args(const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls, const char *what, bool strips) {
    if (!camera || !p || !ls) return fail(RT_ERR_INVALID_ARGUMENT, "camera/params/light_sampling is NULL");
    if (ls->heuristic != RT_MIS_POWER && ls->heuristic != RT_MIS_BALANCE)
        return fail(RT_ERR_INVALID_ARGUMENT, "light_sampling->heuristic is not an RtMisHeuristic");
    if (ls->max_lights < 0 || ls->max_lights > kMaxLights)
        return fail(RT_ERR_INVALID_ARGUMENT, "light_sampling->max_lights must be in 0..64");
    for (int32_t r : ls->_reserved)
        if (r != 0) return fail(RT_ERR_INVALID_ARGUMENT, "light_sampling->_reserved must be 0");
    if (p->strip_count > 1 && !strips) return fail(RT_ERR_INVALID_ARGUMENT, std::string(what) + " renders whole frames: params->strip_* is not supported");
    if (p->scale > 1) return fail(RT_ERR_INVALID_ARGUMENT, std::string(what) + " renders full-resolution frames: params->scale must be 0 or 1");
    return RT_OK;
}

// Everything that is refused before a device is touched; the scene last, so that each refusal names its own cause
int rtapi::check_nee(const RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                     const char *what, bool strips) {
    const int rc = check_nee_args(camera, p, ls, what, strips);
    if (rc != RT_OK) return rc;
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    return rtapi::check_params(camera, p);
}

namespace {
using rtapi::check_nee;

// The argument blocks of a k_nee_f64 / k_nee_pass_f64 / k_nee_stream_f64 launch over all samples of the rows `p` owns (the
// whole frame without strips; rt_plan.cpp: fill_grid sets strip_* and owned_rows)
int fill_nee_args(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls, rtdev::TraceArgs &a,
                  rtdev::NeeArgs &nee, rtdev::NeeLightArgs &lx) {
    // the render's own argument block (tables, tree, camera, grid); its fixed-point sums are the pooled kernel's, and this
    // kernel sums in f64, so they are sized for one sample (which no bound refuses) and not read
    RtRenderParams one = *p;
    one.samples = 1;
    const int rc = rtapi::fill_trace_args(s, camera, &one, a);
    if (rc != RT_OK) return rc;
    a.samples = p->samples;
    a.sample_begin = 0;
    a.sample_end = p->samples;
    if (!s->use_bvh) a.n_bvh_nodes = 0;
    nee.slot = s->nee_slot.ptr;
    nee.prim = s->nee_prim.ptr;
    nee.n_lights = std::min(ls->max_lights, (int32_t)s->lights.size());
    nee.heuristic = ls->heuristic;
    nee.inv_samples = 1.0 / (double)p->samples; // what rtdev_launch_resolve forms
    // the pick of this cap (read by the extended-light kernels only): row n_lights - 1 of the scene's table
    lx.p = lx.cdf = nullptr;
    lx.pick = RT_PICK_UNIFORM;
    lx._pad = 0;
    if (s->lights_extended && nee.n_lights > 0 && !s->pick_uniform[(size_t)nee.n_lights - 1]) {
        const size_t count = s->lights.size();
        lx.p = s->nee_pick.ptr + (size_t)(nee.n_lights - 1) * 2 * count;
        lx.cdf = lx.p + count;
        lx.pick = RT_PICK_POWER;
    }
    return RT_OK;
}

// What precedes the first launch of a call on `stream`: the statistics slots cleared, the item counter of a persistent
// grid (`clear_queue`) cleared, then ev_begin — behind the clearing of the counter: poison_queue waits for it
int open_launches(RtScene *s, hipStream_t stream, bool clear_queue = false) {
    rtapi::RenderBuffers &b = s->buf;
    RT_HIP(hipMemsetAsync(b.segments.ptr, 0, rtdev::RT_STAT_SLOTS * sizeof(unsigned long long), stream));
    if (clear_queue) RT_HIP(hipMemsetAsync(b.queue.ptr, 0, sizeof(unsigned int) * b.queue.count, stream));
    RT_HIP(hipEventRecord(b.ev_begin, stream));
    return RT_OK;
}

} // namespace

// A share that owns no rows launches nothing: its statistics are those of an empty call (no sample, no segment, no launch)
int rtapi::note_idle_share(RtScene *s, hipStream_t stream) {
    RT_HIP(hipSetDevice(s->device));
    const int rc = open_launches(s, stream);
    if (rc != RT_OK) return rc;
    RT_HIP(hipEventRecord(s->buf.ev_traced, stream));
    RT_HIP(hipEventRecord(s->buf.ev_resolved, stream));
    rtapi::note_launches(s, 0);
    return RT_OK;
}

// What the NEE launches of these parameters need in device memory, allocated now (a call over several shares: before its
// first launch, rt_api.hip: reserve_render_buffers says why): the full-frame accumulator of k_nee_f64, or the item counter
// and the delivery counters of k_nee_stream_f64
int rtapi::reserve_nee_buffers(RtScene *s, const RtRenderParams *p, bool delivering) {
    RT_HIP(hipSetDevice(s->device));
    rtapi::RenderBuffers &b = s->buf;
    if (!delivering) {
        const size_t n = (size_t)p->width * (size_t)p->height * 3;
        RT_HIP(b.accum.reserve(n));
        return RT_OK;
    }
    RT_HIP(b.queue.reserve(1));
    return rtapi::reserve_delivery_counters(s, rtapi::tile_count(p->width, rtapi::owned_rows_of(p)));
}

// One launch of k_nee_f64 over the rows `p` owns into the scene's accumulator (a full-frame [height][width][3] buffer, owned
// rows written), then the resolve pass of those rows into out_device
int rtapi::enqueue_nee(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls, double *out_device,
                       hipStream_t stream) {
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    rtdev::NeeArgs nee;
    rtdev::NeeLightArgs lx;
    int rc = fill_nee_args(s, camera, p, ls, a, nee, lx);
    if (rc != RT_OK) return rc;
    if (a.owned_rows <= 0) return note_idle_share(s, stream); // a strip_index whose first strip lies below the image
    if ((rc = reserve_nee_buffers(s, p, false)) != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    a.accum = b.accum.ptr;
    if ((rc = open_launches(s, stream)) != RT_OK) return rc;
    if (s->lights_extended) RT_HIP(s->kernels->nee_lights(&a, &nee, &lx, s->textured, s->specular, s->use_bvh, stream));
    else RT_HIP(s->kernels->nee(&a, &nee, s->prims_class, s->textured, s->specular, s->use_bvh, stream));
    RT_HIP(hipEventRecord(b.ev_traced, stream));
    RT_HIP(s->kernels->resolve(b.accum.ptr, out_device, p->width, p->height, a.strip_rows, a.strip_count, a.strip_index, p->samples, stream));
    RT_HIP(hipEventRecord(b.ev_resolved, stream));
    rtapi::note_launches(s, 1);
    return RT_OK;
}

namespace {
using rtapi::enqueue_nee;

int render_frame_nee(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls, double *out) {
    int rc = check_nee(s, camera, p, ls);
    if (rc != RT_OK) return rc;
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgb is NULL");
    return rtapi::nee_frame_to_host(s, camera, p, ls, out);
}

int render_frame_nee_device(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                            double *out, void *stream) {
    int rc = check_nee(s, camera, p, ls);
    if (rc != RT_OK) return rc;
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_device is NULL");
    return enqueue_nee(s, camera, p, ls, out, (hipStream_t)stream);
}

// ... honouring params->strip_* (the strip values checked as rt_render_frame_device checks them: rt_plan.cpp: check_params)
int render_frame_nee_strips_device(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                                   double *out, void *stream) {
    int rc = check_nee(s, camera, p, ls, "rt_render_frame_nee_strips_device", /*strips=*/true);
    if (rc != RT_OK) return rc;
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_device is NULL");
    return enqueue_nee(s, camera, p, ls, out, (hipStream_t)stream);
}

int scene_lights(const RtScene *s, int32_t *out, int32_t capacity, int32_t *count) {
    if (!s || !count) return fail(RT_ERR_INVALID_ARGUMENT, "scene/out_count is NULL");
    if (capacity < 0 || (capacity > 0 && !out)) return fail(RT_ERR_INVALID_ARGUMENT, "out_prims is NULL or capacity is negative");
    *count = (int32_t)s->lights.size();
    for (int32_t k = 0; k < capacity && k < *count; ++k) out[k] = s->lights[(size_t)k];
    return RT_OK;
}

} // namespace

// rt_render_nee's delivering launch: k_nee_stream_f64 as one persistent grid over the delivery's regions, ONE item per tile
// of the width x owned_rows grid (a share's strips; the whole frame without)
int rtapi::enqueue_nee_stream(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                              const Delivery &delivery) {
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    rtdev::NeeArgs nee;
    rtdev::NeeLightArgs lx;
    int rc = fill_nee_args(s, camera, p, ls, a, nee, lx);
    if (rc != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    hipStream_t stream = b.stream;
    rtapi::set_tile_grid(a, p->width, a.owned_rows); // the tiles k_nee_stream_f64 draws its work from: region rows are owned rows
    a.n_items = (uint32_t)a.n_tiles;
    a.total_chunks = a.n_chunks = 1;
    // (allocations, here and in setup_delivery, may follow earlier work of the stream; nothing of THIS share is in flight
    // before the launch below, and a call over several shares has reserved all of it before its first launch)
    if ((rc = reserve_nee_buffers(s, p, true)) != RT_OK) return rc;
    if ((rc = rtapi::setup_delivery(s, a, delivery, 1, stream)) != RT_OK) return rc;
    a.queue = b.queue.ptr;
    if (delivery.cancellable) rtapi::arm_cancel_word(s, a); // the waves read it at every hand-out and chunk boundary
    const int per_cu = s->lights_extended ? s->kernels->nee_lights_stream_blocks_per_cu(s->textured, s->specular, s->use_bvh)
                                          : s->kernels->nee_stream_blocks_per_cu(s->prims_class, s->textured, s->specular, s->use_bvh);
    const unsigned resident = rtapi::cap_blocks(s, (unsigned)(s->num_cus > 0 ? s->num_cus : 1) * (unsigned)per_cu);
    const unsigned blocks = std::min(resident, (a.n_items + 3u) / 4u);
    rtapi::note_grid(s, blocks, a.n_items);
    if ((rc = open_launches(s, stream, /*clear_queue=*/true)) != RT_OK) return rc;
    if (s->lights_extended) RT_HIP(s->kernels->nee_lights_stream(&a, &nee, &lx, s->textured, s->specular, s->use_bvh, blocks, stream));
    else RT_HIP(s->kernels->nee_stream(&a, &nee, s->prims_class, s->textured, s->specular, s->use_bvh, blocks, stream));
    RT_HIP(hipEventRecord(b.ev_traced, stream));
    RT_HIP(hipEventRecord(b.ev_resolved, stream)); // no resolve launch: the waves finish their own pixels
    rtapi::note_launches(s, 1);
    return RT_OK;
}

int rtapi::nee_frame_to_host(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls, double *out) {
    RT_HIP(hipSetDevice(s->device));
    rtapi::RenderBuffers &b = s->buf;
    const size_t n = (size_t)p->width * (size_t)p->height * 3;
    RT_HIP(b.frame.reserve(n));
    const int rc = enqueue_nee(s, camera, p, ls, b.frame.ptr, b.stream);
    if (rc != RT_OK) return rc;
    RT_HIP(hipStreamSynchronize(b.stream));
    RT_HIP(hipMemcpy(out, b.frame.ptr, n * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rtapi::begin_nee_passes(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                            hipStream_t stream, bool cancellable, NeePasses &np) {
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs &a = np.args;
    int rc = fill_nee_args(s, camera, p, ls, a, np.nee, np.lights);
    if (rc != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    const size_t n = (size_t)p->width * (size_t)p->height * 3;
    if (b.accum.count < n || b.squares.count < n || b.partial.count < n) return fail(RT_ERR_INVALID_ARGUMENT, "begin_nee_passes: the running sums are not reserved");
    a.accum = b.accum.ptr;
    np.starts = rtapi::chunk_plan(p->samples);
    rtapi::set_chunk_table(a, np.starts);
    rtapi::set_tile_grid(a, p->width, p->height); // the tiles k_nee_pass_f64 draws its work from
    if (cancellable) rtapi::arm_cancel_word(s, a); // the waves read it at their start and at chunk boundaries
    if ((rc = open_launches(s, stream)) != RT_OK) return rc;
    rtapi::note_launches(s, 0);
    return RT_OK;
}

int rtapi::enqueue_nee_pass(RtScene *s, NeePasses &np, int c0, int c1, hipStream_t stream, const uint32_t *tile_list, uint32_t n_list) {
    rtdev::TraceArgs &a = np.args;
    if (c0 < 0 || c1 <= c0 || c1 > a.total_chunks || (tile_list && n_list > (uint32_t)a.n_tiles))
        return fail(RT_ERR_INVALID_ARGUMENT, "enqueue_nee_pass: chunk range or tile list out of range");
    a.tile_list = tile_list;
    a.n_list = tile_list ? n_list : 0u;
    a.n_items = tile_list ? n_list : (uint32_t)a.n_tiles;
    a.n_chunks = 1;
    rtapi::RenderBuffers &b = s->buf;
    const size_t n = (size_t)a.width * (size_t)a.height * 3;
    for (int c = c0; c < c1; ++c) { // one launch per chunk: the kernel's header says why
        a.chunk_base = c;
        a.sample_begin = np.starts[(size_t)c];
        a.sample_end = np.starts[(size_t)c + 1];
        if (s->lights_extended) RT_HIP(s->kernels->nee_lights_pass(&a, &np.nee, &np.lights, s->textured, s->specular, s->use_bvh, stream));
        else RT_HIP(s->kernels->nee_pass(&a, &np.nee, s->prims_class, s->textured, s->specular, s->use_bvh, stream));
        RT_HIP(s->kernels->nee_chunk(b.accum.ptr, b.partial.ptr, b.squares.ptr, n, a.sample_end - a.sample_begin, stream));
    }
    ++s->last_launches;
    return RT_OK;
}

int rtapi::build_light_list(RtScene *s, const LightTables &t) {
    s->lights = t.lights;
    RT_HIP(s->nee_slot.alloc(t.slot.size()));
    if (!t.slot.empty()) RT_HIP(hipMemcpy(s->nee_slot.ptr, t.slot.data(), t.slot.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    RT_HIP(s->nee_prim.alloc(t.prim.size()));
    if (!t.prim.empty()) RT_HIP(hipMemcpy(s->nee_prim.ptr, t.prim.data(), t.prim.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return RT_OK;
}

// rt_scene_set_lights: the list of these params from the scene's own facts (rt_plan.cpp: list_lights), its device tables,
// and the pick of every cap n = 1 .. count (RtScene.nee_pick).  The scene's stream is idle first: no launch of an earlier
// call on it still reads the tables that are replaced.  ALL OR NOTHING: the three device tables are made and filled beside
// the scene's own, and the scene takes them — with the list, the params and the kernel choice that go with them — only
// once every allocation and copy has succeeded; a failure leaves the scene exactly as it was.
int rtapi::set_light_list(RtScene *s, const RtLightListParams &lp) {
    RT_HIP(hipSetDevice(s->device));
    RT_HIP(hipStreamSynchronize(s->buf.stream));
    const std::vector<int32_t> lights = rtapi::list_lights(s->light_facts, lp.kinds, kMaxLights);
    const LightTables t = rtapi::light_tables_of(lights, s->table_order);
    bool extended = lp.pick == RT_PICK_POWER;
    for (int32_t i : lights) extended = extended || !rtapi::light_is_plain(s->light_facts[(size_t)i]);
    const size_t count = lights.size();
    std::vector<char> uniform(count, 1);
    std::vector<double> rows(count * count * 2, 0.0);
    for (size_t n = 1; n <= count; ++n) {
        const rtapi::LightPick pick = rtapi::light_pick(s->light_facts, lights, (int)n, lp.pick);
        uniform[n - 1] = pick.uniform ? 1 : 0;
        std::copy(pick.p.begin(), pick.p.end(), rows.begin() + (n - 1) * 2 * count);
        std::copy(pick.cdf.begin(), pick.cdf.end(), rows.begin() + (n - 1) * 2 * count + count);
    }
    std::vector<double> weights = rtapi::light_pick(s->light_facts, lights, (int)count, lp.pick).p;

    // freed on every way out: after the exchange below they hold the scene's OLD tables
    rtapi::DevBuf<int32_t> fresh_slot, fresh_prim;
    rtapi::DevBuf<double> fresh_pick;
    auto fill = [](auto &buf, const auto &host) -> hipError_t {
        hipError_t e = buf.alloc(host.size());
        if (e == hipSuccess && !host.empty())
            e = hipMemcpy(buf.ptr, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice);
        return e;
    };
    RT_HIP(fill(fresh_slot, t.slot));
    RT_HIP(fill(fresh_prim, t.prim));
    RT_HIP(fill(fresh_pick, rows));
    // nothing below can fail
    std::swap(s->nee_slot, fresh_slot);
    std::swap(s->nee_prim, fresh_prim);
    std::swap(s->nee_pick, fresh_pick);
    s->lights = t.lights;
    s->light_params = lp;
    s->lights_extended = extended;
    s->pick_uniform.swap(uniform);
    s->pick_weights.swap(weights);
    return RT_OK;
}

namespace {
int scene_set_lights(RtScene *s, const RtLightListParams *p) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    const int rc = rtapi::check_light_list_params(p);
    if (rc != RT_OK) return rc;
    return rtapi::set_light_list(s, *p);
}

int scene_light_weights(const RtScene *s, double *out, int32_t capacity, int32_t *count) {
    if (!s || !count) return fail(RT_ERR_INVALID_ARGUMENT, "scene/out_count is NULL");
    if (capacity < 0 || (capacity > 0 && !out)) return fail(RT_ERR_INVALID_ARGUMENT, "out_p is NULL or capacity is negative");
    *count = (int32_t)s->pick_weights.size();
    for (int32_t k = 0; k < capacity && k < *count; ++k) out[k] = s->pick_weights[(size_t)k];
    return RT_OK;
}
} // namespace

extern "C" {

void rt_light_list_params_default(RtLightListParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->kinds = RT_LIGHTS_PLAIN;
    out->pick = RT_PICK_UNIFORM;
}

int rt_scene_set_lights(RtScene *s, const RtLightListParams *p) {
    return rtapi::guarded("rt_scene_set_lights", [&] { return scene_set_lights(s, p); });
}

int rt_scene_light_weights(RtScene *s, double *out_p, int32_t capacity, int32_t *out_count) {
    return rtapi::guarded("rt_scene_light_weights", [&] { return scene_light_weights(s, out_p, capacity, out_count); });
}

void rt_light_sampling_params_default(RtLightSamplingParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->heuristic = RT_MIS_POWER;
    out->max_lights = kMaxLights;
}

int rt_scene_lights(RtScene *s, int32_t *out_prims, int32_t capacity, int32_t *out_count) {
    return rtapi::guarded("rt_scene_lights", [&] { return scene_lights(s, out_prims, capacity, out_count); });
}

int rt_render_frame_nee(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                        double *out_rgb) {
    return rtapi::guarded("rt_render_frame_nee", [&] { return render_frame_nee(s, camera, p, ls, out_rgb); });
}

int rt_render_frame_nee_device(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                               double *rgb_device, void *hip_stream) {
    return rtapi::guarded("rt_render_frame_nee_device",
                          [&] { return render_frame_nee_device(s, camera, p, ls, rgb_device, hip_stream); });
}

int rt_render_frame_nee_strips_device(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                                      double *rgb_device, void *hip_stream) {
    return rtapi::guarded("rt_render_frame_nee_strips_device",
                          [&] { return render_frame_nee_strips_device(s, camera, p, ls, rgb_device, hip_stream); });
}

} // extern "C"
