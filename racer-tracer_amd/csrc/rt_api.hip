// rt_api.hip — the render side of the C ABI declared in include/rt_abi.h: a render's argument block, enqueue_render,
// which every render entry point goes through, cancel, statistics and the device-output entry points (the host-output
// ones live in rt_deliver.hip and rt_multi.hip).  Scenes are made in rt_scene_create.hip; the rules that need no device —
// the chunk plan, the pixel grid, the exponent of the fixed-point sums — are rt_plan.cpp's.
//
// Host code only (HIP runtime calls); the kernels live in rt_trace_kernel.hip (v1), rt_trace_pool_kernel.hip (pooled),
// rt_frame_kernels.hip (resolve, folds) and rt_post_kernel.hip.  Nothing here falls back to a CPU renderer: without a
// usable HIP device every entry point returns RT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <atomic>
#include <string>
#include <vector>
#include <thread>
#include <chrono>
#include "rt_scene.h"

extern "C" hipError_t rtdev_launch_post_rgba8(const RtToneMap *tm, const double *rgb, size_t n_pixels, uint8_t *rgba,
                                              double *mapped, hipStream_t stream);

using rtapi::Cancel;
using rtapi::Delivery;
using rtapi::chunk_plan;
using rtapi::fail;
using rtapi::owned_rows_of;

namespace {

int fill_args(const RtScene *s, const RtCamera *c, const RtRenderParams *p, rtdev::TraceArgs &a) {
    memset(&a, 0, sizeof a);
    a.prims = s->prims.ptr;
    a.textures = s->textures.ptr;
    a.images = s->images.ptr;
    a.perlins = s->perlins.ptr;
    a.n_prims = s->n_prims;
    a.n_materials = s->n_materials;
    a.n_textures = s->n_textures;
    a.n_images = s->n_images;
    a.n_perlins = s->n_perlins;
    a.perlin_identity = s->perlin_identity;
    a.perlin_in_lds = s->textured && s->n_perlins > 0 && s->perlin_identity;
    rtapi::fill_grid(p, a);
    for (int k = 0; k < 3; ++k) {
        a.cam.origin[k] = c->origin[k];
        a.cam.ulc[k] = c->upper_left_corner[k];
        a.cam.right[k] = c->right[k];
        a.cam.up[k] = c->up[k];
        a.cam.horizontal[k] = c->horizontal[k];
        a.cam.vertical[k] = c->vertical[k];
    }
    a.cam.lens_radius = c->lens_radius;
    a.lens_lds = c->lens_radius != 0.0;
    a.time_lds = s->has_moving;
    a.cam.time_a = c->time_a;
    a.cam.time_b = c->time_b;
    a.bg = s->bg;
    a.accum = s->buf.accum.ptr;
    a.segments = s->buf.segments.ptr;
    a.bvh_nodes = s->bvh_nodes.ptr;
    a.bvh_nodes_ordered = s->bvh_nodes_in_lds ? nullptr : s->bvh_nodes_ordered.ptr;
    a.bvh_prim_index = s->bvh_prim_index.ptr;
    a.n_bvh_nodes = s->n_bvh_nodes;
    for (int k = 0; k < 3; ++k) {
        a.bvh_root_mn[k] = s->bvh_root_mn[k];
        a.bvh_root_mx[k] = s->bvh_root_mx[k];
        a.bvh_center[k] = s->bvh_center[k];
    }
    a.bvh_lds_nodes = s->bvh_nodes_in_lds ? s->n_bvh_nodes + 1 : 0; // the sentinel behind the tree's nodes is staged too
    a.leaf_geo = s->leaf_geo.ptr;
    a.leaf_time_a = s->leaf_time_a;
    a.leaf_inv_dt = s->leaf_inv_dt;
    for (int g = 0; g < 3; ++g) a.rect_end[g] = s->rect_end[g];
    a.sphere_end = s->sphere_end;
    a.box_end = s->box_end;
    // Fixed-point sums (rt_device_types.h: sum_scale; the variants that keep two items in flight: any primitive kind, BVH)
    if (!s->exact && !s->use_v1 && (s->use_bvh || s->prims_class == 2)) {
        int e = 0;
        const int rc = rtapi::sum_exponent(s->radiance_bound, p->samples, &e);
        if (rc != RT_OK) return rc;
        if (e == 0) return fail(RT_ERR_UNSUPPORTED, "a scene without a radiance bound needs the f64 sums of RT_ARITH_REFERENCE"); // (scene_create)
        a.sum_scale = ldexp(1.0, 52 - e);
        a.sum_unscale = ldexp(1.0, e - 52);
    }
    // the pixels whose camera rays can hit anything (rt_primary_bounds.h), from this call's camera: nothing is kept between calls
    const rtdev::PixelRect seen = rtdev::primary_bounds(a.cam.origin, a.cam.ulc, a.cam.horizontal, a.cam.vertical, a.cam.lens_radius,
                                                        a.width, a.height, s->box_mn, s->box_mx);
    a.cull_px0 = seen.px0;
    a.cull_px1 = seen.px1;
    a.cull_py0 = seen.py0;
    a.cull_py1 = seen.py1;
    a.bg_black = rtdev::background_is_black(a.bg);
    static_assert(RT_BG_SOLID == 1, "rt_device_types.h: background_is_black");
#ifdef RT_DEVELOPER_KNOBS // throw-away kernel knobs of the developer build (tools/perf_ab.sh)
    for (int k = 0; k < 4; ++k) {
        char name[16];
        snprintf(name, sizeof name, "RT_DBG%d", k);
        if (const char *v = getenv(name)) a.dbg[k] = atoi(v);
    }
#endif
    return RT_OK;
}

} // namespace

int rtapi::fill_trace_args(const RtScene *s, const RtCamera *camera, const RtRenderParams *p, rtdev::TraceArgs &a) {
    return fill_args(s, camera, p, a);
}

// The counters of a delivering launch over `n_tiles` item tiles (zero between launches: fresh ones must be cleared).
int rtapi::reserve_delivery_counters(RtScene *s, size_t n_tiles) {
    rtapi::RenderBuffers &b = s->buf;
    bool grew = false;
    RT_HIP(b.tile_done.reserve(n_tiles, &grew));
    b.deliver_dirty = b.deliver_dirty || grew;
    RT_HIP(b.region_done.reserve((size_t)rtdev::RT_MAX_REGIONS, &grew));
    b.deliver_dirty = b.deliver_dirty || grew;
    return RT_OK;
}
using rtapi::reserve_delivery_counters;

// What a pooled-kernel launch of these parameters needs in device memory, allocated now.  enqueue_render does the same
// when it finds a buffer too small; a call over SEVERAL shares reserves for all of them before it launches the first
// (rt_deliver.hip, rt_multi.hip): hipMalloc waits for the device's running kernels, so a share that allocated inside its
// enqueue held the calling thread until the shares launched before it had finished — no cancel poll, no band copied
// meanwhile (measured with two scenes on one card: 122 ms of a 4096-spp frame before the hook was looked at).
int rtapi::reserve_render_buffers(RtScene *s, const RtRenderParams *p, bool delivering) {
    if (s->use_v1) return RT_OK;
    RT_HIP(hipSetDevice(s->device));
    const int owned = p->scale > 1 ? p->height : owned_rows_of(p); // (the preview's grid is smaller: an upper bound)
    const size_t slice_elems = (size_t)p->width * (size_t)owned * 3;
    const size_t chunks = (size_t)chunk_plan(p->samples).size() - 1;
    RT_HIP(s->buf.partial.reserve(slice_elems * chunks));
    RT_HIP(s->buf.queue.reserve(1));
    if (delivering) return reserve_delivery_counters(s, rtapi::tile_count(p->width, owned));
    return RT_OK;
}

namespace {

// The v1 kernel: sample batches into the accumulator, a synchronisation after each while a cancel hook is armed (so
// that the next poll is meaningful), then the resolve pass into out_device.
int enqueue_v1(RtScene *s, rtdev::TraceArgs &a, const RtRenderParams *p, double *out_device, hipStream_t stream, int batch,
               const Cancel &cancel, int &launches) {
    const size_t n = (size_t)p->width * (size_t)p->height * 3;
    RT_HIP(s->buf.accum.reserve(n));
    a.accum = s->buf.accum.ptr;
    RT_HIP(hipMemsetAsync(s->buf.segments.ptr, 0, rtdev::RT_STAT_SLOTS * sizeof(unsigned long long), stream));
    RT_HIP(hipEventRecord(s->buf.ev_begin, stream));
    for (int b = 0; b < p->samples; b += batch) {
        if (cancel.raised()) return RT_ERR_CANCEL_EVENT;
        a.sample_begin = b;
        a.sample_end = b + batch < p->samples ? b + batch : p->samples;
        RT_HIP(s->kernels->trace(&a, s->prims_class, s->textured, s->specular, stream));
        ++launches;
        if (cancel.armed()) RT_HIP(hipStreamSynchronize(stream));
    }
    RT_HIP(hipEventRecord(s->buf.ev_traced, stream));
    RT_HIP(s->kernels->resolve(s->buf.accum.ptr, out_device, p->width, p->height, a.strip_rows, a.strip_count, a.strip_index,
                               p->samples, stream));
    RT_HIP(hipEventRecord(s->buf.ev_resolved, stream));
    return RT_OK;
}

} // namespace

// A delivering launch (rt_deliver.hip): its items queued region by region (rt_plan.h: queue_order), its counters cleared
// where they must be.
int rtapi::setup_delivery(RtScene *s, rtdev::TraceArgs &a, const Delivery &delivery, int total_chunks, hipStream_t stream) {
    int rc = rtapi::queue_order(delivery.regions, a.tiles_x, a.n_tiles, total_chunks, a.regions, a.n_regions);
    if (rc != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    if ((rc = reserve_delivery_counters(s, (size_t)a.n_tiles)) != RT_OK) return rc;
    if (b.deliver_dirty) { // fresh buffers, or a launch that was cut short (cancel, error): counters back to zero
        RT_HIP(hipMemsetAsync(b.tile_done.ptr, 0, b.tile_done.count * sizeof(unsigned int), stream));
        RT_HIP(hipMemsetAsync(b.region_done.ptr, 0, b.region_done.count * sizeof(unsigned int), stream));
    }
    b.deliver_dirty = true; // until every region has been published (rt_deliver.hip clears it)
    a.deliver_out = delivery.out;
    a.tile_done = b.tile_done.ptr;
    a.region_done = b.region_done.ptr;
    a.deliver_flags = b.host_flags.ptr;
    a.deliver_serial = delivery.serial;
    a.deliver_col_step = delivery.col_step;
    a.deliver_cols = delivery.cols;
    return RT_OK;
}

namespace {
using rtapi::setup_delivery;

// A tree that lives in LDS is walked in ONE fixed child order: the order that suits the rays starting at this camera
// (rt_bvh.h: order_bvh_for_origin).  Re-emitted when the camera has moved — microseconds for the few hundred nodes LDS
// holds — and copied in stream order, i.e. behind whatever launch of this scene still walks the old array.
int order_bvh_for_camera(RtScene *s, const RtCamera *camera, hipStream_t stream) {
    if (!s->use_bvh || !s->bvh_nodes_in_lds || s->bvh_host.nodes.empty()) return RT_OK;
    if (s->bvh_is_ordered && camera->origin[0] == s->bvh_ordered_for[0] && camera->origin[1] == s->bvh_ordered_for[1] &&
        camera->origin[2] == s->bvh_ordered_for[2])
        return RT_OK;
    s->bvh_upload_slot ^= 1; // (two host copies in turn: the one a pending copy may still read is left alone)
    std::vector<rtdev::BvhNode> &arr = s->bvh_ordered_nodes[s->bvh_upload_slot];
    arr = rtdev::order_bvh_for_origin(s->bvh_host, camera->origin);
    RT_HIP(hipMemcpyAsync(s->bvh_nodes.ptr, arr.data(), arr.size() * sizeof(rtdev::BvhNode), hipMemcpyHostToDevice, stream));
    for (int k = 0; k < 3; ++k) s->bvh_ordered_for[k] = camera->origin[k];
    s->bvh_is_ordered = true;
    return RT_OK;
}

// The item grid and chunk table of a pooled render, after checking that a block fits one CU's LDS: the primitive table
// of the linear loop, the textures, the Perlin gradients, the lens samples and the ray times all come on top of the
// kernel's static LDS (rt_device_types.h: pool_lds_layout).  A launch that does not fit is refused here, before anything
// is enqueued; the lens part depends on the camera.  max_blocks: the variant's resident blocks on the device, or the
// scene's launch_blocks where that is less.
int setup_pool_grid(const RtScene *s, rtdev::TraceArgs &a, const RtRenderParams *p, std::vector<int> &starts,
                     unsigned &max_blocks) {
    const size_t lds = (size_t)s->pool_static_lds + (a.lens_lds ? s->pool_dyn_lds_lens : s->pool_dyn_lds);
    const int blocks_per_cu = a.lens_lds ? s->pool_blocks_per_cu_lens : s->pool_blocks_per_cu;
    if (lds > rtdev::kLdsPerCu || blocks_per_cu < 1)
        return fail(RT_ERR_UNSUPPORTED, a.lens_lds ? "the trace kernel's LDS (static + tables + lens samples) exceeds a CU's 160 KiB"
                                                   : "the trace kernel's LDS (static + tables) exceeds a CU's 160 KiB");
    max_blocks = rtapi::cap_blocks(s, (unsigned)(s->num_cus * blocks_per_cu));
    rtapi::set_tile_grid(a, a.cover_w / a.step_x, a.owned_rows); // grid cells per row x grid rows
    starts = chunk_plan(p->samples);
    rtapi::set_chunk_table(a, starts);
    return RT_OK;
}

// What precedes a pooled render's first launch, in stream order: slices and `n_launches` item counters allocated where
// they are short, the segment and item counters cleared, the cancel word armed (`cancellable`: the waves read it with
// every item they fetch), the tree ordered for the camera, ev_begin recorded.
int pool_prologue(RtScene *s, rtdev::TraceArgs &a, const RtCamera *camera, const RtRenderParams *p, size_t n_launches,
                  bool cancellable, hipStream_t stream) {
    rtapi::RenderBuffers &b = s->buf;
    if (cancellable) rtapi::arm_cancel_word(s, a);
    // slices hold the launch's owned rows only (the kernel compacts rows: owned_rows, tile_py0)
    a.slice_rows = a.owned_rows;
    const size_t slice_elems = (size_t)p->width * (size_t)a.slice_rows * 3;
    RT_HIP(b.partial.reserve(slice_elems * (size_t)a.total_chunks));
    RT_HIP(b.queue.reserve(n_launches));
    a.partial = b.partial.ptr;
    RT_HIP(hipMemsetAsync(b.segments.ptr, 0, rtdev::RT_STAT_SLOTS * sizeof(unsigned long long), stream));
#ifdef RT_PROFILE_REGIONS
    RT_HIP(hipMemsetAsync(b.segments.ptr + rtdev::RT_STAT_WALL + 0, 0xff, sizeof(unsigned long long), stream)); // min slots
    RT_HIP(hipMemsetAsync(b.segments.ptr + rtdev::RT_STAT_WALL + 2, 0xff, sizeof(unsigned long long), stream));
#endif
    RT_HIP(hipMemsetAsync(b.queue.ptr, 0, sizeof(unsigned int) * b.queue.count, stream));
    const int rc = order_bvh_for_camera(s, camera, stream);
    if (rc != RT_OK) return rc;
    RT_HIP(hipEventRecord(b.ev_begin, stream));
    return RT_OK;
}

// Launch number `index` of a render: chunks [first_chunk, first_chunk + n_chunks) of every tile, or of the n_list tiles of
// `tile_list` (device memory; one-region launches only).
int launch_pool(RtScene *s, rtdev::TraceArgs &a, const std::vector<int> &starts, int first_chunk, int n_chunks, int index,
                unsigned max_blocks, hipStream_t stream, const uint32_t *tile_list = nullptr, uint32_t n_list = 0) {
    if (tile_list && (a.n_regions > 1 || n_list > (uint32_t)a.n_tiles))
        return fail(RT_ERR_INVALID_ARGUMENT, "a tile list is for one-region launches, at most one entry per tile");
    a.sample_begin = starts[(size_t)first_chunk];
    a.sample_end = starts[(size_t)(first_chunk + n_chunks)];
    a.n_chunks = n_chunks;
    a.chunk_base = first_chunk;
    a.tile_list = tile_list;
    a.n_list = tile_list ? n_list : 0u;
    const uint32_t tiles = tile_list ? n_list : (uint32_t)a.n_tiles;
    a.n_items = (uint32_t)a.n_chunks * tiles;
    if ((uint64_t)a.n_chunks * (uint64_t)tiles >= 0x40000000ull) // the item counter's top bit is the cancel poison
        return fail(RT_ERR_UNSUPPORTED, "more than 2^30 work items in one launch");
    a.queue = s->buf.queue.ptr + index;
    const unsigned blocks = std::min(max_blocks, (a.n_items + 3) / 4);
    rtapi::note_grid(s, blocks, a.n_items);
    // the pixel rectangle of every rect record (rt_primary_bounds.h), from this call's camera like the scene's own, which
    // fill_args has put into `a`: the kernel's second argument (tests/test_background_flag_cpu.py holds TraceArgs to
    // ending at bg_black).  A few dozen 3x3 determinants per launch; nothing is kept between calls.
    const rtdev::PrimaryRects rects = rtdev::primary_rects(a.cam.origin, a.cam.ulc, a.cam.horizontal, a.cam.vertical, a.width, a.height,
                                                           rtdev::PixelRect{a.cull_px0, a.cull_px1, a.cull_py0, a.cull_py1},
                                                           s->primary_rect_geo.data(), (int)s->primary_rect_geo.size());
    RT_HIP(s->kernels->trace_pool(&a, &rects, s->prims_class, s->textured, s->specular, s->use_bvh, blocks, stream));
    return RT_OK;
}

// The pooled kernel: work items = 8x8 tiles x sample chunks, one launch per batch of chunks, then — without a Delivery —
// the resolve pass into out_device.
int enqueue_pool(RtScene *s, rtdev::TraceArgs &a, const RtCamera *camera, const RtRenderParams *p, double *out_device,
                 hipStream_t stream, int batch, const Cancel &cancel, const Delivery *delivery, int out_col_step,
                 int out_cols, int &launches) {
    std::vector<int> starts;
    unsigned max_blocks = 0;
    int rc = setup_pool_grid(s, a, p, starts, max_blocks);
    if (rc != RT_OK) return rc;
    const int total_chunks = a.total_chunks;
    const std::vector<rtapi::Launch> plan = rtapi::plan_launches(starts, batch);
    if (delivery) { // one launch, finishing its own pixels
        if (plan.size() != 1 || p->scale > 1) return fail(RT_ERR_UNSUPPORTED, "a delivering launch is one whole-frame launch");
        if ((rc = setup_delivery(s, a, *delivery, total_chunks, stream)) != RT_OK) return rc;
    }
    rtapi::RenderBuffers &b = s->buf;
    // a call whose caller polls a cancel hook: the waves read the scene's cancel word with every item they fetch
    if ((rc = pool_prologue(s, a, camera, p, plan.size(), cancel.armed() || (delivery && delivery->cancellable), stream)) != RT_OK)
        return rc;
    // a slice is only written for the pixels a launch covers; unowned rows are skipped by the resolve
    int chunks_done = 0;
    for (const rtapi::Launch &l : plan) {
        if (cancel.raised()) return RT_ERR_CANCEL_EVENT;
        if ((rc = launch_pool(s, a, starts, l.first_chunk, l.n_chunks, launches, max_blocks, stream)) != RT_OK) return rc;
        chunks_done += a.n_chunks;
        ++launches;
    }
    RT_HIP(hipEventRecord(b.ev_traced, stream));
    if (!delivery)
        RT_HIP(s->kernels->resolve_chunks(b.partial.ptr, out_device, p->width, p->height, chunks_done, a.slice_rows, a.strip_rows,
                                          a.strip_count, a.strip_index, a.step_x, a.step_y, a.cover_w, a.cover_h, out_col_step,
                                          out_cols, p->samples, stream));
    RT_HIP(hipEventRecord(b.ev_resolved, stream));
    return RT_OK;
}

} // namespace

int rtapi::enqueue_render(RtScene *s, const RtCamera *camera, const RtRenderParams *p, double *out_device,
                          hipStream_t stream, int batch, const Cancel &cancel, const Delivery *delivery, int out_col_step,
                          int out_cols) {
    RT_HIP(hipSetDevice(s->device));
    rtdev::TraceArgs a;
    int rc = fill_args(s, camera, p, a);
    if (rc != RT_OK) return rc;
    if (batch <= 0 || batch > p->samples) batch = p->samples;
    int launches = 0;
    if (s->use_v1) {
        if (p->scale > 1) return fail(RT_ERR_UNSUPPORTED, "the v1 kernel has no preview mode");
        if (delivery || out_cols > 1) return fail(RT_ERR_UNSUPPORTED, "the v1 kernel does not deliver its own pixels");
        rc = enqueue_v1(s, a, p, out_device, stream, batch, cancel, launches);
    } else {
        rc = enqueue_pool(s, a, camera, p, out_device, stream, batch, cancel, delivery, out_col_step, out_cols, launches);
    }
    if (rc != RT_OK) return rc;
    note_launches(s, launches);
    return RT_OK;
}
using rtapi::enqueue_render;

int rtapi::begin_passes(RtScene *s, const RtCamera *camera, const RtRenderParams *p, hipStream_t stream, int max_launches,
                        bool cancellable, PoolPasses &pp) {
    if (s->use_v1 || p->strip_count > 1 || p->scale > 1 || max_launches < 1)
        return fail(RT_ERR_UNSUPPORTED, "passes are whole-frame launches of the pooled kernel");
    RT_HIP(hipSetDevice(s->device));
    int rc = fill_args(s, camera, p, pp.args);
    if (rc != RT_OK) return rc;
    if ((rc = setup_pool_grid(s, pp.args, p, pp.starts, pp.max_blocks)) != RT_OK) return rc;
    if ((rc = pool_prologue(s, pp.args, camera, p, (size_t)max_launches, cancellable, stream)) != RT_OK) return rc;
    pp.launches = 0;
    pp.max_launches = max_launches;
    note_launches(s, 0);
    return RT_OK;
}

int rtapi::enqueue_chunks(RtScene *s, PoolPasses &pp, int c0, int c1, hipStream_t stream, const uint32_t *tile_list,
                          uint32_t n_list) {
    if (c0 < 0 || c1 <= c0 || c1 > pp.args.total_chunks || pp.launches >= pp.max_launches)
        return fail(RT_ERR_INVALID_ARGUMENT, "enqueue_chunks: chunk range or launch count out of range");
    const int rc = launch_pool(s, pp.args, pp.starts, c0, c1 - c0, pp.launches, pp.max_blocks, stream, tile_list, n_list);
    if (rc != RT_OK) return rc;
    s->last_launches = ++pp.launches;
    return RT_OK;
}

// Block until `ev` has happened; with a cancel hook, poll it meanwhile and give up
// (RT_ERR_CANCEL_EVENT) as soon as it is raised.
int rtapi::wait_event(hipEvent_t ev, const Cancel &cancel) {
    if (!cancel.armed()) {
        RT_HIP(hipEventSynchronize(ev));
        return RT_OK;
    }
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return RT_OK;
        if (e != hipErrorNotReady) return fail(RT_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
        (void)hipGetLastError(); // hipErrorNotReady is sticky in hipGetLastError otherwise
        if (cancel.raised()) return RT_ERR_CANCEL_EVENT;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// Ends the pool launches of the current call early.  Two ways at once:
// * the scene's CANCEL WORD in pinned host memory (TraceArgs.cancel_flag), which the lane that fetches a wave's next item
//   reads: a CPU store, seen by every wave at its next item — the way that always works;
// * every item counter of the call becomes 2^31 (enqueue_render keeps a launch below 2^30 items, so no count of further
//   hand-outs wraps it), written with hipStreamWriteValue32 on a third stream behind ev_begin (which the render stream
//   records BEHIND its own clearing of the counters, so a cancel raised right after the enqueue cannot be erased).
//   Rounds 2 and 3 relied on this one alone and took it for a command-processor write; it is a small kernel of the
//   runtime's, which lands only while a SIMD has registers to spare: beside the 80-VGPR cornell variant (the one the
//   cancel test rendered) within an item's time, beside a 128-VGPR variant — four waves x 128 = the whole file — or
//   while another share's launch waits on the same device, not before the launch has ended (round 4 found it when the
//   cancel tests began to count the rays a cancelled launch had started instead of taking its time).  It still covers
//   the v1 kernel's launches and anything not yet started.
int rtapi::poison_queue_begin(RtScene *s) {
    // 1. the cancel word in pinned memory, which every wave reads with its next item: a CPU store, lands at once
    if (s->buf.host_flags.ptr) {
        reinterpret_cast<volatile unsigned int *>(s->buf.host_flags.ptr)[rtdev::RT_MAX_REGIONS] = 1u;
        std::atomic_thread_fence(std::memory_order_seq_cst);
    }
    // 2. the item counters themselves, for a launch that has not started yet or a caller without the word (the v1
    //    kernel's batches); this write is a small kernel of the runtime's and lands when it finds room
    RT_HIP(hipSetDevice(s->device));
    RT_HIP(hipStreamWaitEvent(s->buf.stream_ctl, s->buf.ev_begin, 0));
    bool by_cp = true;
    for (size_t i = 0; i < s->buf.queue.count && by_cp; ++i)
        by_cp = hipStreamWriteValue32(s->buf.stream_ctl, s->buf.queue.ptr + i, 0x80000000u, 0) == hipSuccess;
    if (!by_cp) { // a runtime without stream memory operations: a fill kernel does it, once it finds room
        (void)hipGetLastError();
        RT_HIP(hipMemsetD32Async((hipDeviceptr_t)s->buf.queue.ptr, (int)0x80000000u, s->buf.queue.count, s->buf.stream_ctl));
    }
    return RT_OK;
}

int rtapi::poison_queue(RtScene *s) {
    const int rc = poison_queue_begin(s);
    if (rc != RT_OK) return rc;
    RT_HIP(hipStreamSynchronize(s->buf.stream_ctl));
    return RT_OK;
}

namespace {

// ------------------------------------------------------------------------------------------ device-output entry points
int post_rgba8(RtScene *s, const RtToneMap *tm, const double *rgb_device, size_t n_pixels, uint8_t *rgba_device,
               double *mapped_device, hipStream_t stream) {
    if (!s || !tm || !rgb_device || !rgba_device) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (tm->kind < RT_TM_NONE || tm->kind > RT_TM_ACES) return fail(RT_ERR_INVALID_ARGUMENT, "unknown tone map kind");
    RT_HIP(hipSetDevice(s->device));
    RT_HIP(rtdev_launch_post_rgba8(tm, rgb_device, n_pixels, rgba_device, mapped_device, stream));
    return RT_OK;
}

int render_frame_rgba8(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtToneMap *tm, uint8_t *out_rgba) {
    if (!s || !tm || !out_rgba) return fail(RT_ERR_INVALID_ARGUMENT, "scene/tone_map/out is NULL");
    int rc = rtapi::check_params(camera, p);
    if (rc != RT_OK) return rc;
    if (p->strip_count > 1) // the packed frame is a whole picture; gather strips with rt_render_frame_device, then rt_post_rgba8_device
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_frame_rgba8 packs the whole frame: strip ownership is not supported here");
    RT_HIP(hipSetDevice(s->device));
    rtapi::RenderBuffers &b = s->buf;
    const size_t px = (size_t)p->width * (size_t)p->height;
    RT_HIP(b.frame.reserve(px * 3));
    RT_HIP(b.rgba.reserve(px * 4));
    rc = enqueue_render(s, camera, p, b.frame.ptr, b.stream, 0, Cancel());
    if (rc != RT_OK) return rc;
    rc = post_rgba8(s, tm, b.frame.ptr, px, b.rgba.ptr, nullptr, b.stream);
    if (rc != RT_OK) return rc;
    RT_HIP(hipStreamSynchronize(b.stream));
    RT_HIP(hipMemcpy(out_rgba, b.rgba.ptr, px * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

int last_stats(RtScene *s, RtRenderStats *out) {
    if (!s || !out) return fail(RT_ERR_INVALID_ARGUMENT, "scene/out is NULL");
    memset(out, 0, sizeof *out);
    if (!s->has_stats) return RT_OK;
    RT_HIP(hipSetDevice(s->device));
    RT_HIP(hipEventSynchronize(s->buf.ev_resolved));
    float ms_trace = 0.f, ms_resolve = 0.f;
    RT_HIP(hipEventElapsedTime(&ms_trace, s->buf.ev_begin, s->buf.ev_traced));
    RT_HIP(hipEventElapsedTime(&ms_resolve, s->buf.ev_traced, s->buf.ev_resolved));
    unsigned long long counters[rtdev::RT_STAT_SLOTS]; // rt_device_types.h: RT_STAT_*
    RT_HIP(hipMemcpy(counters, s->buf.segments.ptr, sizeof counters, hipMemcpyDeviceToHost));
    const unsigned long long segs = counters[rtdev::RT_STAT_SEGMENTS];
#ifdef RT_PROFILE_REGIONS
    {
        const unsigned long long *c = counters;
        static const char *names[16] = {"item setup", "batches", "hand-out + primary ray", "closest hit", "miss / material",
                                        "sampler", "scatter + accumulate", "item end", "hit record", "texture, step 1",
                                        "Noise rounds", "BVH: descent to a leaf", "BVH: leaf primitives", "-", "-", "-"};
        double total = 0;
        for (int k = 0; k < 16; ++k) total += (double)c[rtdev::RT_STAT_REGIONS + k];
        for (int k = 0; k < 13; ++k)
            if (k < 11 || c[rtdev::RT_STAT_REGIONS + k])
            fprintf(stderr, "region %-24s %6.2f %%  (%.3g wave-cycles, %4.1f lanes active at its closing marker)\n", names[k],
                    100.0 * (double)c[rtdev::RT_STAT_REGIONS + k] / total, (double)c[rtdev::RT_STAT_REGIONS + k],
                    c[rtdev::RT_STAT_REGIONS + k] ? (double)c[rtdev::RT_STAT_REGION_LANES + k] / (double)c[rtdev::RT_STAT_REGIONS + k] : 0.0);
        if (c[rtdev::RT_STAT_NOISE])
            fprintf(stderr, "region noise lookups: %.3g wave-iterations with one, %.1f lanes each on average\n", (double)c[rtdev::RT_STAT_NOISE],
                    (double)c[rtdev::RT_STAT_NOISE + 1] / (double)c[rtdev::RT_STAT_NOISE]);
        if (c[rtdev::RT_STAT_NOISE + 2])
            fprintf(stderr, "region BVH walk: %.1f nodes visited and %.1f leaf primitives tested per segment\n",
                    (double)c[rtdev::RT_STAT_NOISE + 2] / (double)segs, (double)c[rtdev::RT_STAT_NOISE + 3] / (double)segs);
        // lanes tracing per iteration: while the pool has paths to hand out / in the item's tail
        for (int part = 0; part < 2; ++part) {
            const unsigned long long *h = c + (part ? rtdev::RT_STAT_LANES_TAIL : rtdev::RT_STAT_LANES_BODY);
            double iters = 0, lanes = 0;
            for (int k = 0; k < 9; ++k) {
                iters += (double)h[k];
                lanes += (double)h[k] * (k == 0 ? 0.0 : 8.0 * k - 3.5); // bin centre
            }
            fprintf(stderr, "region lanes tracing, %s: %.4g iterations, mean %.1f lanes; bins 0|1-8|..|57-64:", part ? "item tail (pool dry)" : "pool not dry  ",
                    iters, iters > 0 ? lanes / iters : 0.0);
            for (int k = 0; k < 9; ++k) fprintf(stderr, " %.1f%%", iters > 0 ? 100.0 * (double)h[k] / iters : 0.0);
            fprintf(stderr, "\n");
        }
        // 100 MHz wall clock: when did the first/last wave start and end (last launch of the call)
        const unsigned long long *w = c + rtdev::RT_STAT_WALL;
        fprintf(stderr, "region waves: last start +%.3f ms, first end +%.3f ms, last end +%.3f ms after the first start\n",
                (double)(w[1] - w[0]) * 1e-5, (double)(w[2] - w[0]) * 1e-5, (double)(w[3] - w[0]) * 1e-5);
    }
#endif
    out->samples = counters[rtdev::RT_STAT_SAMPLES]; // counted on the device where a path is handed out
    out->segments = segs;
    out->kernel_ms = s->summed_times ? s->summed_kernel_ms : ms_trace;
    out->resolve_ms = s->summed_times ? s->summed_resolve_ms : ms_resolve;
    out->kernel_launches = s->last_launches;
    return RT_OK;
}

} // namespace

// ------------------------------------------------------------------------------------------------------- C entry points
// Every one that returns a status runs its body through rtapi::guarded; the others cannot throw.
extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *rt_strerror(int code) {
    switch (code) {
    case RT_OK: return "Ok";
    case RT_ERR_FAILED_TO_CREATE_WINDOW: return "Failed to create window";
    case RT_ERR_FAILED_TO_UPDATE_WINDOW: return "Failed to update window";
    case RT_ERR_CONFIGURATION: return "Config Error";
    case RT_ERR_UNKNOWN_MATERIAL: return "Unknown Material";
    case RT_ERR_FAILED_TO_ACQUIRE_LOCK: return "Failed to acquire lock";
    case RT_ERR_EXIT_EVENT: return "Exit event";
    case RT_ERR_CANCEL_EVENT: return "Cancel event";
    case RT_ERR_IMAGE_SAVE: return "Image save error";
    case RT_ERR_SCENE_LOAD: return "Scene failed to load";
    case RT_ERR_ARGUMENT_PARSING: return "Argument parsing Error";
    case RT_ERR_KEY: return "Key callback failed";
    case RT_ERR_CREATE_LOG: return "Failed to create log";
    case RT_ERR_RECEIVE: return "Failed to recieve data";
    case RT_ERR_SEND: return "Failed to send data";
    case RT_ERR_ACTION_PROTOCOL: return "Action protocol error";
    case RT_ERR_BUS_WRITE: return "Failed to write data to bus";
    case RT_ERR_BUS_READ: return "Failed to read data from bus";
    case RT_ERR_BUS_UPDATE: return "Failed to update databus";
    case RT_ERR_BUS_TIMEOUT: return "Bus timeout error";
    case RT_ERR_NO_OBJECT_WITH_ID: return "No object with id";
    case RT_ERR_FAILED_TO_OPEN_IMAGE: return "Failed to open image";
    case RT_ERR_FAILED_TO_PARSE: return "Failed to parse into a vector";
    case RT_ERR_NO_DEVICE: return "No usable HIP device";
    case RT_ERR_HIP: return "HIP runtime error";
    case RT_ERR_INVALID_ARGUMENT: return "Invalid argument";
    case RT_ERR_UNSUPPORTED: return "Unsupported scene feature";
    case RT_ERR_OUT_OF_MEMORY: return "Out of memory";
    default: return "Unknown error";
    }
}

int rt_render_frame_device(RtScene *s, const RtCamera *camera, const RtRenderParams *p, double *out_dev,
                           void *hip_stream) {
    return rtapi::guarded("rt_render_frame_device", [&] {
        if (!s || !out_dev) return fail(RT_ERR_INVALID_ARGUMENT, "scene/out is NULL");
        int rc = rtapi::check_params(camera, p);
        if (rc != RT_OK) return rc;
        return enqueue_render(s, camera, p, out_dev, (hipStream_t)hip_stream, 0, Cancel());
    });
}

int rt_post_rgba8_device(RtScene *s, const RtToneMap *tm, const double *rgb_device, size_t n_pixels,
                         uint8_t *rgba_device, double *mapped_device, void *hip_stream) {
    return rtapi::guarded("rt_post_rgba8_device", [&] {
        return post_rgba8(s, tm, rgb_device, n_pixels, rgba_device, mapped_device, (hipStream_t)hip_stream);
    });
}

int rt_render_frame_rgba8(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtToneMap *tm,
                          uint8_t *out_rgba) {
    return rtapi::guarded("rt_render_frame_rgba8", [&] { return render_frame_rgba8(s, camera, p, tm, out_rgba); });
}

int rt_scene_last_stats(RtScene *s, RtRenderStats *out) {
    return rtapi::guarded("rt_scene_last_stats", [&] { return last_stats(s, out); });
}

int rtdev_sum_exponent(double bound, int32_t samples, int32_t *e) {
    return rtapi::guarded("rtdev_sum_exponent", [&] {
        if (!e) return fail(RT_ERR_INVALID_ARGUMENT, "e is NULL");
        int k = 0;
        const int rc = rtapi::sum_exponent(bound, samples, &k);
        *e = k;
        return rc;
    });
}

} // extern "C"
