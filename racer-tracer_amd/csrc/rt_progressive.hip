// rt_progressive.hip — rt_render_progressive and rt_render_adaptive: the whole frame handed to the caller once per pass
// while it converges, the last pass's frame being rt_render_frame's.
//
// The reference's author wanted this shape: renderer/denoised.rs:291-331 renders the frame in passes and writes a
// whole-frame BufferUpdate after each (:210-216).  Here a pass is a run of whole chunks of the frame's chunk plan (rt_plan.cpp:
// chunk_plan, a function of the TOTAL sample count), traced by one launch of the pooled kernel into the chunks' slices.  A
// fold pass (k_fold_chunks_f64) then adds those slices to the running per-pixel sums (RenderBuffers.accum) in chunk order
// and writes sqrt(sum / samples so far).  The running sums start at +0.0, so after the last pass they are
// k_resolve_chunks_f64's left fold over every slice — the sum the delivering launch of rt_render_frame forms — and the frame
// is bit-identical.  Draws are addressed by (pixel, sample, ...) (include/rt_rng.h), so samples [0, s) are the same whatever
// the total: an earlier frame is an s-spp frame summed in another order.
//
// Schedule (frame slot k % 2, on the device and in pinned host memory): the render stream runs pass k's launch, its fold
// into device slot k % 2 and records ev_folded; the copy stream waits for that and copies the slot into pinned slot k % 2
// (ev_copied).  The calling thread keeps the GPU one pass ahead of the callback: passes 0 and 1 are enqueued, then for
// every k it waits for copy k (polling the cancel hook), runs callback k on the pinned slot and only then enqueues pass
// k + 2 — whose fold waits for copy k (same device slot) and whose copy overwrites the pinned slot callback k has read.
//
// rt_render_adaptive runs the same passes through the same loop: pass k traces the tiles that
// fold k - 1 left running (TraceArgs.tile_list), k_fold_adaptive_f64 folds, measures every running tile's error and
// stops it or lists it for pass k + 1, and the count of running tiles travels to the host ahead of the frame.
//
// rt_render_progressive_nee and rt_render_adaptive_nee are the same loop with the next-event
// estimator: a pass is one launch of k_nee_pass_f64 (rt_nee_pass_kernel.hip), which adds the pass's samples to the running
// sums itself — there are no slices and no fold — and k_nee_decide_f64 behind it writes the frame slot and, adaptive,
// decides every running tile.  Slots, events, cancel polling and the count-ahead-of-frame hand-off are unchanged.
//
// Host code only.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "rt_scene.h"

using rtapi::Cancel;
using rtapi::fail;
using rtapi::pass_ends;

namespace {

// rt_render_adaptive's side of a call (rt_render_progressive and its denoised form have none): its parameters, checked,
// and the caller's outputs.
struct Adaptive {
    const RtAdaptiveParams *params;
    double *out_rgb;
    int32_t *out_samples;
    double *out_tile_error;
};

// What rt_render_adaptive refuses before it looks at the scene.
int check_adaptive(const RtRenderParams *p, const RtAdaptiveParams *a, const double *out_rgb) {
    if (!a) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive is NULL");
    if (!out_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgb is NULL");
    if (!std::isfinite(a->threshold)) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive->threshold must be finite");
    if (a->pass_samples <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive->pass_samples must be positive");
    if (a->min_samples < 0) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive->min_samples must not be negative");
    for (int k = 0; k < 4; ++k)
        if (a->_reserved[k] != 0) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive->_reserved must be 0");
    if (p && p->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive frames are whole frames: params->strip_* is not supported here");
    if (p && p->scale > 1) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive frames are full-resolution frames: params->scale must be 0 or 1");
    return RT_OK;
}

// Everything the call needs, allocated before its first launch (a hipMalloc between passes would wait for the running
// kernels): slices, one item counter per pass, the running sums, `slots` device and pinned frame slots, the copy stream and
// the events of the slots; adaptive (n_tiles > 0): the sums of squares and the per-tile state, lists and counts.
// nee: the NEE passes keep no slices and no item counters (their per-tile state is the adaptive one: n_tiles > 0).
int reserve_passes(RtScene *s, const RtRenderParams *p, int passes, size_t n, int slots, size_t n_tiles, bool nee) {
    int rc = nee ? RT_OK : rtapi::reserve_render_buffers(s, p, false);
    if (rc != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    if (!nee) RT_HIP(b.queue.reserve((size_t)passes));
    if (nee) RT_HIP(b.partial.reserve(n)); // (here: the running sums at the last chunk boundary)
    RT_HIP(b.accum.reserve(n));
    RT_HIP(b.frame.reserve((size_t)slots * n));
    if ((rc = rtapi::ensure_host_frame(s, (size_t)slots * n)) != RT_OK) return rc;
    RT_HIP(b.stream_copy.ensure(hipStreamNonBlocking));
    for (int k = 0; k < slots; ++k) { // (the spans are read with hipEventElapsedTime: timing events)
        RT_HIP(b.ev_pass_begin[k].ensure());
        RT_HIP(b.ev_pass_traced[k].ensure());
        RT_HIP(b.ev_folded[k].ensure());
        RT_HIP(b.ev_copied[k].ensure(hipEventDisableTiming));
        if (n_tiles) RT_HIP(b.ev_counted[k].ensure(hipEventDisableTiming));
    }
    if (n_tiles) {
        RT_HIP(b.squares.reserve(n));
        RT_HIP(b.tile_stop.reserve(n_tiles));
        RT_HIP(b.tile_scale.reserve(n_tiles));
        RT_HIP(b.tile_err.reserve(3 * n_tiles));
        RT_HIP(b.tile_lists.reserve(2 * n_tiles));
        RT_HIP(b.tile_counts.reserve((size_t)passes));
        RT_HIP(b.host_counts.reserve(rtdev::RT_MAX_CHUNKS, hipHostMallocDefault));
    }
    return RT_OK;
}

// dn: the filter of rt_render_progressive_denoised, or NULL.  ad: rt_render_adaptive's outputs and parameters, or NULL.
// The adaptive form keeps three frame slots and enqueues pass k + 1 as soon as pass k's running-tile count has arrived —
// before callback k, and only if a tile still runs — so that a cancel seen while pass k + 1 waits still finds the slots
// of pass k whole (pass k + 2 may be enqueued by then).
// nee: the light sampling of rt_render_progressive_nee / rt_render_adaptive_nee (checked by the caller), or NULL: the plain
// estimator.
int render_progressive(RtScene *s, const RtCamera *camera, const RtRenderParams *p, int pass_samples, RtFrameCallback callback,
                       void *user, const Cancel &cancel, const RtDenoiseParams *dn = nullptr, const Adaptive *ad = nullptr,
                       const RtLightSamplingParams *nee = nullptr) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (!callback && !ad) return fail(RT_ERR_INVALID_ARGUMENT, "callback is NULL");
    if (pass_samples <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "pass_samples must be positive");
    int rc = rtapi::check_params(camera, p);
    if (rc != RT_OK) return rc;
    if (p->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "progressive frames are whole frames: params->strip_* is not supported here");
    if (p->scale > 1) return fail(RT_ERR_INVALID_ARGUMENT, "progressive frames are full-resolution frames: params->scale must be 0 or 1");
    if (dn && (rc = rtapi::check_denoise(p, dn)) != RT_OK) return rc;
    if (s->use_v1 && !nee) return fail(RT_ERR_UNSUPPORTED, "rt_render_progressive needs the pooled kernel (the v1 kernel has no sample chunks)");
    if (cancel.raised()) return RT_ERR_CANCEL_EVENT; // cpu.rs:82-85, as rt_render_ex
    RT_HIP(hipSetDevice(s->device));
    const std::vector<int> starts = rtapi::chunk_plan(p->samples);
    const std::vector<int> ends = pass_ends(starts, pass_samples);
    const int passes = (int)ends.size();
    const size_t n = (size_t)p->width * (size_t)p->height * 3; // a frame, and a slice (whole-frame slices: slice_rows = height)
    const int slots = ad ? 3 : 2;
    const int tiles_x = rtapi::tiles_across(p->width);
    const size_t n_tiles = ad || nee ? rtapi::tile_count(p->width, p->height) : 0;
    if ((rc = reserve_passes(s, p, passes, n, slots, n_tiles, nee != nullptr)) != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    // denoised: the guides, the filter's scratch and a third device frame slot, the filter's output
    if (dn && (rc = rtapi::reserve_denoise(s, n / 3, true)) != RT_OK) return rc;
    if (dn) RT_HIP(b.frame.reserve(3 * n));
    const RtGuides guides = dn ? rtapi::scene_guides(s, n / 3) : RtGuides();
    const hipStream_t stream = b.stream, copy = b.stream_copy;
    rtapi::PoolPasses pp;
    rtapi::NeePasses np;
    double kernel_ms = 0.0, fold_ms = 0.0;
    uint32_t running = (uint32_t)n_tiles; // adaptive: the tiles the next pass traces
    int delivered = -1;                    // the last pass whose callback has run

    auto enqueue_pass = [&](int k) -> int {
        const int slot = k % slots, c0 = k > 0 ? ends[(size_t)k - 1] : 0, c1 = ends[(size_t)k];
        double *dev = b.frame.ptr + (size_t)slot * n; // (then the filter's output, when denoised)
        RT_HIP(hipEventRecord(b.ev_pass_begin[slot], stream));
        // adaptive: pass 0 traces every tile, pass k the list fold k - 1 wrote
        const uint32_t *list = ad && k > 0 ? b.tile_lists.ptr + (size_t)(k & 1) * n_tiles : nullptr;
        const int rc2 = nee ? rtapi::enqueue_nee_pass(s, np, c0, c1, stream, list, running)
                            : rtapi::enqueue_chunks(s, pp, c0, c1, stream, list, running);
        if (rc2 != RT_OK) return rc2;
        RT_HIP(hipEventRecord(b.ev_pass_traced[slot], stream));
        if (k >= slots) RT_HIP(hipStreamWaitEvent(stream, b.ev_copied[slot], 0)); // device slot k % slots held pass k - slots's frame
        // what the decision step of either estimator is told (rtdev::TileDecision): the sums, the pass's frame slot, the
        // tiles' state and lists, and where the pass ends in the chunk plan
        auto decision = [&]() -> rtdev::TileDecision {
            rtdev::TileDecision d;
            memset(&d, 0, sizeof d);
            d.running = b.accum.ptr;
            d.squares = b.squares.ptr;
            d.out = dev;
            d.tile_stop = b.tile_stop.ptr;
            d.tile_scale = b.tile_scale.ptr;
            d.err_prev = b.tile_err.ptr + (size_t)((k + slots - 1) % slots) * n_tiles;
            d.err = b.tile_err.ptr + (size_t)slot * n_tiles;
            d.next_list = ad ? b.tile_lists.ptr + (size_t)((k + 1) & 1) * n_tiles : nullptr;
            d.next_count = b.tile_counts.ptr + k;
            d.width = p->width;
            d.height = p->height;
            d.tiles_x = tiles_x;
            d.n_tiles = (int32_t)n_tiles;
            d.chunks_done = c1;
            d.samples_done = starts[(size_t)c1];
            d.eligible = ad && c1 >= 4 && d.samples_done >= ad->params->min_samples && ad->params->threshold > 0.0;
            d.scale = 1.0 / (double)d.samples_done; // what rtdev_launch_resolve (rt_render_frame_nee) and rtdev_launch_fold_chunks pass
            d.inv_batches = c1 >= 2 ? 1.0 / (double)(c1 - 1) : 0.0;
            d.threshold = ad ? ad->params->threshold : 0.0;
            return d;
        };
        if (nee) { // the sums are where the pass left them: the frame slot and, adaptive, the tiles' decisions
            const rtdev::NeeDecide f = {decision()};
            RT_HIP(s->kernels->nee_decide(&f, stream));
        } else if (ad) {
            rtdev::AdaptiveFold f;
            memset(&f, 0, sizeof f);
            f.d = decision();
            f.partial = b.partial.ptr;
            f.c0 = c0;
            for (size_t c = 0; c + 1 < starts.size(); ++c) f.inv_chunk[c] = 1.0 / (double)(starts[c + 1] - starts[c]);
            RT_HIP(s->kernels->fold_adaptive(&f, stream));
        } else {
            RT_HIP(s->kernels->fold_chunks(b.partial.ptr, b.accum.ptr, dev, n, c0, c1, starts[(size_t)c1], stream));
        }
        if (dn) { // the filter writes the third slot, which copy k - 1 must have read first
            if (k >= 1) RT_HIP(hipStreamWaitEvent(stream, b.ev_copied[slot ^ 1], 0));
            const int rc2 = rtapi::enqueue_denoise(s, p, dn, dev, guides, b.frame.ptr + 2 * n, stream);
            if (rc2 != RT_OK) return rc2;
            dev = b.frame.ptr + 2 * n;
        }
        RT_HIP(hipEventRecord(b.ev_folded[slot], stream));
        RT_HIP(hipStreamWaitEvent(copy, b.ev_folded[slot], 0));
        if (ad) { // the count first: the calling thread enqueues the next pass on it, not on the frame
            RT_HIP(hipMemcpyAsync(b.host_counts.ptr + k, b.tile_counts.ptr + k, sizeof(uint32_t), hipMemcpyDeviceToHost, copy));
            RT_HIP(hipEventRecord(b.ev_counted[slot], copy));
        }
        RT_HIP(hipMemcpyAsync(b.host_frame.ptr + (size_t)slot * n, dev, n * sizeof(double), hipMemcpyDeviceToHost, copy));
        RT_HIP(hipEventRecord(b.ev_copied[slot], copy));
        return RT_OK;
    };
    bool begun = false;
    auto run = [&]() -> int {
        // (fill_args inside refuses what rt_render_frame refuses at this sample count, before anything is enqueued)
        int rc2 = nee ? rtapi::begin_nee_passes(s, camera, p, nee, stream, cancel.armed(), np)
                      : rtapi::begin_passes(s, camera, p, stream, passes, cancel.armed(), pp);
        if (rc2 != RT_OK) return rc2;
        begun = true;
        if (ad && (nee ? np.args.n_tiles : pp.args.n_tiles) != (int)n_tiles)
            return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_adaptive: tile grid mismatch");
        RT_HIP(hipMemsetAsync(b.accum.ptr, 0, n * sizeof(double), stream)); // the running sums start at +0.0
        if (nee) RT_HIP(hipMemsetAsync(b.partial.ptr, 0, n * sizeof(double), stream)); // ... and their copy at the last boundary
        if (n_tiles) { // ... and so do the squares; every tile runs, no tile has been counted
            RT_HIP(hipMemsetAsync(b.squares.ptr, 0, n * sizeof(double), stream));
            RT_HIP(hipMemsetAsync(b.tile_stop.ptr, 0, n_tiles * sizeof(int32_t), stream));
            RT_HIP(hipMemsetAsync(b.tile_counts.ptr, 0, (size_t)passes * sizeof(uint32_t), stream));
        }
        if (dn && (rc2 = rtapi::enqueue_guides(s, camera, p, guides, stream)) != RT_OK) return rc2; // once, before pass 0
        int enqueued = 0;
        for (; enqueued < passes && enqueued < (ad ? 1 : 2); ++enqueued)
            if ((rc2 = enqueue_pass(enqueued)) != RT_OK) return rc2;
        for (int k = 0; k < passes; ++k) {
            const int slot = k % slots;
            if (ad) { // pass k + 1 goes out as soon as it is known to trace something
                if ((rc2 = rtapi::wait_event(b.ev_counted[slot], cancel)) != RT_OK) return rc2;
                running = b.host_counts.ptr[k];
                if (running > 0 && enqueued < passes) {
                    if (cancel.raised()) return RT_ERR_CANCEL_EVENT;
                    if ((rc2 = enqueue_pass(enqueued++)) != RT_OK) return rc2;
                }
            }
            if ((rc2 = rtapi::wait_event(b.ev_copied[slot], cancel)) != RT_OK) return rc2;
            RT_HIP(hipEventSynchronize(b.ev_folded[slot])); // (done: the copy waited for it)
            float ms = 0.f;
            RT_HIP(hipEventElapsedTime(&ms, b.ev_pass_begin[slot], b.ev_pass_traced[slot]));
            kernel_ms += ms;
            RT_HIP(hipEventElapsedTime(&ms, b.ev_pass_traced[slot], b.ev_folded[slot]));
            fold_ms += ms;
            if (cancel.raised()) return RT_ERR_CANCEL_EVENT;
            if (callback) callback(user, b.host_frame.ptr + (size_t)slot * n, starts[(size_t)ends[(size_t)k]], p->samples);
            delivered = k;
            if (ad) {
                if (running == 0) break; // every tile has stopped
            } else if (enqueued < passes) {
                if (cancel.raised()) return RT_ERR_CANCEL_EVENT; // enqueue nothing more
                if ((rc2 = enqueue_pass(enqueued++)) != RT_OK) return rc2;
            }
        }
        return RT_OK;
    };
    rc = run();
    if (!begun) return rc; // nothing was enqueued
    if (rc == RT_ERR_CANCEL_EVENT) { // cpu.rs:55-62: Ok, nothing further delivered; the waves in flight stop at their next item
        rc = rtapi::poison_queue(s);
    }
    // the stats' events behind everything of the call, then both streams drained (on success too: the last copy is done,
    // its fold and launch before it)
    (void)hipEventRecord(b.ev_traced, stream);
    (void)hipEventRecord(b.ev_resolved, stream);
    const hipError_t e1 = hipStreamSynchronize(stream), e2 = hipStreamSynchronize(copy);
    s->summed_times = true;
    s->summed_kernel_ms = kernel_ms;
    s->summed_resolve_ms = fold_ms;
    if (rc == RT_OK && (e1 != hipSuccess || e2 != hipSuccess))
        return fail(RT_ERR_HIP, std::string("rt_render_progressive: stream synchronisation failed: ") +
                                    hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    if (rc != RT_OK || !ad || delivered < 0) return rc;
    // adaptive: the outputs are the state of the last callback.  Its frame and tile errors are in slot `delivered` % 3,
    // which no later pass has written (at most two passes run beyond it); a tile stopped after it ran on to its boundary.
    const int slot = delivered % slots, done = starts[(size_t)ends[(size_t)delivered]];
    memcpy(ad->out_rgb, b.host_frame.ptr + (size_t)slot * n, n * sizeof(double));
    if (ad->out_tile_error)
        RT_HIP(hipMemcpy(ad->out_tile_error, b.tile_err.ptr + (size_t)slot * n_tiles, n_tiles * sizeof(double), hipMemcpyDeviceToHost));
    if (ad->out_samples) {
        std::vector<int32_t> stop(n_tiles);
        RT_HIP(hipMemcpy(stop.data(), b.tile_stop.ptr, n_tiles * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int y = 0; y < p->height; ++y)
            for (int x = 0; x < p->width; ++x) {
                const int32_t t = stop[(size_t)(y / 8) * (size_t)tiles_x + (size_t)(x / 8)];
                ad->out_samples[(size_t)y * (size_t)p->width + (size_t)x] = t != 0 && t <= done ? t : done;
            }
    }
    return RT_OK;
}

} // namespace

extern "C" {

int rt_render_progressive(RtScene *s, const RtCamera *camera, const RtRenderParams *p, int32_t pass_samples,
                          RtFrameCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user) {
    const Cancel c{nullptr, cancelled, cancel_user};
    return rtapi::guarded("rt_render_progressive", [&] { return render_progressive(s, camera, p, pass_samples, callback, user, c); });
}

int rt_render_progressive_denoised(RtScene *s, const RtCamera *camera, const RtRenderParams *p, int32_t pass_samples,
                                   const RtDenoiseParams *denoise, RtFrameCallback callback, void *user, RtCancelCallback cancelled,
                                   void *cancel_user) {
    const Cancel c{nullptr, cancelled, cancel_user};
    return rtapi::guarded("rt_render_progressive_denoised", [&]() -> int {
        const int rc = rtapi::check_denoise(p, denoise); // (before the scene: the filter's refusals need no device)
        if (rc != RT_OK) return rc;
        return render_progressive(s, camera, p, pass_samples, callback, user, c, denoise);
    });
}

void rt_adaptive_params_default(RtAdaptiveParams *out) {
    if (!out) return;
    memset(out, 0, sizeof *out);
    out->threshold = 0.01;
    out->pass_samples = 64;
    out->min_samples = 0;
}

int rt_render_adaptive(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtAdaptiveParams *adaptive,
                       double *out_rgb, int32_t *out_samples, double *out_tile_error, RtFrameCallback callback, void *user,
                       RtCancelCallback cancelled, void *cancel_user) {
    const Cancel c{nullptr, cancelled, cancel_user};
    return rtapi::guarded("rt_render_adaptive", [&]() -> int {
        const int rc = check_adaptive(p, adaptive, out_rgb); // (before the scene: these refusals need no device)
        if (rc != RT_OK) return rc;
        const Adaptive ad{adaptive, out_rgb, out_samples, out_tile_error};
        return render_progressive(s, camera, p, adaptive->pass_samples, callback, user, c, nullptr, &ad);
    });
}

int rt_render_progressive_nee(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *light_sampling,
                              int32_t pass_samples, RtFrameCallback callback, void *user, RtCancelCallback cancelled,
                              void *cancel_user) {
    const Cancel c{nullptr, cancelled, cancel_user};
    return rtapi::guarded("rt_render_progressive_nee", [&]() -> int {
        // (before the scene: these refusals need no device)
        if (pass_samples <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "pass_samples must be positive");
        if (!callback) return fail(RT_ERR_INVALID_ARGUMENT, "callback is NULL");
        const int rc = rtapi::check_nee(s, camera, p, light_sampling, "rt_render_progressive_nee");
        if (rc != RT_OK) return rc;
        return render_progressive(s, camera, p, pass_samples, callback, user, c, nullptr, nullptr, light_sampling);
    });
}

int rt_render_adaptive_nee(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *light_sampling,
                           const RtAdaptiveParams *adaptive, double *out_rgb, int32_t *out_samples, double *out_tile_error,
                           RtFrameCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user) {
    const Cancel c{nullptr, cancelled, cancel_user};
    return rtapi::guarded("rt_render_adaptive_nee", [&]() -> int {
        int rc = check_adaptive(p, adaptive, out_rgb); // (before the scene: these refusals need no device)
        if (rc != RT_OK) return rc;
        if ((rc = rtapi::check_nee(s, camera, p, light_sampling, "rt_render_adaptive_nee")) != RT_OK) return rc;
        const Adaptive ad{adaptive, out_rgb, out_samples, out_tile_error};
        return render_progressive(s, camera, p, adaptive->pass_samples, callback, user, c, nullptr, &ad, light_sampling);
    });
}

int rtdev_progressive_passes(int32_t samples, int32_t pass_samples, int32_t *out, int32_t n_out, int32_t *n_passes) {
    return rtapi::guarded("rtdev_progressive_passes", [&]() -> int {
        if (!n_passes || n_out < 0 || (!out && n_out > 0)) return fail(RT_ERR_INVALID_ARGUMENT, "n_passes/out is NULL or n_out is negative");
        *n_passes = 0;
        if (samples <= 0 || pass_samples <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "samples and pass_samples must be positive");
        const std::vector<int> starts = rtapi::chunk_plan(samples);
        const std::vector<int> ends = pass_ends(starts, pass_samples);
        for (size_t k = 0; k < ends.size() && (int32_t)k < n_out; ++k) out[k] = starts[(size_t)ends[k]];
        *n_passes = (int32_t)ends.size();
        return RT_OK;
    });
}

} // extern "C"
