// rt_progressive.hip — rt_render_progressive: the whole frame handed to the caller once per pass while it converges, the
// last pass's frame being rt_render_frame's.
//
// The reference's author wanted this shape: renderer/denoised.rs:291-331 renders the frame in passes and writes a
// whole-frame BufferUpdate after each (:210-216).  Here a pass is a run of whole chunks of the frame's chunk plan (rt_api.hip:
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
// Host code only.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "rt_scene.h"

using rtapi::Cancel;
using rtapi::fail;

namespace {

// Pass k ends at chunk boundary ends[k] (an index into chunk_starts): the first boundary at least pass_samples beyond the
// one it starts at, or the end of the frame.
std::vector<int> pass_ends(const std::vector<int> &starts, int pass_samples) {
    const int total = (int)starts.size() - 1;
    std::vector<int> ends;
    for (int c = 0; c < total;) {
        int e = c + 1;
        while (e < total && starts[(size_t)e] - starts[(size_t)c] < pass_samples) ++e;
        ends.push_back(e);
        c = e;
    }
    return ends;
}

// Everything the call needs, allocated before its first launch (a hipMalloc between passes would wait for the running
// kernels): slices, one item counter per pass, the running sums, two device and two pinned frame slots, the copy stream and
// the events of the two slots.
int reserve_passes(RtScene *s, const RtRenderParams *p, int passes, size_t n) {
    int rc = rtapi::reserve_render_buffers(s, p, false);
    if (rc != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    if (b.queue.count < (size_t)passes) RT_HIP(b.queue.alloc((size_t)passes));
    if (b.accum.count < n) RT_HIP(b.accum.alloc(n));
    if (b.frame.count < 2 * n) RT_HIP(b.frame.alloc(2 * n));
    if ((rc = rtapi::ensure_host_frame(s, 2 * n)) != RT_OK) return rc;
    if (!b.stream_copy) RT_HIP(hipStreamCreateWithFlags(&b.stream_copy, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) {
        if (!b.ev_pass_begin[k]) RT_HIP(hipEventCreate(&b.ev_pass_begin[k]));
        if (!b.ev_pass_traced[k]) RT_HIP(hipEventCreate(&b.ev_pass_traced[k]));
        if (!b.ev_folded[k]) RT_HIP(hipEventCreate(&b.ev_folded[k]));
        if (!b.ev_copied[k]) RT_HIP(hipEventCreateWithFlags(&b.ev_copied[k], hipEventDisableTiming));
    }
    return RT_OK;
}

// dn: the filter of rt_render_progressive_denoised, or NULL
int render_progressive(RtScene *s, const RtCamera *camera, const RtRenderParams *p, int pass_samples, RtFrameCallback callback,
                       void *user, const Cancel &cancel, const RtDenoiseParams *dn = nullptr) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (!callback) return fail(RT_ERR_INVALID_ARGUMENT, "callback is NULL");
    if (pass_samples <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "pass_samples must be positive");
    int rc = rtapi::check_params(camera, p);
    if (rc != RT_OK) return rc;
    if (p->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "progressive frames are whole frames: params->strip_* is not supported here");
    if (p->scale > 1) return fail(RT_ERR_INVALID_ARGUMENT, "progressive frames are full-resolution frames: params->scale must be 0 or 1");
    if (dn && (rc = rtapi::check_denoise(p, dn)) != RT_OK) return rc;
    if (s->use_v1) return fail(RT_ERR_UNSUPPORTED, "rt_render_progressive needs the pooled kernel (the v1 kernel has no sample chunks)");
    if (cancel.raised()) return RT_ERR_CANCEL_EVENT; // cpu.rs:82-85, as rt_render_ex
    RT_HIP(hipSetDevice(s->device));
    const std::vector<int> starts = rtapi::chunk_starts(p->samples);
    const std::vector<int> ends = pass_ends(starts, pass_samples);
    const int passes = (int)ends.size();
    const size_t n = (size_t)p->width * (size_t)p->height * 3; // a frame, and a slice (whole-frame slices: slice_rows = height)
    if ((rc = reserve_passes(s, p, passes, n)) != RT_OK) return rc;
    rtapi::RenderBuffers &b = s->buf;
    // denoised: the guides, the filter's scratch and a third device frame slot, the filter's output
    if (dn && (rc = rtapi::reserve_denoise(s, n / 3, true)) != RT_OK) return rc;
    if (dn && b.frame.count < 3 * n) RT_HIP(b.frame.alloc(3 * n));
    const RtGuides guides = dn ? rtapi::scene_guides(s, n / 3) : RtGuides();
    const hipStream_t stream = b.stream, copy = b.stream_copy;
    rtapi::PoolPasses pp;
    double kernel_ms = 0.0, fold_ms = 0.0;

    auto enqueue_pass = [&](int k) -> int {
        const int slot = k & 1, c0 = k > 0 ? ends[(size_t)k - 1] : 0, c1 = ends[(size_t)k];
        double *dev = b.frame.ptr + (size_t)slot * n; // (then the filter's output, when denoised)
        RT_HIP(hipEventRecord(b.ev_pass_begin[slot], stream));
        const int rc2 = rtapi::enqueue_chunks(s, pp, c0, c1, stream);
        if (rc2 != RT_OK) return rc2;
        RT_HIP(hipEventRecord(b.ev_pass_traced[slot], stream));
        if (k >= 2) RT_HIP(hipStreamWaitEvent(stream, b.ev_copied[slot], 0)); // device slot k % 2 held pass k - 2's frame
        RT_HIP(s->kernels->fold_chunks(b.partial.ptr, b.accum.ptr, dev, n, c0, c1, starts[(size_t)c1], stream));
        if (dn) { // the filter writes the third slot, which copy k - 1 must have read first
            if (k >= 1) RT_HIP(hipStreamWaitEvent(stream, b.ev_copied[slot ^ 1], 0));
            const int rc2 = rtapi::enqueue_denoise(s, p, dn, dev, guides, b.frame.ptr + 2 * n, stream);
            if (rc2 != RT_OK) return rc2;
            dev = b.frame.ptr + 2 * n;
        }
        RT_HIP(hipEventRecord(b.ev_folded[slot], stream));
        RT_HIP(hipStreamWaitEvent(copy, b.ev_folded[slot], 0));
        RT_HIP(hipMemcpyAsync(b.host_frame + (size_t)slot * n, dev, n * sizeof(double), hipMemcpyDeviceToHost, copy));
        RT_HIP(hipEventRecord(b.ev_copied[slot], copy));
        return RT_OK;
    };
    bool begun = false;
    auto run = [&]() -> int {
        // (fill_args inside refuses what rt_render_frame refuses at this sample count, before anything is enqueued)
        int rc2 = rtapi::begin_passes(s, camera, p, stream, passes, cancel.armed(), pp);
        if (rc2 != RT_OK) return rc2;
        begun = true;
        RT_HIP(hipMemsetAsync(b.accum.ptr, 0, n * sizeof(double), stream)); // the running sums start at +0.0
        if (dn && (rc2 = rtapi::enqueue_guides(s, camera, p, guides, stream)) != RT_OK) return rc2; // once, before pass 0
        int enqueued = 0;
        for (; enqueued < passes && enqueued < 2; ++enqueued)
            if ((rc2 = enqueue_pass(enqueued)) != RT_OK) return rc2;
        for (int k = 0; k < passes; ++k) {
            const int slot = k & 1;
            if ((rc2 = rtapi::wait_event(b.ev_copied[slot], cancel)) != RT_OK) return rc2;
            RT_HIP(hipEventSynchronize(b.ev_folded[slot])); // (done: the copy waited for it)
            float ms = 0.f;
            RT_HIP(hipEventElapsedTime(&ms, b.ev_pass_begin[slot], b.ev_pass_traced[slot]));
            kernel_ms += ms;
            RT_HIP(hipEventElapsedTime(&ms, b.ev_pass_traced[slot], b.ev_folded[slot]));
            fold_ms += ms;
            if (cancel.raised()) return RT_ERR_CANCEL_EVENT;
            callback(user, b.host_frame + (size_t)slot * n, starts[(size_t)ends[(size_t)k]], p->samples);
            if (enqueued < passes) {
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
    return rc;
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

int rtdev_progressive_passes(int32_t samples, int32_t pass_samples, int32_t *out, int32_t n_out, int32_t *n_passes) {
    return rtapi::guarded("rtdev_progressive_passes", [&]() -> int {
        if (!n_passes || n_out < 0 || (!out && n_out > 0)) return fail(RT_ERR_INVALID_ARGUMENT, "n_passes/out is NULL or n_out is negative");
        *n_passes = 0;
        if (samples <= 0 || pass_samples <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "samples and pass_samples must be positive");
        const std::vector<int> starts = rtapi::chunk_starts(samples);
        const std::vector<int> ends = pass_ends(starts, pass_samples);
        for (size_t k = 0; k < ends.size() && (int32_t)k < n_out; ++k) out[k] = starts[(size_t)ends[k]];
        *n_passes = (int32_t)ends.size();
        return RT_OK;
    });
}

} // extern "C"
