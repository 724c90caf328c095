// rt_deliver.hip — the entry points that hand finished pixels to the HOST: rt_render_frame, rt_render /
// rt_render_ex (the reference's tile stream), their several-device forms rt_render_frame_multi / rt_render_multi, and
// rt_render_nee (the tile stream of the next-event estimator) with its several-device forms
// rt_render_frame_nee_multi / rt_render_nee_multi.
//
// What the reference does here: CpuRenderer::render shards the frame into tiles, every tile is traced on a rayon
// worker and sent to the writer the moment it is finished (racer-tracer/src/renderer/cpu.rs:64-70,118-131), with
// do_cancel polled per tile row (cpu.rs:55, renderer.rs:25-30).
//
// Here ONE persistent launch per device renders the whole frame (its share of it with several devices) and
// DELIVERS ITS OWN PIXELS (rt_device_types.h: TraceArgs.deliver_out): the items are queued region by region — a
// region is a tile column of the stream, or a band of rows of a whole-frame call — the wave that completes the last
// sample chunk of an 8x8 item tile sums the tile's slices and writes sqrt(sum / samples) straight into pinned host
// memory (mapped into every device, laid out so that a tile of the stream is one contiguous run), and the wave that
// completes a region publishes it in a host-visible flag.  The calling thread only polls flags, runs the callbacks
// (or copies finished bands into the caller's frame) while the GPU works on the next region, and polls the cancel
// hook.  No resolve launch, no copy engine, no second stream: nothing has to find a free compute unit beside the
// persistent grid, which is what the round-2 form (ten windowed launches on two streams + a strided copy per column)
// paid 15 % of the frame for.  Pixels are bit-identical to the two-pass path (same slices, same sum order).
//
// Host code only.  What a call launches, waits for and copies is planned without a device (rt_plan.h: TileGrid,
// frame_bands, stream_windows, copy_runs); this file holds what needs the runtime.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>
#include "rt_scene.h"

using rtapi::Cancel;
using rtapi::Delivery;
using rtapi::ensure_host_frame;
using rtapi::fail;

// Pinned frame + flags of the call live on shares[0]'s scene.
int rtapi::ensure_host_frame(RtScene *s, size_t doubles) {
    if (s->buf.host_frame.count >= doubles) return RT_OK; // (the device is made current only where the frame grows)
    RT_HIP(hipSetDevice(s->device));
    RT_HIP(s->buf.host_frame.reserve(doubles, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
    return RT_OK;
}

namespace {

// One device's part of a delivering call.
struct Share {
    RtScene *scene = nullptr;
    RtRenderParams params;
    Delivery delivery;
    int next_region = 0; // regions [0, next_region) have been seen published
    bool launched = false;
};

// Blocks until region `r` of `sh` has been published.  RT_ERR_CANCEL_EVENT when the hook is raised first.
int wait_region(Share &sh, int r, const Cancel &cancel) {
    RtScene *s = sh.scene;
    const volatile unsigned int *flags = s->buf.host_flags.ptr;
    const uint32_t serial = sh.delivery.serial;
    for (unsigned spins = 1;; ++spins) {
        if (flags[r] == serial) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return RT_OK;
        }
        if (cancel.raised()) return RT_ERR_CANCEL_EVENT;
        if ((spins & 127u) == 0) { // has the launch ended (or failed) without publishing?
            (void)hipSetDevice(s->device);
            const hipError_t e = hipEventQuery(s->buf.ev_traced);
            if (e == hipSuccess) {
                if (flags[r] == serial) continue;
                return fail(RT_ERR_HIP, "the launch ended without publishing region " + std::to_string(r));
            }
            if (e != hipErrorNotReady) return fail(RT_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
            (void)hipGetLastError();
        }
        if (spins < 64u) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// Ends everything in flight (cancel or error) and leaves the scenes reusable.
void abort_shares(std::vector<Share> &shares) {
    for (Share &sh : shares) // every share's poison is on its way before any of them is waited for
        if (sh.launched) (void)rtapi::poison_queue_begin(sh.scene);
    for (Share &sh : shares)
        if (sh.launched) {
            (void)hipSetDevice(sh.scene->device);
            (void)hipStreamSynchronize(sh.scene->buf.stream_ctl);
            (void)hipStreamSynchronize(sh.scene->buf.stream);
        }
    (void)hipGetLastError();
}

int finish_shares(std::vector<Share> &shares) {
    int rc = RT_OK;
    for (Share &sh : shares) {
        if (!sh.launched) continue;
        if (hipSetDevice(sh.scene->device) != hipSuccess || hipStreamSynchronize(sh.scene->buf.stream) != hipSuccess) {
            if (rc == RT_OK) rc = fail(RT_ERR_HIP, "stream synchronisation failed");
        } else {
            sh.scene->buf.deliver_dirty = false; // every region was published: the counters are back at zero
        }
    }
    return rc;
}

// shares[i].params: the caller's parameters for one scene, strips dealt out for several
int make_shares(RtScene *const *scenes, int n, const RtRenderParams *p, int strip_rows, std::vector<Share> &shares) {
    std::vector<RtRenderParams> params(1, *p);
    if (n > 1) {
        const int rc = rtapi::deal_strips(p, n, strip_rows, params);
        if (rc != RT_OK) return rc;
    }
    shares.assign((size_t)n, Share());
    for (int i = 0; i < n; ++i) {
        shares[(size_t)i].scene = scenes[i];
        shares[(size_t)i].params = params[(size_t)i];
    }
    return RT_OK;
}

int launch_shares(std::vector<Share> &shares, const RtCamera *camera, bool cancellable = false) {
    for (Share &sh : shares) { // every allocation of the call before its first launch (rt_api.hip: reserve_render_buffers)
        if (sh.delivery.regions.empty()) continue;
        const int rc = sh.delivery.nee ? rtapi::reserve_nee_buffers(sh.scene, &sh.params, true) : rtapi::reserve_render_buffers(sh.scene, &sh.params, true);
        if (rc != RT_OK) return rc;
    }
    for (Share &sh : shares) {
        sh.delivery.cancellable = cancellable;
        // A share that owns no rows (more shares than strips: height 16 over three scenes; a strip_index whose first
        // strip lies below the image) has nothing to launch and nothing to wait for: it counts as published, and the
        // rows of the frame stay as they are — what the two-pass path does with n_items == 0.  (The NEE calls promise such a
        // share's statistics: those of an empty call.)
        if (sh.delivery.regions.empty()) {
            if (sh.delivery.nee) {
                const int rc = rtapi::note_idle_share(sh.scene, sh.scene->buf.stream);
                if (rc != RT_OK) return rc;
            }
            continue;
        }
        sh.delivery.serial = ++sh.scene->buf.deliver_serial;
        if (sh.delivery.serial == 0) sh.delivery.serial = ++sh.scene->buf.deliver_serial; // 0 is the flags' idle value
        const int rc = sh.delivery.nee ? rtapi::enqueue_nee_stream(sh.scene, camera, &sh.params, sh.delivery.nee, sh.delivery)
                                       : rtapi::enqueue_render(sh.scene, camera, &sh.params, nullptr, sh.scene->buf.stream, 0, Cancel(), &sh.delivery);
        if (rc != RT_OK) return rc;
        sh.launched = true;
    }
    return RT_OK;
}

// ------------------------------------------------------------------------------------------------ whole frames
// Regions = bands of tile rows (rt_plan.h: frame_bands); the calling thread copies a band's rows from the pinned frame
// into the caller's (pageable) frame while the GPU renders the next band, so only the last band's copy is exposed.
// nee: NULL, or rt_render_frame_nee_multi's light sampling — the same bands from k_nee_stream_f64's launch, whose item is a
// whole tile: the bands change nothing in its queue (tile rows top to bottom either way), so it gets as many as fit.
int deliver_frame(RtScene *const *scenes, int n, const RtCamera *camera, const RtRenderParams *p, int strip_rows,
                  double *out_rgb, const RtLightSamplingParams *nee = nullptr) {
    std::vector<Share> shares;
    int rc = make_shares(scenes, n, p, strip_rows, shares);
    if (rc != RT_OK) return rc;
    const size_t row_doubles = (size_t)p->width * 3;
    rc = ensure_host_frame(scenes[0], row_doubles * (size_t)p->height);
    if (rc != RT_OK) return rc;
    size_t most_bands = 0;
    for (Share &sh : shares) {
        sh.delivery.regions = rtapi::frame_bands(rtapi::tiles_across(rtapi::owned_rows_of(&sh.params)), rtapi::tiles_across(p->width),
                                                 nee ? rtdev::RT_MAX_REGIONS : rtapi::chunk_count(sh.params.samples));
        sh.delivery.out = scenes[0]->buf.host_frame.ptr;
        sh.delivery.col_step = p->width;
        sh.delivery.cols = 1;
        sh.delivery.nee = nee;
        most_bands = std::max(most_bands, sh.delivery.regions.size());
    }
    rc = launch_shares(shares, camera);
    for (size_t b = 0; b < most_bands && rc == RT_OK; ++b)
        for (Share &sh : shares) {
            if (b >= sh.delivery.regions.size()) continue;
            rc = wait_region(sh, (int)b, Cancel());
            if (rc != RT_OK) break;
            for (const rtapi::RowRun &run : rtapi::copy_runs(&sh.params, sh.delivery.regions[b], p->height))
                memcpy(out_rgb + (size_t)run.image_row * row_doubles, scenes[0]->buf.host_frame.ptr + (size_t)run.image_row * row_doubles,
                       (size_t)run.rows * row_doubles * sizeof(double));
        }
    if (rc != RT_OK) {
        abort_shares(shares);
        return rc;
    }
    return finish_shares(shares);
}

// ------------------------------------------------------------------------------------------------- tile stream
// One callback per tile of tile column `ws` of the grid, top to bottom; `col` is that column as [height][w][3], so a
// tile is a contiguous run of it.  The hook is polled before every tile; true: it cut the column short.  An empty tile —
// more tile rows than image rows, more tile columns than pixels — is still ONE BufferUpdate, as in the reference, whose
// raytrace sends the buffer of every SubImage, empty or not (cpu.rs:64-70).
bool emit_column(const rtapi::TileGrid &grid, int ws, const double *col, RtTileCallback callback, void *user, const Cancel &cancel) {
    const rtapi::TileGrid::Span x = grid.column(ws);
    for (int hs = 0; hs < grid.tiles_h; ++hs) {
        if (cancel.raised()) return true;
        const rtapi::TileGrid::Span y = grid.row(hs);
        callback(user, col + (size_t)y.at * (size_t)x.size * 3, y.at, x.at, x.size, y.size);
    }
    return false;
}

// Regions = windows of tile columns (rt_plan.h: stream_windows).  The pinned frame holds tile column ws as
// [height][w][3] behind the columns before it, and a column goes out as soon as every share has published its window.
// nee: NULL, or rt_render_nee's / rt_render_nee_multi's light sampling — the same stream from k_nee_stream_f64's launches
int deliver_tiles(RtScene *const *scenes, int n, const RtCamera *camera, const RtRenderParams *p, int strip_rows,
                  RtTileCallback callback, void *user, const Cancel &cancel, const RtLightSamplingParams *nee = nullptr) {
    std::vector<Share> shares;
    int rc = make_shares(scenes, n, p, strip_rows, shares);
    if (rc != RT_OK) return rc;
    const rtapi::TileGrid grid(p->width, p->height, p->tiles_w, p->tiles_h);
    rc = ensure_host_frame(scenes[0], (size_t)p->width * (size_t)p->height * 3);
    if (rc != RT_OK) return rc;
    const double *frame = scenes[0]->buf.host_frame.ptr;
    const std::vector<int> columns_after = rtapi::stream_windows(p->width, p->tiles_w, rtapi::tiles_across(p->height)).columns_after;
    if (columns_after.empty()) return fail(RT_ERR_INVALID_ARGUMENT, "empty frame");
    for (Share &sh : shares) {
        sh.delivery.regions = rtapi::stream_windows(p->width, p->tiles_w, rtapi::tiles_across(rtapi::owned_rows_of(&sh.params))).regions;
        sh.delivery.out = scenes[0]->buf.host_frame.ptr;
        sh.delivery.col_step = grid.width_step;
        sh.delivery.cols = p->tiles_w;
        sh.delivery.nee = nee;
    }
    rc = launch_shares(shares, camera, cancel.armed());
    bool cancelled = false;
    int emitted = 0;
    for (size_t r = 0; r < columns_after.size() && rc == RT_OK && !cancelled; ++r) {
        for (Share &sh : shares) {
            if (!sh.launched) continue; // owns no rows
            rc = wait_region(sh, (int)r, cancel);
            if (rc != RT_OK) break;
        }
        if (rc != RT_OK) break;
        for (; emitted < columns_after[r] && !cancelled; ++emitted)
            cancelled = emit_column(grid, emitted, frame + (size_t)p->height * (size_t)grid.column(emitted).at * 3, callback, user, cancel);
    }
    if (rc == RT_ERR_CANCEL_EVENT) {
        cancelled = true;
        rc = RT_OK;
    }
    if (rc != RT_OK || cancelled) { // cpu.rs:55-62: a cancelled render returns Ok(()), nothing further is written
        abort_shares(shares);
        return rc;
    }
    return finish_shares(shares);
}

// The two-pass path behind the tile stream where the delivering launch does not apply (preview scale, the v1 kernel, a
// tile grid wider than the image): the tiles are cut from the finished frame.  The pooled kernel's resolve pass writes
// the stream's tile-column layout itself (k_resolve_chunks_f64), ONE copy brings the frame into the scene's pinned
// buffer and the callbacks read it in place — the reference's interactive mode renders a preview on every camera move
// (interactive.rs:196-267), so what this path costs beyond the 0.5 ms of device work is the frame rate of the window
// (1080p preview: 14.3 ms with a pageable frame, a zero-initialised staging vector and a host-side repack; now 1.44).
// The v1 kernel is traced in sample batches with a synchronisation after each, so that the hook is polled about as
// often as the reference polls it per tile row (cpu.rs:55), and its plain frame is repacked per column on the host.
int tiles_from_frame(RtScene *s, const RtCamera *camera, const RtRenderParams *p, RtTileCallback callback, void *user,
                     const Cancel &cancel) {
    const size_t n = (size_t)p->width * (size_t)p->height * 3;
    RT_HIP(s->buf.frame.reserve(n));
    int rc = ensure_host_frame(s, n);
    if (rc != RT_OK) return rc;
    int batch = 0;
    if (cancel.armed() && s->use_v1) { // at most 32 launches, at least 16 samples each
        batch = (p->samples + 31) / 32;
        if (batch < 16) batch = 16;
        if (batch > p->samples) batch = p->samples;
    }
    const rtapi::TileGrid grid(p->width, p->height, p->tiles_w, p->tiles_h);
    const bool column_layout = !s->use_v1 && grid.width_step > 0 && p->tiles_w > 1; // written by the resolve pass itself
    rc = rtapi::enqueue_render(s, camera, p, s->buf.frame.ptr, s->buf.stream, batch, cancel, nullptr, column_layout ? grid.width_step : 0,
                               column_layout ? p->tiles_w : 1);
    hipEvent_t copied = s->buf.ev_resolved; // re-recorded behind the copy: rt_scene_last_stats reads ev_traced -> ev_resolved (+ the copy)
    if (rc == RT_OK) {
        hipError_t e = hipMemcpyAsync(s->buf.host_frame.ptr, s->buf.frame.ptr, n * sizeof(double), hipMemcpyDeviceToHost, s->buf.stream);
        if (e == hipSuccess) e = hipEventRecord(copied, s->buf.stream);
        if (e != hipSuccess) { // the kernels are in flight on the scene's buffers: drain before the error goes up
            (void)hipStreamSynchronize(s->buf.stream);
            return fail(RT_ERR_HIP, std::string("tiles_from_frame: ") + hipGetErrorString(e));
        }
    }
    if (rc == RT_OK) rc = rtapi::wait_event(copied, cancel);
    if (rc == RT_ERR_CANCEL_EVENT) { // cpu.rs:55-62: return Ok, no tile written
        rc = s->use_v1 ? RT_OK : rtapi::poison_queue(s);
        (void)hipStreamSynchronize(s->buf.stream);
        return rc;
    }
    if (rc != RT_OK) {
        (void)hipStreamSynchronize(s->buf.stream);
        return rc;
    }
    RT_HIP(hipStreamSynchronize(s->buf.stream));
    std::vector<double> column; // v1 / single-column grids: one column of the plain frame, repacked
    for (int ws = 0; ws < p->tiles_w; ++ws) {
        const int x = grid.column(ws).at, w = grid.column(ws).size;
        const double *col;
        if (column_layout) {
            col = s->buf.host_frame.ptr + (size_t)p->height * (size_t)x * 3;
        } else if (w == p->width || w == 0) {
            col = s->buf.host_frame.ptr; // (w == 0: an empty tile column — more tile columns than pixels — reads nothing)
        } else {
            column.resize((size_t)w * (size_t)p->height * 3);
            for (int r = 0; r < p->height; ++r)
                memcpy(&column[(size_t)r * w * 3], s->buf.host_frame.ptr + ((size_t)r * p->width + x) * 3, (size_t)w * 3 * sizeof(double));
            col = column.data();
        }
        if (emit_column(grid, ws, col, callback, user, cancel)) return RT_OK;
    }
    return RT_OK;
}

// rt_render_frame where the delivering launch does not apply (the v1 kernel, the preview scale): resolve kernel + one copy
int frame_two_pass(RtScene *s, const RtCamera *camera, const RtRenderParams *p, double *out_rgb) {
    const size_t n = (size_t)p->width * (size_t)p->height * 3;
    RT_HIP(s->buf.frame.reserve(n));
    int rc = rtapi::enqueue_render(s, camera, p, s->buf.frame.ptr, s->buf.stream, 0, Cancel());
    if (rc != RT_OK) {
        (void)hipStreamSynchronize(s->buf.stream);
        return rc;
    }
    RT_HIP(hipStreamSynchronize(s->buf.stream));
    if (p->strip_count > 1) { // the owned rows only; the rest of out_rgb stays untouched
        const size_t row_bytes = (size_t)p->width * 3 * sizeof(double);
        for (int r = 0; r < p->height; ++r)
            if ((r / p->strip_rows) % p->strip_count == p->strip_index)
                RT_HIP(hipMemcpy(out_rgb + (size_t)r * p->width * 3, s->buf.frame.ptr + (size_t)r * p->width * 3, row_bytes, hipMemcpyDeviceToHost));
    } else {
        RT_HIP(hipMemcpy(out_rgb, s->buf.frame.ptr, n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

// rt_render_nee / rt_render_nee_multi: render_tiles with rt_render_frame_nee's estimator, over the shares of `n` scenes.  The
// delivering launch is k_nee_stream_f64's, one per share (the NEE kernels are their own: a scene made with RT_KERNEL_V1
// streams too); where it does not apply — a tile grid wider than the image — ONE scene's frame is rt_render_frame_nee's
// launch and the tiles are cut from it on the host, the hook being looked at before the launch and before every tile;
// several scenes have no such route (as rt_render_multi has none for its non-delivering ones).
int render_tiles_nee(RtScene *const *scenes, int n, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *ls,
                     int strip_rows, RtTileCallback callback, void *user, const Cancel &cancel, const char *what) {
    if (!callback) return fail(RT_ERR_INVALID_ARGUMENT, "callback is NULL");
    int rc = rtapi::check_nee_shares(scenes, n, camera, p, ls, strip_rows, what);
    if (rc != RT_OK) return rc;
    if (p->tiles_w <= 0 || p->tiles_h <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "tile grid must be positive");
    if ((rc = rtapi::check_same_light_lists(scenes, n, what)) != RT_OK) return rc;
    if (cancel.raised()) return RT_ERR_CANCEL_EVENT; // cpu.rs:82-85
    if (p->width / p->tiles_w > 0) return deliver_tiles(scenes, n, camera, p, strip_rows, callback, user, cancel, ls);
    if (n > 1) return fail(RT_ERR_UNSUPPORTED, std::string(what) + ": a tile grid wider than the image renders on one device");
    RtScene *s = scenes[0];
    RT_HIP(hipSetDevice(s->device));
    std::vector<double> frame((size_t)p->width * (size_t)p->height * 3);
    if ((rc = rtapi::nee_frame_to_host(s, camera, p, ls, frame.data())) != RT_OK) return rc;
    const rtapi::TileGrid grid(p->width, p->height, p->tiles_w, p->tiles_h);
    for (int ws = 0; ws < p->tiles_w; ++ws) // width_step == 0: empty columns, the last one is the whole frame
        if (emit_column(grid, ws, frame.data(), callback, user, cancel)) return RT_OK; // cpu.rs:55-62
    return RT_OK;
}

int render_tiles(RtScene *const *scenes, int n, const RtCamera *camera, const RtRenderParams *p, int strip_rows,
                 RtTileCallback callback, void *user, const Cancel &cancel) {
    int rc = rtapi::check_scenes(scenes, n);
    if (rc != RT_OK) return rc;
    if (!callback) return fail(RT_ERR_INVALID_ARGUMENT, "callback is NULL");
    rc = rtapi::check_params(camera, p);
    if (rc != RT_OK) return rc;
    if (p->tiles_w <= 0 || p->tiles_h <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "tile grid must be positive");
    if (p->strip_count > 1) // a tile of the stream is a finished piece of the frame; row ownership is for rt_render_frame*
        return fail(RT_ERR_INVALID_ARGUMENT, "the tile stream delivers whole tiles: params->strip_* is not supported here");
    if (cancel.raised()) return RT_ERR_CANCEL_EVENT; // cpu.rs:82-85: prepare_threads fails with CancelEvent
    bool delivering = p->scale <= 1 && p->width / p->tiles_w > 0;
    for (int i = 0; i < n; ++i) delivering = delivering && !scenes[i]->use_v1;
    if (delivering) return deliver_tiles(scenes, n, camera, p, strip_rows, callback, user, cancel);
    if (n > 1) return fail(RT_ERR_UNSUPPORTED, "rt_render_multi: the preview scale and the v1 kernel render on one device");
    RT_HIP(hipSetDevice(scenes[0]->device));
    return tiles_from_frame(scenes[0], camera, p, callback, user, cancel);
}

} // namespace

int rtapi::check_scenes(RtScene *const *scenes, int n) {
    if (!scenes || n <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "no scenes");
    for (int i = 0; i < n; ++i)
        if (!scenes[i]) return fail(RT_ERR_INVALID_ARGUMENT, "scenes[" + std::to_string(i) + "] is NULL");
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (scenes[i] == scenes[j]) return fail(RT_ERR_INVALID_ARGUMENT, "the same RtScene is listed twice (create one per share)");
    return RT_OK;
}

// What the several-scene NEE calls refuse before a device is touched: what check_nee refuses about camera, params and light
// sampling (strips of the caller's own and the preview scale included), then the scene list and a negative strip height
int rtapi::check_nee_shares(RtScene *const *scenes, int n, const RtCamera *camera, const RtRenderParams *p,
                            const RtLightSamplingParams *ls, int strip_rows, const char *what) {
    int rc = rtapi::check_nee_args(camera, p, ls, what);
    if (rc != RT_OK) return rc;
    if ((rc = rtapi::check_scenes(scenes, n)) != RT_OK) return rc;
    if (strip_rows < 0) return fail(RT_ERR_INVALID_ARGUMENT, "strip_rows must not be negative");
    return rtapi::check_params(camera, p);
}

// The shares of one NEE frame sample one light list (rt_scene_set_lights).  The only refusal that READS a scene: an entry
// point asks it last, behind every refusal about its other arguments, and still before a device is touched.
int rtapi::check_same_light_lists(RtScene *const *scenes, int n, const char *what) {
    for (int i = 1; i < n; ++i)
        if (scenes[i]->light_params.kinds != scenes[0]->light_params.kinds || scenes[i]->light_params.pick != scenes[0]->light_params.pick)
            return fail(RT_ERR_INVALID_ARGUMENT, std::string(what) + ": the scenes do not carry the same light list params");
    return RT_OK;
}

extern "C" {

int rt_render_frame(RtScene *s, const RtCamera *camera, const RtRenderParams *p, double *out_rgb) {
    return rtapi::guarded("rt_render_frame", [&] {
        if (!s || !out_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "scene/out is NULL");
        int rc = rtapi::check_params(camera, p);
        if (rc != RT_OK) return rc;
        RT_HIP(hipSetDevice(s->device));
        if (s->use_v1 || p->scale > 1) return frame_two_pass(s, camera, p, out_rgb);
        RtScene *scenes[1] = {s};
        return deliver_frame(scenes, 1, camera, p, 0, out_rgb);
    });
}

int rt_render_frame_multi(RtScene *const *scenes, int n_scenes, const RtCamera *camera, const RtRenderParams *params,
                          int strip_rows, double *out_rgb) {
    return rtapi::guarded("rt_render_frame_multi", [&] {
        int rc = rtapi::check_scenes(scenes, n_scenes);
        if (rc != RT_OK) return rc;
        if (!out_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
        rc = rtapi::check_params(camera, params);
        if (rc != RT_OK) return rc;
        if (params->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "params->strip_* must be unset: the call assigns strips itself");
        if (params->scale > 1) return fail(RT_ERR_INVALID_ARGUMENT, "the preview scale cannot be combined with strips");
        for (int i = 0; i < n_scenes; ++i)
            if (scenes[i]->use_v1) return fail(RT_ERR_UNSUPPORTED, "rt_render_frame_multi needs the pooled kernel");
        return deliver_frame(scenes, n_scenes, camera, params, strip_rows, out_rgb);
    });
}

int rt_render(RtScene *s, const RtCamera *camera, const RtRenderParams *p, RtTileCallback callback, void *user,
              const volatile int *cancel) {
    RtScene *scenes[1] = {s};
    return rtapi::guarded("rt_render", [&] { return render_tiles(scenes, 1, camera, p, 0, callback, user, Cancel{cancel}); });
}

int rt_render_ex(RtScene *s, const RtCamera *camera, const RtRenderParams *p, RtTileCallback callback, void *user,
                 RtCancelCallback cancelled, void *cancel_user) {
    RtScene *scenes[1] = {s};
    return rtapi::guarded("rt_render_ex",
                          [&] { return render_tiles(scenes, 1, camera, p, 0, callback, user, Cancel{nullptr, cancelled, cancel_user}); });
}

int rt_render_nee(RtScene *s, const RtCamera *camera, const RtRenderParams *p, const RtLightSamplingParams *light_sampling,
                  RtTileCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user) {
    RtScene *scenes[1] = {s};
    return rtapi::guarded("rt_render_nee", [&] {
        if (!callback) return fail(RT_ERR_INVALID_ARGUMENT, "callback is NULL");
        const int rc = rtapi::check_nee(s, camera, p, light_sampling, "rt_render_nee"); // (one scene: the refusal names it, not a list)
        if (rc != RT_OK) return rc;
        return render_tiles_nee(scenes, 1, camera, p, light_sampling, 0, callback, user, Cancel{nullptr, cancelled, cancel_user}, "rt_render_nee");
    });
}

int rt_render_nee_multi(RtScene *const *scenes, int n_scenes, const RtCamera *camera, const RtRenderParams *p,
                        const RtLightSamplingParams *light_sampling, int strip_rows, RtTileCallback callback, void *user,
                        RtCancelCallback cancelled, void *cancel_user) {
    const Cancel c{nullptr, cancelled, cancel_user};
    return rtapi::guarded("rt_render_nee_multi", [&] {
        return render_tiles_nee(scenes, n_scenes, camera, p, light_sampling, strip_rows, callback, user, c, "rt_render_nee_multi");
    });
}

int rt_render_frame_nee_multi(RtScene *const *scenes, int n_scenes, const RtCamera *camera, const RtRenderParams *p,
                              const RtLightSamplingParams *light_sampling, int strip_rows, double *out_rgb) {
    return rtapi::guarded("rt_render_frame_nee_multi", [&] {
        int rc = rtapi::check_nee_shares(scenes, n_scenes, camera, p, light_sampling, strip_rows, "rt_render_frame_nee_multi");
        if (rc != RT_OK) return rc;
        if (!out_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgb is NULL");
        if ((rc = rtapi::check_same_light_lists(scenes, n_scenes, "rt_render_frame_nee_multi")) != RT_OK) return rc;
        return deliver_frame(scenes, n_scenes, camera, p, strip_rows, out_rgb, light_sampling);
    });
}

int rt_render_multi(RtScene *const *scenes, int n_scenes, const RtCamera *camera, const RtRenderParams *p, int strip_rows,
                    RtTileCallback callback, void *user, RtCancelCallback cancelled, void *cancel_user) {
    const Cancel c{nullptr, cancelled, cancel_user};
    return rtapi::guarded("rt_render_multi", [&] { return render_tiles(scenes, n_scenes, camera, p, strip_rows, callback, user, c); });
}

} // extern "C"
