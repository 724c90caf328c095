// rt_temporal_state.h — the RtTemporal object behind include/rt_abi.h's opaque handle and the layout of its planes, for the
// two units that render into one: rt_temporal.hip (rt_render_temporal) and rt_preview_temporal.hip
// (rt_render_preview_temporal).  Below them, what rt_temporal.hip's host side lends the second unit.  Private to the library.
#pragma once
#include "rt_scene.h"

struct RtTemporal {
    int device = 0;
    int width = 0, height = 0;
    rtapi::DevBuf<double> planes; // two histories of 12 doubles per pixel, the guides' 10, the frame's 3 and the output's 3
    rtapi::DevBuf<int32_t> ids;   // the histories' and the guides' obj_id
    double *host_length = nullptr; // pinned, W*H
    bool has_prev = false;
    int current = 0; // the history the next frame reads
    RtCamera camera;
};

namespace rtapi {

// the planes of an RtTemporal: [history 0 | history 1 | guides | frame | output]
constexpr size_t kHistoryDoubles = 12, kStateDoubles = 2 * kHistoryDoubles + 10 + 3 + 3;

inline RtHistory state_history(RtTemporal *t, int k) {
    const size_t pixels = (size_t)t->width * (size_t)t->height;
    double *base = t->planes.ptr + (size_t)k * kHistoryDoubles * pixels;
    RtHistory h;
    h.radiance = base;
    h.moments = base + 3 * pixels;
    h.length = base + 5 * pixels;
    h.normal = base + 6 * pixels;
    h.position = base + 9 * pixels;
    h.obj_id = t->ids.ptr + (size_t)k * pixels;
    return h;
}

inline RtGuides state_guides(RtTemporal *t) {
    const size_t pixels = (size_t)t->width * (size_t)t->height;
    double *base = t->planes.ptr + 2 * kHistoryDoubles * pixels;
    RtGuides g;
    g.normal = base;
    g.position = base + 3 * pixels;
    g.albedo = base + 6 * pixels;
    g.footprint = base + 9 * pixels;
    g.obj_id = t->ids.ptr + 2 * pixels;
    return g;
}

// the traced frame (W*H*3); the filtered output lies W*H*3 doubles behind it
inline double *state_frame(RtTemporal *t) {
    return t->planes.ptr + (2 * kHistoryDoubles + 10) * (size_t)t->width * (size_t)t->height;
}

// rt_temporal.hip.  check_temporal: what every temporal entry point refuses about an RtTemporalParams.
// check_accumulate_buffers: what rt_temporal_accumulate_device refuses about its frame, guides and histories — NULLs, an
// incomplete plane set, prev_camera without prev_history or the reverse, out_history sharing a plane with prev_history.
// enqueue_denoise_history: rt_denoise_history_device's launches (arguments checked by the caller).
int check_temporal(const RtTemporalParams *t);
int check_accumulate_buffers(const double *rgb, const RtGuides *g, const RtCamera *prev_camera, const RtHistory *prev,
                             const RtHistory *out);
int enqueue_denoise_history(RtScene *s, const RtRenderParams *p, const RtDenoiseParams *d, const RtTemporalParams *t,
                            const RtHistory *h, const RtGuides *g, double *out, hipStream_t stream);

} // namespace rtapi
