// rt_temporal_state.h — the RtTemporal object behind include/rt_abi.h's opaque handle and the layout of its planes, for the
// two units that render into one: rt_temporal.hip (rt_render_temporal) and rt_preview_temporal.hip
// (rt_render_preview_temporal).  Below them, what rt_temporal.hip's host side lends the second unit: its checks, the fill of
// an argument block's history fields and the one body of the two whole-frame calls.  Private to the library.
#pragma once
#include "rt_scene.h"

#include <cstring>
#include <functional>

struct RtTemporal {
    int device = 0;
    int width = 0, height = 0;
    rtapi::DevBuf<double> planes; // two histories of 12 doubles per pixel, the guides' 10, the frame's 3 and the output's 3
    rtapi::DevBuf<int32_t> ids;   // the histories' and the guides' obj_id
    rtapi::PinnedBuf<double> host_length; // W*H
    bool has_prev = false;
    int current = 0; // the history the next frame reads
    RtCamera camera;
    ~RtTemporal() { (void)hipSetDevice(device); } // the owners above free themselves behind this, on their device
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

// What the two accumulating kernels' argument blocks (AccumulateArgs, PreviewAccumulateArgs; the block zeroed by the
// caller) say about the previous camera, where there is one, and about `temporal`.
template <class Args> void fill_history_args(Args &a, const RtTemporalParams *t, const RtCamera *prev_camera) {
    a.has_prev = prev_camera != nullptr; // (check_accumulate_buffers: with prev_history or not at all)
    if (prev_camera) {
        memcpy(a.o, prev_camera->origin, sizeof a.o);
        memcpy(a.ulc, prev_camera->upper_left_corner, sizeof a.ulc);
        memcpy(a.hor, prev_camera->horizontal, sizeof a.hor);
        memcpy(a.ver, prev_camera->vertical, sizeof a.ver);
    }
    a.alpha = t->alpha;
    a.alpha_moments = t->alpha_moments;
    a.max_history = t->max_history;
    a.normal_tol2 = t->normal_tolerance * t->normal_tolerance;
    a.plane_tol = t->plane_tolerance;
}

// One frame into an RtTemporal, for rt_render_temporal and rt_render_preview_temporal, each after its refusals about its
// parameters.  Refused here, in this order: out_rgb NULL, the state NULL or of another size, the scene NULL or on another
// device, a v1-kernel scene (with `v1_message`).  Then on the scene's stream: the frame of `render_camera` and `p` into the
// state, the guides of `camera` and `full` (params at full resolution, which the filter's levels take too), `accumulate`
// from the state's current history and stored camera (both NULL on its first frame) into the other one,
// enqueue_denoise_history, the downloads (out_length may be NULL); after the synchronise the histories are swapped and
// `camera` is stored.
using EnqueueAccumulate = std::function<int(const double *frame, const RtGuides *g, const RtCamera *prev_camera,
                                            const RtHistory *prev, const RtHistory *out, hipStream_t stream)>;
int render_into_state(RtScene *s, RtTemporal *t, const char *v1_message, const RtCamera *camera, const RtCamera *render_camera,
                      const RtRenderParams *p, const RtRenderParams *full, const RtTemporalParams *tp, const RtDenoiseParams *d,
                      const EnqueueAccumulate &accumulate, double *out_rgb, double *out_length);

} // namespace rtapi
