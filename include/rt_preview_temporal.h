/* rt_preview_temporal.h — jittered preview frames accumulated into a full-resolution history.  Plain C; the types are
 * rt_abi.h's, the grid is rt_preview.h's.  DESIGN.md section 4.14 has the definition, tests/preview_temporal_model.py
 * restates it.
 *
 * The scaled preview (RtRenderParams.scale > 1) traces one pixel per step_x x step_y block.  Here that pixel moves from
 * frame to frame — the PHASE (jx, jy), 0 <= jx < step_x, 0 <= jy < step_y, a camera shift on the host — and every frame
 * is accumulated at full resolution through rt_temporal_accumulate_device's re-projection: a pixel the frame sampled
 * blends its sample into its history (or starts afresh), a pixel it did not sample carries its re-projected history
 * unchanged, and a pixel with neither is FILLED with rt_upsample_preview_device's blend of the four anchors around it and
 * gets length 0.  A tap of length 0 is never read as history, so no interpolated colour is fed back.  After
 * step_x * step_y frames of a still camera every covered pixel holds a sample of its own, at the preview's cost per
 * frame.  The history is an ordinary RtHistory in an ordinary RtTemporal: calls of rt_render_preview_temporal and
 * rt_render_temporal may alternate on one state.
 *
 * Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: NULL pointers and incomplete guides or histories, what
 * rt_upsample_preview_device refuses about `params` and `denoise`, what rt_temporal_accumulate_device refuses about
 * `temporal`, the prev_* pair and aliasing, a phase outside the grid, frame_index < 0, a state of another size or device.
 * RT_ERR_UNSUPPORTED for rt_render_preview_temporal on a scene of the v1 kernel, which has no preview mode.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
#ifndef RT_PREVIEW_TEMPORAL_H
#define RT_PREVIEW_TEMPORAL_H

#include "rt_preview.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The phase of frame `frame_index` (>= 0) for these params, without a device: with n = step_x * step_y and g the smallest
 * integer >= max(1, (5 n + 4) / 8) coprime to n, i = ((frame_index mod n) * g) mod n, jx = i mod step_x, jy = i / step_x.
 * Every pixel of the block once per n frames; frame 0 has phase (0, 0).  Refuses what rt_preview_grid refuses. */
int rt_preview_phase(const RtRenderParams *params, int64_t frame_index, int32_t *jx, int32_t *jy);

/* `camera` with upper_left_corner += (jx / (W - 1)) horizontal - (jy / (H - 1)) vertical into `out` (which may be
 * `camera`): rendered with these params, the anchor of block (i, j) traces the rays of the full-resolution pixel
 * (i step_x + jx, j step_y + jy).  Phase (0, 0) copies the camera bit for bit. */
int rt_preview_phase_camera(const RtCamera *camera, const RtRenderParams *params, int32_t jx, int32_t jy, RtCamera *out);

/* One accumulation, enqueued on `hip_stream` (NULL = default stream) without synchronising.  rgb_device: what
 * rt_render_frame_device wrote for `params` (scale > 1) and the phase camera of (jx, jy).  guides_device: the
 * full-resolution guides of the UNSHIFTED camera (rt_render_guides_device, the same params with scale = 0).
 * prev_camera (unshifted) and prev_history: both NULL for a first frame.  out_history receives all six planes. */
int rt_preview_accumulate_device(RtScene *scene, const RtRenderParams *params, const RtTemporalParams *temporal,
                                 const RtDenoiseParams *denoise, int32_t jx, int32_t jy, const double *rgb_device,
                                 const RtGuides *guides_device, const RtCamera *prev_camera, const RtHistory *prev_history,
                                 const RtHistory *out_history, void *hip_stream);

/* Host-memory convenience, synchronous, on the scene's stream.  In order: the phase of frame_index and its camera, the
 * preview frame with that camera, the guides at scale 0 with the caller's camera, the accumulation against the state's
 * history and stored camera, rt_denoise_history_device, the download into out_rgb_host (W*H*3) and, when it is not NULL,
 * of the history length into out_length_host (W*H); then the state's histories are swapped and the caller's camera is
 * stored.  The caller advances params->seed from frame to frame.  rt_scene_last_stats afterwards reports the preview
 * render's samples and segments. */
int rt_render_preview_temporal(RtScene *scene, RtTemporal *temporal_state, const RtCamera *camera, const RtRenderParams *params,
                               const RtTemporalParams *temporal, const RtDenoiseParams *denoise, int64_t frame_index,
                               double *out_rgb_host, double *out_length_host /* may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* RT_PREVIEW_TEMPORAL_H */
