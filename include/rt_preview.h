/* rt_preview.h — the scaled preview frame (RtRenderParams.scale > 1, the reference's CpuRendererScaled) upsampled to
 * full resolution with full-resolution first-hit guides.  Plain C; the types are rt_abi.h's.  DESIGN.md section 4.13 has
 * the definition, tests/upsample_model.py restates it.
 *
 * The preview traces one pixel per step_x x step_y block (the block's top-left pixel, its ANCHOR) and fills the block
 * with it.  The upsample gives every pixel of the W x H frame, the uncovered right and bottom edges included, the blend
 * of the four anchors around it: bilinear weights, times rt_denoise_device's normal and plane stops against the
 * pixel's own full-resolution guides, anchors of another obj_id left out; demodulated by the anchors' albedo and
 * re-modulated by the pixel's own (RT_DENOISE_DEMODULATE), so texture detail comes back at full resolution.  A pixel
 * none of whose anchors qualifies keeps the value of its block's anchor, bit for bit.  Everything is f64.
 *
 * The parameter block is RtDenoiseParams: flags, sigma_normal and sigma_plane drive the upsample (the plane stop's
 * distance unit is sigma_plane * max(step_x, step_y) pixel footprints); iterations and sigma_color are read by
 * rt_render_preview_upsampled's a-trous levels only.
 *
 * Refused with RT_ERR_INVALID_ARGUMENT before a device is touched: NULL pointers and incomplete guides, scale <= 1,
 * strip_count > 1, rgb_device == out_device, and what rt_denoise_device refuses about `denoise`.  RT_ERR_UNSUPPORTED for
 * rt_render_preview_upsampled on a scene of the v1 kernel, which has no preview mode.
 * A binding detects these entry points by symbol lookup (RT_ABI_VERSION is unchanged by them). */
#ifndef RT_PREVIEW_H
#define RT_PREVIEW_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The preview's grid for these params, without a device: step = the largest divisor <= scale of width / max(tiles_w, 1)
 * (rows likewise), cover = (size / step) * step.  scale <= 1 gives 1, 1, W, H.  Refuses what rt_render_frame refuses
 * about width, height, scale and strips. */
int rt_preview_grid(const RtRenderParams *params, int32_t *step_x, int32_t *step_y, int32_t *cover_w, int32_t *cover_h);

/* Upsample rgb_device — what rt_render_frame_device wrote for these params (scale > 1) — with the full-resolution guides
 * of the same camera (rt_render_guides_device with the same params and scale = 0) into out_device (W*H*3 f64), enqueued
 * on `hip_stream` (NULL = default stream) without synchronising. */
int rt_upsample_preview_device(RtScene *scene, const RtRenderParams *params, const RtDenoiseParams *denoise,
                               const double *rgb_device, const RtGuides *guides_device, double *out_device,
                               void *hip_stream);

/* Host-memory convenience, synchronous.  In order: the preview frame on the device, the guides, the upsample, then
 * denoise->iterations levels of rt_denoise_device on the result when > 0, then the download into out_rgb_host (W*H*3);
 * the replicated preview frame goes into out_preview_host when it is not NULL.  Device memory is the scene's.
 * rt_scene_last_stats afterwards reports the preview render's samples and segments. */
int rt_render_preview_upsampled(RtScene *scene, const RtCamera *camera, const RtRenderParams *params,
                                const RtDenoiseParams *denoise, double *out_rgb_host,
                                double *out_preview_host /* may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* RT_PREVIEW_H */
