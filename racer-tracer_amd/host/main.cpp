// main.cpp — `racer-tracer-amd`: headless stand-in for the reference binary
// with the same flags (racer-tracer/src/config.rs:12-28):
//     -c/--config <file.yml>   (default ./config.yml, env CONFIG)
//     -s/--scene  <file.yml|sandbox|random>
//     --image-action <png|none>
// plus --seed, --device and --devices N (the frame is sharded over N GPUs of this
// process the way the reference shards it over its rayon pool, cpu.rs:118-131) and --denoise (the assembled frame goes
// through rt_denoise_frame on the first device before the tone map and the PNG) and --adaptive T (one device renders the
// frame through rt_render_adaptive, a tile stopping once its error is at most T; --denoise filters that frame) and --nee (one
// device renders the frame through rt_render_frame_nee, next-event estimation; --denoise filters that frame) and
// --nee-adaptive T (--adaptive's stop rule with the next-event estimator: rt_render_adaptive_nee) and --nee-stream (--nee's
// frame through rt_render_nee, tile by tile into the screen buffer; the PNG has --nee's bytes) and --nee-devices N (the same
// stream through rt_render_nee_multi, the frame's strips dealt to devices device .. device+N-1) and --temporal K (one device
// renders K frames of the configured sample count at seeds seed .. seed + K - 1 from the configured camera through
// rt_render_temporal and writes the last; --denoise gives the filter its levels, without it the history alone is shown).
// --denoise-variance sends the frame of the default, --nee, --adaptive T or --nee-adaptive T route through
// rt_render_adaptive_filtered instead (threshold 0 where no T is given): the variance-guided filter fed by the batch sums.
// --nee-lights plain|all and --nee-pick uniform|power give every scene of an NEE run its light list (rt_scene_set_lights).
// --preview-upsample renders the config's `preview:` block (scale > 1) through rt_render_preview_upsampled: the scaled preview
// frame upsampled to full resolution with full-resolution guides; --denoise passes the default number of a-trous levels.
// --preview-temporal K renders K frames of the `preview:` block at seeds seed .. seed + K - 1 through rt_render_preview_temporal
// (include/rt_preview_temporal.h): each traces another pixel of its block, all go into one full-resolution history, the last
// is written; --denoise gives the filter its levels.
// --pick X,Y asks the scene, after the run, what lies under pixel (X, Y) of the configured camera (include/rt_rays.h) and
// prints the answer on stdout.
// --pick-through X,Y[,K] asks for the first K primitives under that pixel, in order (include/rt_multihit.h), one line each.
// --visible AX,AY,AZ,BX,BY,BZ asks the scene, after the run, whether the segment between the two points is free
// (include/rt_occlusion.h) and prints yes or no on stdout.
// --ao S[,RADIUS] renders the ambient-occlusion frame of the configured camera (include/rt_ambient.h: rt_render_ambient, S
// hemisphere samples per pixel within RADIUS) in place of the path-traced one; it goes through the tone map and the image action.
// The reference opens a window and renders when R is released (scene_controller/interactive.rs:83-86); this renders the final
// image once and exits, which is what `--image-action png` is for.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rt_host.h"
#include "../../include/rt_preview_temporal.h"
#include "../../include/rt_ambient.h"
#include "../../include/rt_multihit.h"
#include "../../include/rt_occlusion.h"
#include "../../include/rt_rays.h"
#include "config.h"
#include "error.h"

namespace {

struct ScreenBuffer { // image_buffer.rs:104-170: tone-map each tile, keep the frame
    RthSession *session;
    int width, height;
    std::vector<double> buffer;
    std::vector<double> raw; // --denoise, --adaptive: the frame before the tone map
};

void on_tile(void *user, const double *rgb, int32_t r, int32_t c, int32_t w, int32_t h) {
    ScreenBuffer *sb = static_cast<ScreenBuffer *>(user);
    std::vector<double> mapped((size_t)w * (size_t)h * 3);
    rth_tone_map(sb->session, rgb, mapped.data(), (size_t)w * (size_t)h);
    if (!sb->raw.empty())
        for (int row = 0; row < h; ++row)
            memcpy(&sb->raw[((size_t)(r + row) * (size_t)sb->width + (size_t)c) * 3], &rgb[(size_t)row * (size_t)w * 3],
                   (size_t)w * 3 * sizeof(double));
    for (int row = 0; row < h; ++row)
        memcpy(&sb->buffer[((size_t)(r + row) * (size_t)sb->width + (size_t)c) * 3], &mapped[(size_t)row * (size_t)w * 3],
               (size_t)w * 3 * sizeof(double));
}

// --pick X,Y: what lies under the pixel.  The ray is the guides' (rt_render_guides_device): through the pixel's centre, no
// lens offset, at the middle of the shutter interval.  One line on stdout: `pick X Y prim obj_id t px py pz nx ny nz`, or
// `pick X Y miss`.
void pixel_ray(const RtCamera *cam, const RtRenderParams &params, int x, int y, double o[3], double d[3], double &time) {
    const double u = ((double)x + 0.5) / (double)(params.width - 1), v = ((double)y + 0.5) / (double)(params.height - 1);
    for (int k = 0; k < 3; ++k) {
        o[k] = cam->origin[k];
        d[k] = cam->upper_left_corner[k] + u * cam->horizontal[k] - v * cam->vertical[k] - o[k];
    }
    time = (cam->time_a + cam->time_b) * 0.5;
}

int pick_pixel(RtScene *scene, const RtCamera *cam, const RtRenderParams &params, int x, int y) {
    double o[3], d[3], time;
    pixel_ray(cam, params, x, y, o, d, time);
    RtRays rays = {o, d, nullptr, nullptr, &time};
    double t = 0.0, point[3] = {0, 0, 0}, normal[3] = {0, 0, 0};
    int32_t prim = RT_RAY_MISS, obj_id = -1;
    RtRayHits hits = {&t, point, normal, nullptr, &prim, &obj_id, nullptr};
    RtRayQueryParams query;
    rt_ray_query_params_default(&query);
    const int rc = rt_trace_rays(scene, &rays, 1, &query, &hits);
    if (rc != RT_OK) {
        fprintf(stderr, "%s: %s\n", rt_strerror(rc), rt_last_error_message());
        return rc;
    }
    if (prim < 0) printf("pick %d %d miss\n", x, y);
    else
        printf("pick %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", x, y, (int)prim, (int)obj_id, t, point[0], point[1],
               point[2], normal[0], normal[1], normal[2]);
    return RT_OK;
}

// --pick-through X,Y[,K]: the first K primitives under the pixel, along --pick's ray.  One line on stdout per filled slot j:
// `pick-through X Y j prim obj_id t px py pz nx ny nz`, or `pick-through X Y miss` when there is none.
int pick_through(RtScene *scene, const RtCamera *cam, const RtRenderParams &params, int x, int y, int k) {
    double o[3], d[3], time;
    pixel_ray(cam, params, x, y, o, d, time);
    RtRays rays = {o, d, nullptr, nullptr, &time};
    double t[RT_MULTIHIT_MAX], point[3 * RT_MULTIHIT_MAX], normal[3 * RT_MULTIHIT_MAX];
    int32_t prim[RT_MULTIHIT_MAX], obj_id[RT_MULTIHIT_MAX], count = 0;
    RtRayHits hits = {t, point, normal, nullptr, prim, obj_id, nullptr}; // (n = 1: slot j of a plane is its entry j)
    RtMultiHitParams mp;
    rt_multihit_params_default(&mp);
    mp.k = k;
    const int rc = rt_trace_rays_multi(scene, &rays, 1, &mp, &hits, &count);
    if (rc != RT_OK) {
        fprintf(stderr, "%s: %s\n", rt_strerror(rc), rt_last_error_message());
        return rc;
    }
    if (count <= 0) printf("pick-through %d %d miss\n", x, y);
    for (int j = 0; j < count; ++j)
        printf("pick-through %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", x, y, j, (int)prim[j], (int)obj_id[j], t[j],
               point[3 * j], point[3 * j + 1], point[3 * j + 2], normal[3 * j], normal[3 * j + 1], normal[3 * j + 2]);
    return RT_OK;
}

// --visible AX,AY,AZ,BX,BY,BZ: is the segment from a to b free of the scene?  The ray (a, b - a) over the window
// [1e-3, 1 - 1e-3], at time 0.  One line on stdout: `visible ax ay az bx by bz yes` or `... no`.
int visible_between(RtScene *scene, const double ab[6]) {
    const double d[3] = {ab[3] - ab[0], ab[4] - ab[1], ab[5] - ab[2]};
    const double t_min = 1e-3, t_max = 1.0 - 1e-3;
    RtRays rays = {ab, d, &t_min, &t_max, nullptr};
    int32_t occluded = 0;
    const int rc = rt_trace_occlusion(scene, &rays, 1, &occluded);
    if (rc != RT_OK) {
        fprintf(stderr, "%s: %s\n", rt_strerror(rc), rt_last_error_message());
        return rc;
    }
    if (occluded == RT_RAY_INVALID) { // (a == b: the direction is all zeros)
        fprintf(stderr, "--visible: the two points do not span a segment\n");
        return RT_ERR_INVALID_ARGUMENT;
    }
    printf("visible %.17g %.17g %.17g %.17g %.17g %.17g %s\n", ab[0], ab[1], ab[2], ab[3], ab[4], ab[5], occluded ? "no" : "yes");
    return RT_OK;
}

} // namespace

int main(int argc, char **argv) {
    rthost::Args args;
    try {
        args = rthost::Args::parse(argc, argv);
    } catch (const rthost::TracerError &e) {
        fprintf(stderr, "%s\n", e.what());
        return e.code();
    }
    if (args.help) {
        printf("racer-tracer-amd [-c config.yml] [-s scene.yml|sandbox] [--image-action png|none] [--seed N] [--device N] [--devices N] [--denoise] [--denoise-variance] [--adaptive T] [--nee] [--nee-stream] [--nee-devices N] [--nee-adaptive T] [--nee-lights plain|all] [--nee-pick uniform|power] [--temporal K] [--preview-upsample] [--preview-temporal K] [--pick X,Y] [--pick-through X,Y[,K]] [--visible AX,AY,AZ,BX,BY,BZ] [--ao S[,RADIUS]]\n");
        return 0;
    }
    RthSession *session = nullptr;
    const char *action = nullptr;
    if (args.image_action) action = *args.image_action == rthost::ImageActionConfig::SavePng ? "png" : "none";
    int rc = rth_session_open(args.config.c_str(), args.scene ? args.scene->c_str() : nullptr, action, args.seed, &session);
    if (rc != RT_OK) {
        fprintf(stderr, "%s\n", rth_last_error_message());
        return rc;
    }
    RtRenderParams params;
    rth_session_params(session, args.preview_upsample || args.preview_temporal > 0 ? 1 : 0, &params); // ... the `preview:` block
    if (args.devices < 1) {
        fprintf(stderr, "--devices must be at least 1\n");
        rth_session_close(session);
        return RT_ERR_ARGUMENT_PARSING;
    }
    if (args.pick && (args.pick_x >= params.width || args.pick_y >= params.height)) {
        fprintf(stderr, "--pick %d,%d lies outside the %d x %d image\n", args.pick_x, args.pick_y, params.width, params.height);
        rth_session_close(session);
        return RT_ERR_ARGUMENT_PARSING;
    }
    if (args.pick_through && (args.through_x >= params.width || args.through_y >= params.height)) {
        fprintf(stderr, "--pick-through %d,%d lies outside the %d x %d image\n", args.through_x, args.through_y, params.width, params.height);
        rth_session_close(session);
        return RT_ERR_ARGUMENT_PARSING;
    }
    std::vector<RtScene *> scenes;
    auto destroy_scenes = [&] {
        for (RtScene *s : scenes) rt_scene_destroy(s);
    };
    const int n_devices = args.nee_devices > 0 ? args.nee_devices : args.devices;
    for (int k = 0; k < n_devices; ++k) { // one upload of the (tiny) scene per device
        RtScene *scene = nullptr;
        rc = rt_scene_create(rth_session_scene(session), args.device + k, &scene);
        if (rc != RT_OK) {
            fprintf(stderr, "%s: %s\n", rt_strerror(rc), rt_last_error_message());
            destroy_scenes();
            rth_session_close(session);
            return rc;
        }
        scenes.push_back(scene);
        if (args.nee_list_given) { // --nee-lights / --nee-pick: the same list on every scene of the run
            RtLightListParams lp;
            rt_light_list_params_default(&lp);
            lp.kinds = args.nee_lights_all ? RT_LIGHTS_ALL : RT_LIGHTS_PLAIN;
            lp.pick = args.nee_pick_power ? RT_PICK_POWER : RT_PICK_UNIFORM;
            rc = rt_scene_set_lights(scene, &lp);
            if (rc != RT_OK) {
                fprintf(stderr, "%s: %s\n", rt_strerror(rc), rt_last_error_message());
                destroy_scenes();
                rth_session_close(session);
                return rc;
            }
        }
    }
    const size_t n_rgb = (size_t)params.width * (size_t)params.height * 3;
    ScreenBuffer sb{session, params.width, params.height, std::vector<double>(n_rgb, 0.0), std::vector<double>(args.denoise || args.adaptive > 0.0 || args.nee || args.nee_adaptive > 0.0 ? n_rgb : 0, 0.0)};
    fprintf(stderr, "Rendering image...\n"); // interactive.rs:229
    auto t0 = std::chrono::steady_clock::now();
    double traced = 1.0; // --adaptive: the fraction of the frame's samples traced
    double mean_length = 0.0; // --temporal, --preview-temporal: the mean history length behind the last frame
    double filled = 0.0;      // --preview-temporal: the share of pixels with length 0 (filled from the last frame's anchors)
    double mean_sigma = 0.0;  // --denoise-variance: the mean of sqrt(var) over the frame
    if (args.ao > 0) { // the ambient-occlusion frame in the path-traced one's place
        RtAmbientParams ao;
        rt_ambient_params_default(&ao);
        ao.samples = args.ao;
        if (args.ao_radius > 0.0) ao.radius = args.ao_radius;
        ao.seed = params.seed;
        std::vector<double> frame(n_rgb);
        rc = rt_render_ambient(scenes[0], rth_session_camera(session), &params, &ao, frame.data());
        if (rc == RT_OK) rth_tone_map(session, frame.data(), sb.buffer.data(), n_rgb / 3);
    } else if (args.preview_upsample) { // the preview frame, its guides, the upsample and (--denoise) the levels in one call
        RtDenoiseParams dp;
        rt_denoise_params_default(&dp);
        if (!args.denoise) dp.iterations = 0;
        std::vector<double> frame(n_rgb);
        rc = rt_render_preview_upsampled(scenes[0], rth_session_camera(session), &params, &dp, frame.data(), nullptr);
        if (rc == RT_OK) rth_tone_map(session, frame.data(), sb.buffer.data(), n_rgb / 3);
    } else if (args.denoise_variance) { // the adaptive passes (or, with threshold 0, the still frame) and the filter in one call
        RtAdaptiveParams ap;
        rt_adaptive_params_default(&ap);
        ap.threshold = args.adaptive > 0.0 ? args.adaptive : args.nee_adaptive > 0.0 ? args.nee_adaptive : 0.0;
        RtLightSamplingParams ls;
        rt_light_sampling_params_default(&ls);
        RtDenoiseParams dp;
        rt_denoise_params_default(&dp);
        RtVarianceFilterParams fp;
        rt_variance_filter_params_default(&fp);
        std::vector<int32_t> counts(n_rgb / 3);
        std::vector<double> filtered(n_rgb), var(n_rgb / 3);
        RtBatchOutputs outputs;
        memset(&outputs, 0, sizeof outputs);
        outputs.samples = counts.data();
        outputs.variance = var.data();
        rc = rt_render_adaptive_filtered(scenes[0], rth_session_camera(session), &params, args.nee || args.nee_adaptive > 0.0 ? &ls : nullptr,
                                         &ap, &dp, &fp, filtered.data(), &outputs, nullptr, nullptr, nullptr, nullptr);
        double sum = 0.0;
        for (int32_t c : counts) sum += (double)c;
        traced = sum / ((double)counts.size() * (double)params.samples);
        for (double v : var) mean_sigma += std::sqrt(v);
        mean_sigma /= (double)var.size();
        if (rc == RT_OK) rth_tone_map(session, filtered.data(), sb.buffer.data(), n_rgb / 3);
    } else if (args.preview_temporal > 0) { // K jittered preview frames into one full-resolution history; the last one is shown
        RtTemporalParams tp;
        rt_temporal_params_default(&tp);
        RtDenoiseParams dp;
        rt_denoise_params_default(&dp);
        if (!args.denoise) dp.iterations = 0;
        RtTemporal *history = nullptr;
        rc = rt_temporal_create(args.device, params.width, params.height, &history);
        std::vector<double> frame(n_rgb), length(n_rgb / 3);
        RtRenderParams one = params;
        for (int k = 0; rc == RT_OK && k < args.preview_temporal; ++k) {
            one.seed = params.seed + (uint64_t)k; // equal seeds would trace equal samples
            rc = rt_render_preview_temporal(scenes[0], history, rth_session_camera(session), &one, &tp, &dp, k, frame.data(), length.data());
        }
        rt_temporal_destroy(history);
        for (double l : length) {
            mean_length += l;
            if (l == 0.0) filled += 1.0;
        }
        mean_length /= (double)length.size();
        filled /= (double)length.size();
        if (rc == RT_OK) rth_tone_map(session, frame.data(), sb.buffer.data(), n_rgb / 3);
    } else if (args.temporal > 0) { // K frames into one history; the last one, filtered inside the call, is tone-mapped here
        RtTemporalParams tp;
        rt_temporal_params_default(&tp);
        RtDenoiseParams dp;
        rt_denoise_params_default(&dp);
        if (!args.denoise) dp.iterations = 0;
        RtTemporal *history = nullptr;
        rc = rt_temporal_create(args.device, params.width, params.height, &history);
        std::vector<double> frame(n_rgb), length(n_rgb / 3);
        RtRenderParams one = params;
        for (int k = 0; rc == RT_OK && k < args.temporal; ++k) {
            one.seed = params.seed + (uint64_t)k; // equal seeds would trace equal samples
            rc = rt_render_temporal(scenes[0], history, rth_session_camera(session), &one, &tp, &dp, frame.data(), length.data());
        }
        rt_temporal_destroy(history);
        for (double l : length) mean_length += l;
        mean_length /= (double)length.size();
        if (rc == RT_OK) rth_tone_map(session, frame.data(), sb.buffer.data(), n_rgb / 3);
    } else if (args.adaptive > 0.0) { // the whole frame at once; tone-mapped below (after the filter, with --denoise)
        RtAdaptiveParams ap;
        rt_adaptive_params_default(&ap);
        ap.threshold = args.adaptive;
        std::vector<int32_t> counts(n_rgb / 3);
        rc = rt_render_adaptive(scenes[0], rth_session_camera(session), &params, &ap, sb.raw.data(), counts.data(), nullptr, nullptr,
                                nullptr, nullptr, nullptr);
        double sum = 0.0;
        for (int32_t c : counts) sum += (double)c;
        traced = sum / ((double)counts.size() * (double)params.samples);
        if (rc == RT_OK && !args.denoise) rth_tone_map(session, sb.raw.data(), sb.buffer.data(), n_rgb / 3);
    } else if (args.nee_adaptive > 0.0) { // as --adaptive, with the next-event estimator
        RtAdaptiveParams ap;
        rt_adaptive_params_default(&ap);
        ap.threshold = args.nee_adaptive;
        RtLightSamplingParams ls;
        rt_light_sampling_params_default(&ls);
        std::vector<int32_t> counts(n_rgb / 3);
        rc = rt_render_adaptive_nee(scenes[0], rth_session_camera(session), &params, &ls, &ap, sb.raw.data(), counts.data(), nullptr,
                                    nullptr, nullptr, nullptr, nullptr);
        double sum = 0.0;
        for (int32_t c : counts) sum += (double)c;
        traced = sum / ((double)counts.size() * (double)params.samples);
        if (rc == RT_OK && !args.denoise) rth_tone_map(session, sb.raw.data(), sb.buffer.data(), n_rgb / 3);
    } else if (args.nee) { // the whole frame at once; tone-mapped below (after the filter, with --denoise)
        RtLightSamplingParams ls;
        rt_light_sampling_params_default(&ls);
        rc = rt_render_frame_nee(scenes[0], rth_session_camera(session), &params, &ls, sb.raw.data());
        if (rc == RT_OK && !args.denoise) rth_tone_map(session, sb.raw.data(), sb.buffer.data(), n_rgb / 3);
    } else if (args.nee_stream) { // --nee's frame as a tile stream: every finished tile goes through the tone map as it arrives
        RtLightSamplingParams ls;
        rt_light_sampling_params_default(&ls);
        rc = rt_render_nee(scenes[0], rth_session_camera(session), &params, &ls, on_tile, &sb, nullptr, nullptr);
    } else if (args.nee_devices > 0) { // --nee-stream's tiles from every device's strips: a tile column arrives once all have it
        RtLightSamplingParams ls;
        rt_light_sampling_params_default(&ls);
        rc = rt_render_nee_multi(scenes.data(), (int)scenes.size(), rth_session_camera(session), &params, &ls, 0, on_tile, &sb, nullptr,
                                 nullptr);
    } else if (scenes.size() == 1) {
        // the reference's tile stream (cpu.rs:64-70): every finished tile goes through ScreenBuffer::update's tone map;
        // with several devices a tile column arrives once every device has finished its strips of it
        rc = rt_render(scenes[0], rth_session_camera(session), &params, on_tile, &sb, nullptr);
    } else {
        rc = rt_render_multi(scenes.data(), (int)scenes.size(), rth_session_camera(session), &params, 0, on_tile, &sb, nullptr, nullptr);
    }
    if (rc == RT_OK && args.denoise && args.temporal == 0 && !args.denoise_variance && !args.preview_upsample && args.preview_temporal == 0) { // the whole frame, filtered, then tone-mapped like the tiles were
        RtDenoiseParams dp;
        rt_denoise_params_default(&dp);
        std::vector<double> filtered(n_rgb);
        rc = rt_denoise_frame(scenes[0], rth_session_camera(session), &params, &dp, sb.raw.data(), filtered.data());
        if (rc == RT_OK) rth_tone_map(session, filtered.data(), sb.buffer.data(), n_rgb / 3);
    }
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != RT_OK) {
        fprintf(stderr, "%s: %s\n", rt_strerror(rc), rt_last_error_message());
    } else {
        RtRenderStats st{};
        for (RtScene *s : scenes) { // every device's share
            RtRenderStats one;
            rt_scene_last_stats(s, &one);
            st.samples += one.samples;
            st.segments += one.segments;
            st.kernel_ms = one.kernel_ms > st.kernel_ms ? one.kernel_ms : st.kernel_ms;
        }
        if (args.adaptive > 0.0 || args.nee_adaptive > 0.0)
            fprintf(stderr, "Adaptive sampling (threshold %g) traced %.1f %% of the %d samples per pixel.\n",
                    args.adaptive > 0.0 ? args.adaptive : args.nee_adaptive, 100.0 * traced, params.samples);
        if (args.denoise_variance)
            fprintf(stderr, "Variance-guided filter: mean standard error of the luminance %.6f.\n", mean_sigma);
        if (args.temporal > 0)
            fprintf(stderr, "Temporal accumulation over %d frames: mean history length %.2f.\n", args.temporal, mean_length);
        if (args.preview_temporal > 0)
            fprintf(stderr, "Preview accumulation over %d frames: mean history length %.2f, %.1f %% of the pixels with length 0.\n",
                    args.preview_temporal, mean_length, 100.0 * filled);
        fprintf(stderr, "It took %.3f seconds to render the image. (%.1f Msamples/s, %.2f segments/sample, kernel %.1f ms)\n",
                secs, (double)st.samples / secs / 1e6, st.samples ? (double)st.segments / (double)st.samples : 0.0, st.kernel_ms);
        if (rth_session_image_action(session) == RTH_IMAGE_ACTION_SAVE_PNG) { // main.rs:153-156
            char path[4096];
            fprintf(stderr, "Saving image...\n");
            rc = rth_save_png(session, sb.buffer.data(), params.width, params.height, nullptr, path, sizeof path);
            if (rc != RT_OK) fprintf(stderr, "%s\n", rth_last_error_message());
            else if (path[0]) fprintf(stderr, "Saved image to: %s\n", path);
            else fprintf(stderr, "No output directory for saving pngs. Skipping.\n");
        }
    }
    if (rc == RT_OK && args.pick) rc = pick_pixel(scenes[0], rth_session_camera(session), params, args.pick_x, args.pick_y);
    if (rc == RT_OK && args.pick_through)
        rc = pick_through(scenes[0], rth_session_camera(session), params, args.through_x, args.through_y, args.through_k);
    if (rc == RT_OK && args.visible) rc = visible_between(scenes[0], args.visible_ab);
    destroy_scenes();
    rth_session_close(session);
    return rc;
}
