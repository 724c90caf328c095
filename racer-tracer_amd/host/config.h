// config.h — Config / Args of racer-tracer (racer-tracer/src/config.rs), same
// keys, same precedence (CLI over file, config.rs:30-67).
#pragma once
#include <optional>
#include <string>
#include "vec3.h"
#include "yaml.h"

namespace rthost {

struct ScreenConfig { // config.rs:69-73
    size_t height = 0, width = 0;
};

struct RenderConfig { // config.rs:75-82
    size_t samples = 0, max_depth = 0, num_threads_width = 0, num_threads_height = 0, scale = 0;
};

struct SceneLoaderConfig { // config.rs:84-93
    enum Kind { None, Yml, Random, Sandbox } kind = None;
    std::string path;
};

enum class ImageActionConfig { None, SavePng }; // config.rs:95-100

// config.rs:108-113 plus the one new variant a GPU backend adds
enum class RendererConfig { Cpu, CpuPreview, Hip };

struct ToneMapConfig { // config.rs:136-167
    enum Kind { None, Reinhard, Hable, Aces } kind = None;
    std::optional<double> max_white;
    std::optional<double> shoulder_strength, linear_strength, linear_angle, toe_strength, toe_numerator,
        toe_denominator, exposure_bias, linear_white_point;
    std::optional<std::array<Vec3, 3>> input_matrix, output_matrix;
};

struct CameraConfig { // config.rs:169-178
    std::optional<double> vfov, aperture, focus_distance;
    std::optional<Vec3> pos, look_at;
    std::optional<double> speed, sensitivity;
};

struct Config { // config.rs:180-214
    RenderConfig preview, render;
    ScreenConfig screen;
    SceneLoaderConfig loader;
    ImageActionConfig image_action = ImageActionConfig::None;
    std::optional<std::string> image_output_dir;
    RendererConfig renderer = RendererConfig::Hip;
    RendererConfig preview_renderer = RendererConfig::CpuPreview;
    CameraConfig camera;
    ToneMapConfig tone_map;

    static Config from_file(const std::string &file); // config.rs:216-225
};

struct Args { // config.rs:12-28
    std::string config = "./config.yml"; // -c/--config, env CONFIG
    std::optional<std::string> scene;    // -s/--scene <file.yml|random|sandbox>
    std::optional<ImageActionConfig> image_action; // --image-action <png|none>
    // additive (the reference has no headless mode and no seed):
    uint64_t seed = 1;
    int device = 0;
    int devices = 1; // --devices N: render the frame on devices device .. device+N-1 (rt_render_frame_multi)
    bool denoise = false; // --denoise: filter the assembled frame (rt_denoise_frame) before tone map and PNG
    bool nee = false; // --nee: one device renders the frame through rt_render_frame_nee (next-event estimation)
    bool nee_stream = false; // --nee-stream: the same frame through rt_render_nee, tile by tile into the screen buffer, one device only
    int nee_devices = 0; // --nee-devices N (N >= 1): --nee-stream's frame through rt_render_nee_multi on devices device .. device+N-1
    double adaptive = 0.0; // --adaptive T (T > 0): render through rt_render_adaptive with threshold T, one device only
    // --nee-lights plain|all and --nee-pick uniform|power: rt_scene_set_lights on every scene the run creates (an NEE mode only)
    bool nee_lights_all = false, nee_pick_power = false, nee_list_given = false;
    double nee_adaptive = 0.0; // --nee-adaptive T (T > 0): render through rt_render_adaptive_nee with threshold T, one device only
    int temporal = 0; // --temporal K (K >= 1): K frames at seeds seed .. seed + K - 1 through rt_render_temporal, the last one written; one device only
    // --denoise-variance: the frame of the default, --nee, --adaptive T or --nee-adaptive T route through
    // rt_render_adaptive_filtered (threshold 0 where no T is given), filtered by its batch variance; one device only
    bool denoise_variance = false;
    // --preview-upsample: the config's `preview:` block through rt_render_preview_upsampled (include/rt_preview.h): the scaled
    // preview frame upsampled with full-resolution guides; --denoise adds the default a-trous levels; one device only
    bool preview_upsample = false;
    // --preview-temporal K (K >= 1): K frames of the `preview:` block at seeds seed .. seed + K - 1 and the phases of frames
    // 0 .. K - 1 through rt_render_preview_temporal (include/rt_preview_temporal.h) into one history, the last one written;
    // --denoise gives the filter its levels; one device only
    int preview_temporal = 0;
    // --pick X,Y: after the run, the guides' ray of that pixel of the configured camera and image (its centre, pinhole, the
    // middle of the shutter) through rt_trace_rays (include/rt_rays.h), one line on stdout; a pixel outside the image is refused
    bool pick = false;
    int pick_x = 0, pick_y = 0;
    // --pick-through X,Y[,K]: after the run, the first K (1..RT_MULTIHIT_MAX = 8, default 4) primitives along that same ray
    // through rt_trace_rays_multi (include/rt_multihit.h), one line per hit on stdout; refused like --pick
    bool pick_through = false;
    int through_x = 0, through_y = 0, through_k = 4;
    // --visible AX,AY,AZ,BX,BY,BZ: after the run, whether the segment from a to b is free of the scene, through
    // rt_trace_occlusion (include/rt_occlusion.h) with the window [1e-3, 1 - 1e-3], one line on stdout; six finite numbers
    bool visible = false;
    double visible_ab[6] = {0, 0, 0, 0, 0, 0};
    // --ao S[,RADIUS]: the ambient-occlusion frame of the configured camera (rt_render_ambient, include/rt_ambient.h) in
    // place of the path-traced one: S samples per pixel, a power of two in 1..1024, and a radius > 0 (default: none)
    int ao = 0;
    double ao_radius = 0.0; // 0: the default, +inf
    bool help = false;

    static Args parse(int argc, const char *const *argv);
};

ImageActionConfig image_action_from_str(const std::string &s); // config.rs:119-129
Config config_try_from(const Args &args);                      // config.rs:30-67

// Shared YAML -> value helpers (also used by the scene loader).
double yaml_f64(const YamlNode &n, const std::string &file, const std::string &what);
Vec3 yaml_vec3(const YamlNode &n, const std::string &file, const std::string &what);
Vec3 yaml_vec3_flat(const YamlNode &parent, const std::string &file, const std::string &what);
CameraConfig yaml_camera(const YamlNode &n, const std::string &file);
ToneMapConfig yaml_tone_map(const YamlNode &n, const std::string &file);
// Externally tagged enum: "Name" (unit) or {Name: body}.  Returns the variant
// name; *body is the payload or nullptr.
std::string yaml_variant(const YamlNode &n, const YamlNode **body, const std::string &file,
                         const std::string &what);

} // namespace rthost
