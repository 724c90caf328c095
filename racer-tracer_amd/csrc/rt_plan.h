// rt_plan.h — the rules that turn a scene description and render parameters into plain numbers and tables: what a
// description may hold, which kernel it selects, its radiance bound, the device records and their order, the light list,
// the sample chunks and launches of a render, its pixel grid and strips, the regions, tiles and copies of a delivering
// call.  Nothing here needs a device or the runtime, and nothing takes an RtScene: rt_scene_create.hip, rt_api.hip and
// rt_deliver.hip upload, enqueue and wait for what these functions return, and tests/plan_driver.cpp runs them as they
// are.  Private to the library.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/rt_abi.h"
#include "rt_device_types.h"
#include "rt_bvh.h"
#include "rt_primary_bounds.h"
#include "rt_error.h"

namespace rtapi {

// ------------------------------------------------------------------------------------------------------------ a scene
// The linear loop costs ~35 VALU instructions per primitive with scalar loads and
// no divergence; the BVH walk ~25 node visits plus leaf tests with per-lane loads.
// They cross at a few dozen primitives (clown.yml, 23 spheres, is still linear).
constexpr int kBvhThreshold = 48;
constexpr size_t kBvhLdsBytes = 32 * 1024;       // a node array up to this size is staged in dynamic LDS
constexpr size_t kLinearTableBytes = 120 * 1024; // the linear-loop variants keep the whole primitive table in LDS
constexpr int kMaxLights = 64;                   // listed lights of a scene (RtLightSamplingParams.max_lights)

// What rt_scene_create refuses about a description, with the error code and text of each refusal.
int validate_desc(const RtSceneDesc *d);
// The options as given, or all zero; refused when a field is out of range.
int check_options(const RtSceneOptions *options, RtSceneOptions &opt);

// Which trace-kernel instantiation a (validated) description needs: the primitive class (rtdev::PRIMS_*: untransformed rects
// only, untransformed spheres only, anything), whether some material reads a texture that is not a plain SolidColor (a
// Dielectric reads none), whether some material is Metal or Dielectric, and whether a MovingSphere is present.
struct Selection {
    int prims_class, textured, specular, has_moving;
};
Selection select_variant(const RtSceneDesc *d);

// What a finished sample can be at most (RtScene.radiance_bound), or 0: the scene has no bound (rt_plan.cpp).
double scene_radiance_bound(const RtSceneDesc *d);

// The union of the primitives' bounds (rt_bvh.h: primitive_bounds; a NaN bound stays: it turns the primary-ray cull off);
// empty (mn > mx) for a scene without primitives.
void scene_bounds(const RtSceneDesc *d, double mn[3], double mx[3]);

// The device records of the primitives, each carrying its material (the only device copy of a material).
std::vector<rtdev::Prim> pack_prims(const RtSceneDesc *d);
// The device records of the textures; an image texture embeds its image's record (rt_device_types.h).
std::vector<rtdev::Texture> pack_textures(const RtSceneDesc *d, const std::vector<rtdev::Image> &images);
// The Perlin tables as they are; `identity` is cleared when some permutation is not the identity.
std::vector<rtdev::Perlin> pack_perlins(const RtSceneDesc *d, int &identity);

// Linear loop: group the table (rt_device_types.h: rect_end, sphere_end, box_end); the order inside a group is kept.
// `order` (the description index of each record) is permuted alongside.  Returns where the groups end.
struct LinearGroups {
    int rect_end[3], sphere_end, box_end;
};
LinearGroups group_linear_table(std::vector<rtdev::Prim> &prims, std::vector<int32_t> &order);

// The compact records the walk tests leaves with (rt_device_types.h: LeafGeo), of a table in leaf order; the first
// MovingSphere with a finite interval sets the scene-wide one (TraceArgs.leaf_time_a, leaf_inv_dt).
struct LeafTable {
    std::vector<rtdev::LeafGeo> geo;
    double time_a = 0.0, inv_dt = 1.0;
};
LeafTable leaf_geometry(const std::vector<rtdev::Prim> &prims);

// Next-event estimation: the listed lights as description indices, in description order (at most max_lights), and what
// rtdev::NeeArgs reads: the light slot of every device primitive (-1: none) and the device primitive of every light.
// order[j] is the description index of device primitive j.
struct LightTables {
    std::vector<int32_t> lights, slot, prim;
};
LightTables light_tables(const RtSceneDesc *d, const std::vector<int32_t> &order, int max_lights);

// The extended list (rt_scene_set_lights, include/rt_abi.h).  What a scene keeps on the host about each primitive to list
// its lights again: kind, flags, geometry, whether its material is DiffuseLight, that material's texture kind and colour.
struct LightFact {
    int32_t kind, flags, emitter, tex_kind;
    double p[6];
    double color[3];
};
std::vector<LightFact> light_facts(const RtSceneDesc *d);
// What the list params may hold: kinds in 0..7, a known pick, _reserved all zero.
int check_light_list_params(const RtLightListParams *p);
// The listed primitives of a `kinds` mask (RtLightKinds) in table order, at most max_lights; mask 0 is light_tables' rule.
std::vector<int32_t> list_lights(const std::vector<LightFact> &facts, int kinds, int max_lights);
// ... as light_tables' three arrays for a device table in `order`.
LightTables light_tables_of(const std::vector<int32_t> &lights, const std::vector<int32_t> &order);
// Does the NEE kernel of today sample this listed light?  (An unwrapped Sphere or rect.)
bool light_is_plain(const LightFact &f);
// w = A L of a listed light: the object-frame surface area times the largest colour component of a SolidColor emitter
// (negative or not finite: 0), else 1.
double light_weight(const LightFact &f);
// The pick among the first n listed lights: p_k and the running sums cdf_k (cdf_{n-1} = 1), formed in f64 in table order.
// RT_PICK_UNIFORM, or a sum of weights that is not positive and finite: p_k = 1 / n, `uniform` set, cdf_k = (k + 1) / n
// (not read by the device, which keeps min(floor(e0 n), n - 1)).
struct LightPick {
    std::vector<double> p, cdf;
    bool uniform = true;
};
LightPick light_pick(const std::vector<LightFact> &facts, const std::vector<int32_t> &lights, int n, int pick);

// ----------------------------------------------------------------------------------------------------------- a render
int check_params(const RtCamera *camera, const RtRenderParams *p);

// Sample chunks a frame of `samples` samples per pixel is cut into, a function of spp only: the start sample of every
// chunk plus the total (chunks + 1 entries; rt_plan.cpp).
std::vector<int> chunk_plan(int samples);
inline int chunk_count(int samples) { return (int)chunk_plan(samples).size() - 1; }
// ... in a render's argument block: chunk_start[], total_chunks, chunk_samples.
void set_chunk_table(rtdev::TraceArgs &a, const std::vector<int> &starts);

// The exponent e of the fixed-point sums (sum_scale = 2^(52-e)) for a radiance bound and a sample count, or 0: f64 sums.
int sum_exponent(double bound, int samples, int *e_out);

// One launch of the pooled kernel: chunks [first_chunk, first_chunk + n_chunks) of every tile.
struct Launch {
    int first_chunk, n_chunks;
};
// Sample batches are cut on chunk boundaries (chunk_plan), so batching changes no sum.
std::vector<Launch> plan_launches(const std::vector<int> &starts, int batch);

// Pass k ends at chunk boundary ends[k] (an index into chunk_plan): the first boundary at least pass_samples beyond the
// one it starts at, or the end of the frame.
std::vector<int> pass_ends(const std::vector<int> &starts, int pass_samples);

// The preview's coarser grid (cpu_scaled.rs:18-41): step = the largest divisor <= scale of width / max(tiles_w, 1), rows
// likewise; cover = (size / step) * step.  scale <= 1: steps of 1 and the whole image.
struct PreviewGrid {
    int step_x, step_y, cover_w, cover_h;
};
PreviewGrid preview_grid(const RtRenderParams *p);
// The pixel of its block that frame `frame_index` (>= 0) of a jittered preview traces: with
// n = step_x step_y and g the smallest integer >= max(1, (5 n + 4) / 8) coprime to n, i = (frame_index mod n) g mod n,
// jx = i mod step_x, jy = i / step_x.  A permutation of the block per n frames that starts at (0, 0).
struct PreviewPhase {
    int jx, jy;
};
PreviewPhase preview_phase(const PreviewGrid &g, int64_t frame_index);
// `camera` with upper_left_corner += (jx / (W - 1)) horizontal - (jy / (H - 1)) vertical, per component as written: the
// anchor of block (i, j) then traces the rays of pixel (i step_x + jx, j step_y + jy).  (0, 0): the camera bit for bit.
RtCamera preview_phase_camera(const RtCamera &camera, int width, int height, int jx, int jy);
// The render's pixel grid: sizes, samples, strips, the preview's coarser grid (preview_grid), the seed.
void fill_grid(const RtRenderParams *p, rtdev::TraceArgs &a);
// Rows of the owned-row grid of a render with these parameters (a multiple of strip_rows with strips).
int owned_rows_of(const RtRenderParams *p);
// Image row of row `vr` of the launch's owned-row grid (identity without strips).
inline int owned_row_to_image_row(const RtRenderParams *p, int vr) {
    if (p->strip_count <= 1) return vr;
    return ((vr / p->strip_rows) * p->strip_count + p->strip_index) * p->strip_rows + vr % p->strip_rows;
}
// The strips of a several-device call: strip j of `strip_rows` rows (0: 8, written back) goes to share j % n; params[i] is
// share i's (the caller's own with n == 1).  Refuses parameters that cannot be combined with strips dealt out by the call.
int deal_strips(const RtRenderParams *p, int n, int &strip_rows, std::vector<RtRenderParams> &params);

// Work is handed out in tiles of 8x8 cells: the tiles across `cells`, the tiles of a cols x rows grid, and that grid in a
// render's argument block (tiles_x, n_tiles).
inline int tiles_across(int cells) { return (cells + 7) / 8; }
inline size_t tile_count(int cols, int rows) { return (size_t)tiles_across(cols) * (size_t)tiles_across(rows); }
inline void set_tile_grid(rtdev::TraceArgs &a, int cols, int rows) {
    a.tiles_x = tiles_across(cols);
    a.n_tiles = a.tiles_x * tiles_across(rows);
}

// ---------------------------------------------------------------------------------------------------------- a delivery
// What rt_deliver.hip launches, waits for and copies; rt_api.hip queues it.

// The reference's tile grid (cpu.rs:73-115): tiles_w x tiles_h tiles of width_step x height_step pixels, sent column by
// column, the remainders in the last column and row.  Sizes come out as the callbacks get them: never below 0.
struct TileGrid {
    int width, height, tiles_w, tiles_h, width_step, height_step;
    struct Span {
        int at, size;
    };
    TileGrid(int w, int h, int tw, int th) : width(w), height(h), tiles_w(tw), tiles_h(th), width_step(w / tw), height_step(h / th) {}
    Span column(int ws) const { return span(ws, tiles_w, width_step, width); } // (x, w)
    Span row(int hs) const { return span(hs, tiles_h, height_step, height); }  // (y, h)

  private:
    static Span span(int i, int n, int step, int extent) {
        const int size = i == n - 1 ? extent - step * i : step;
        return Span{step * i, size > 0 ? size : 0};
    }
};

// The regions of a whole-frame call: bands of tile rows over all `tiles_x` tile columns, top to bottom (rt_plan.cpp).
std::vector<rtdev::Region> frame_bands(int tile_rows, int tiles_x, int chunk_count);

// The regions of the tile stream, `tile_rows` tile rows each (none for a share that owns no rows): windows of tile
// columns of the grid's `tiles_w` columns, cut on the whole-frame item grid.  Tile columns [.., columns_after[r]) are
// complete once regions [0, r] are.  No window at all: an empty frame.
struct StreamWindows {
    std::vector<rtdev::Region> regions;
    std::vector<int> columns_after;
};
StreamWindows stream_windows(int width, int tiles_w, int tile_rows);

// The queue order of a launch: `regions`, each inside the tiles_x-wide grid of n_tiles tiles, with item_begin set for
// `chunks_per_tile` items per tile.  Refused: no region or more than RT_MAX_REGIONS, a region outside the grid, item
// counts that do not add up to the grid's.
int queue_order(const std::vector<rtdev::Region> &regions, int tiles_x, int n_tiles, int chunks_per_tile,
                rtdev::Region out[rtdev::RT_MAX_REGIONS], int &n_out);

// The rows of a finished band that exist in an image of `height` rows, as runs of consecutive image rows in increasing
// order (a strip, or the whole band without strips).
struct RowRun {
    int image_row, rows;
};
std::vector<RowRun> copy_runs(const RtRenderParams *p, const rtdev::Region &band, int height);

} // namespace rtapi
