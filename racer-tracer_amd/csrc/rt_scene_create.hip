// rt_scene_create.hip — scenes on the device: rt_scene_create / rt_scene_create_ex, rt_scene_destroy (include/rt_abi.h; the
// render-buffer cache between them is rt_render_cache.h's), plus the scene-level exports for the tests.  scene_create reads top to bottom:
// validate, plan (rt_plan.h: values only), choose the tree, upload, size the pooled kernel, take render buffers.
//
// Host code only (HIP runtime calls).  Nothing here falls back to a CPU renderer: without a usable HIP device
// rt_scene_create returns RT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "rt_rect_pairs.h"
#include "rt_render_cache.h"
#include "rt_scene.h"

using rtapi::DevBuf;
using rtapi::fail;

namespace {
// ------------------------------------------------------------------------------------------------ scene creation
#define RT_FAST_LAUNCHER(member, name, ret, params) name,
#define RT_EXACT_LAUNCHER(member, name, ret, params) name##_exact,
const rtapi::Launchers kFastLaunchers = {RT_LAUNCHER_LIST(RT_FAST_LAUNCHER)};
const rtapi::Launchers kExactLaunchers = {RT_LAUNCHER_LIST(RT_EXACT_LAUNCHER)};
#undef RT_FAST_LAUNCHER
#undef RT_EXACT_LAUNCHER

template <class T> int upload(DevBuf<T> &buf, const std::vector<T> &host) {
    RT_HIP(buf.alloc(host.size()));
    if (!host.empty()) RT_HIP(hipMemcpy(buf.ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

// The images' texels on the device (RtScene.image_pixels) and their device records.
int upload_images(const RtSceneDesc *d, RtScene *s, std::vector<rtdev::Image> &images) {
    images.assign((size_t)d->n_images, rtdev::Image());
    s->image_pixels = std::vector<DevBuf<uint8_t>>((size_t)d->n_images);
    for (int i = 0; i < d->n_images; ++i) {
        size_t bytes = (size_t)d->images[i].width * (size_t)d->images[i].height * 4;
        DevBuf<uint8_t> &texels = s->image_pixels[(size_t)i];
        RT_HIP(texels.alloc(bytes));
        RT_HIP(hipMemcpy(texels.ptr, d->images[i].rgba, bytes, hipMemcpyHostToDevice));
        images[(size_t)i].rgba = texels.ptr;
        images[(size_t)i].width = d->images[i].width;
        images[(size_t)i].height = d->images[i].height;
    }
    return RT_OK;
}

// Primitives per leaf.  A leaf primitive costs a lane four times what a node costs (its record comes from global memory,
// the node from LDS; `random`: 40 % of the walk for 5.8 tests against 26.5 nodes per segment), so leaves of three beat
// leaves of four (66.1 -> 62.1 ms) — as long as the larger node array does not cost the variant a block per CU (leaves of
// two: 70.6 ms with three blocks instead of four).  A tree whose nodes stay in global memory, where a step is two dependent
// loads and every node not visited counts, comes with the eight direction-ordered copies (rt_bvh.cpp; 8 x 32 B per node).
rtdev::BvhBuild choose_bvh(const RtSceneDesc *d, const RtScene *s) {
    using rtapi::kBvhLdsBytes;
    auto blocks_with = [&](const rtdev::BvhBuild &b) {
        const size_t bytes = b.nodes.size() * sizeof(rtdev::BvhNode);
        const size_t dyn = rtdev::pool_lds_layout(true, s->textured, d->n_primitives, d->n_textures, bytes <= kBvhLdsBytes ? (int)b.nodes.size() : 0,
                                                  d->n_perlins > 0 && s->perlin_identity, false, s->has_moving).bytes;
        return s->kernels->pool_blocks_per_cu(s->prims_class, s->textured, s->specular, 1, dyn);
    };
    // (more than 2048 primitives: at most four to a leaf, the node array cannot fit LDS — the direction-ordered copies are
    // wanted, built in the same pass)
    const bool surely_large = d->n_primitives > 2048;
    rtdev::BvhBuild bvh = rtdev::build_bvh(d->primitives, d->n_primitives, 4, surely_large);
    int max_leaf = 0;
#ifdef RT_DEVELOPER_KNOBS
    if (const char *k = getenv("RT_BVH_LEAF")) max_leaf = atoi(k);
#endif
    if (max_leaf > 0) {
        bvh = rtdev::build_bvh(d->primitives, d->n_primitives, max_leaf);
    } else if (bvh.nodes.size() * sizeof(rtdev::BvhNode) <= kBvhLdsBytes) { // the nodes live in LDS
        rtdev::BvhBuild three = rtdev::build_bvh(d->primitives, d->n_primitives, 3);
        if (three.nodes.size() * sizeof(rtdev::BvhNode) <= kBvhLdsBytes && blocks_with(three) == blocks_with(bvh)) bvh = std::move(three);
    }
    bool ordered = true;
#ifdef RT_DEVELOPER_KNOBS
    if (const char *k = getenv("RT_BVH_ORDERED")) ordered = atoi(k) != 0;
#endif
    if (!ordered) bvh.ordered.clear();
    else if (bvh.nodes.size() * sizeof(rtdev::BvhNode) > kBvhLdsBytes && bvh.ordered.empty())
        bvh = rtdev::build_bvh(d->primitives, d->n_primitives, max_leaf > 0 ? max_leaf : 4, true);
    return bvh;
}

// The tree on the device, its leaf records beside it, and its numbers in the scene.
int upload_bvh(RtScene *s, const rtdev::BvhBuild &bvh, const rtapi::LeafTable &leaves) {
    const bool nodes_fit_lds = bvh.nodes.size() * sizeof(rtdev::BvhNode) <= rtapi::kBvhLdsBytes;
    int rc = RT_OK;
    if (!nodes_fit_lds && !bvh.ordered.empty() && (rc = upload(s->bvh_nodes_ordered, bvh.ordered)) != RT_OK) return rc;
    if ((rc = upload(s->bvh_nodes, bvh.nodes)) != RT_OK) return rc;
    if (nodes_fit_lds) { // kept for the per-camera child order (enqueue_render: order_bvh_for_camera)
        s->bvh_host.nodes = bvh.nodes;
        for (int k = 0; k < 3; ++k) s->bvh_host.center[k] = bvh.center[k];
    }
    if ((rc = upload(s->bvh_prim_index, bvh.prim_index)) != RT_OK) return rc;
    s->n_bvh_nodes = (int)bvh.nodes.size() - 1; // the array ends with the sentinel (rt_device_types.h: BvhNode)
    for (int k = 0; k < 3; ++k) {
        s->bvh_root_mn[k] = bvh.root_mn[k];
        s->bvh_root_mx[k] = bvh.root_mx[k];
        s->bvh_center[k] = bvh.center[k];
    }
    s->leaf_time_a = leaves.time_a;
    s->leaf_inv_dt = leaves.inv_dt;
    return upload(s->leaf_geo, leaves.geo);
}

// The pooled variant's LDS bill — its dynamic LDS (rt_device_types.h: pool_lds_layout) without and with the lens
// samples, and its static LDS: what enqueue_render checks against the CU's LDS before a launch — and its resident blocks
// per CU.  The v1 kernel has no dynamic LDS.
int size_pool(RtScene *s) {
    RT_HIP(hipDeviceGetAttribute(&s->num_cus, hipDeviceAttributeMultiprocessorCount, s->device));
    s->bvh_nodes_in_lds = s->use_bvh && (size_t)(s->n_bvh_nodes + 1) * sizeof(rtdev::BvhNode) <= rtapi::kBvhLdsBytes;
#ifdef RT_DEVELOPER_KNOBS
    if (const char *k = getenv("RT_BVH_LDS")) s->bvh_nodes_in_lds = s->bvh_nodes_in_lds && atoi(k) != 0;
#endif
    if (!s->use_v1) {
        auto dyn_lds = [&](bool lens) {
            return rtdev::pool_lds_layout(s->use_bvh, s->textured, s->n_prims, s->n_textures, s->bvh_nodes_in_lds ? s->n_bvh_nodes + 1 : 0,
                                          s->n_perlins > 0 && s->perlin_identity, lens, s->has_moving).bytes;
        };
        s->pool_dyn_lds = dyn_lds(false);
        s->pool_dyn_lds_lens = dyn_lds(true);
        s->pool_static_lds = s->kernels->pool_static_lds(s->prims_class, s->textured, s->specular, s->use_bvh);
        if (s->pool_static_lds < 0) return fail(RT_ERR_HIP, "hipFuncGetAttributes of the trace kernel failed");
        s->pool_blocks_per_cu = s->kernels->pool_blocks_per_cu(s->prims_class, s->textured, s->specular, s->use_bvh, s->pool_dyn_lds);
        s->pool_blocks_per_cu_lens = s->kernels->pool_blocks_per_cu(s->prims_class, s->textured, s->specular, s->use_bvh, s->pool_dyn_lds_lens);
    }
#ifdef RT_DEVELOPER_KNOBS // occupancy experiments
    if (const char *k = getenv("RT_POOL_BLOCKS_PER_CU"))
        if (atoi(k) > 0) s->pool_blocks_per_cu = s->pool_blocks_per_cu_lens = atoi(k);
#endif
    return RT_OK;
}

// The scene's render buffers: a cached set of this device's, or a fresh one of what every render needs.
int acquire_render_buffers(RtScene *s) {
    rtapi::RenderBuffers &b = s->buf;
    if (!rtapi::render_cache_take(s->device, b)) { // nothing of this device's to take over: the first scene, or more than the cache holds
        b.device = s->device;
        RT_HIP(b.segments.alloc(rtdev::RT_STAT_SLOTS)); // rt_device_types.h: RT_STAT_*
        RT_HIP(b.stream.ensure(hipStreamNonBlocking));
        RT_HIP(b.ev_begin.ensure()); // (timing events: rt_scene_last_stats reads their spans)
        RT_HIP(b.ev_traced.ensure());
        RT_HIP(b.ev_resolved.ensure());
        RT_HIP(b.host_flags.alloc(rtdev::RT_MAX_REGIONS + 1, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
        memset(b.host_flags.ptr, 0, (rtdev::RT_MAX_REGIONS + 1) * sizeof(unsigned int));
        RT_HIP(b.stream_ctl.ensure(hipStreamNonBlocking));
    }
    RT_HIP(hipMemsetAsync(b.segments.ptr, 0, rtdev::RT_STAT_SLOTS * sizeof(unsigned long long), b.stream));
    return RT_OK;
}

int scene_create(const RtSceneDesc *d, int device, const RtSceneOptions *options, RtScene **out) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int rc = rtapi::validate_desc(d);
    if (rc != RT_OK) return rc;
    RtSceneOptions opt;
    if ((rc = rtapi::check_options(options, opt)) != RT_OK) return rc;
    int n_dev = rt_device_count();
    if (n_dev <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device is visible to this process");
    if (device < 0 || device >= n_dev) return fail(RT_ERR_INVALID_ARGUMENT, "device index out of range");
    RT_HIP(hipSetDevice(device));

    RtScene *s = new RtScene(); // (std::bad_alloc: rtapi::guarded)
    std::unique_ptr<RtScene, void (*)(RtScene *)> half_built(s, rt_scene_destroy); // destroyed on any early return
    s->device = device;
    s->exact = opt.arithmetic == RT_ARITH_REFERENCE;
    s->gather_staged = opt.gather == RT_GATHER_STAGED;
    s->use_v1 = opt.kernel == RT_KERNEL_V1;
    s->launch_blocks = opt.launch_blocks;

    // ---- plan: what the description alone decides (rt_plan.h)
    std::vector<rtdev::Prim> prims = rtapi::pack_prims(d);
    s->radiance_bound = rtapi::scene_radiance_bound(d);
    const std::vector<rtdev::Perlin> perlins = rtapi::pack_perlins(d, s->perlin_identity);
    const rtapi::Selection sel = rtapi::select_variant(d);
    s->prims_class = sel.prims_class;
    s->textured = sel.textured;
    s->specular = sel.specular;
    s->has_moving = sel.has_moving;
    rtapi::scene_bounds(d, s->box_mn, s->box_mx);
    s->use_bvh = d->n_primitives > rtapi::kBvhThreshold;
    if (opt.closest_hit != RT_HIT_AUTO) s->use_bvh = opt.closest_hit == RT_HIT_BVH && d->n_primitives > 0;
    // The RT_ARITH_FAST copies of the pooled variants that keep two items in flight (any primitive kind, BVH:
    // rt_trace_pool_kernel.hip, OVERLAP) have fixed-point sums only: a scene without a radiance bound is rendered by their
    // RT_ARITH_REFERENCE copies (f64 sums, one item per wave at a time, the reference's own divisions: ~25 % slower).
    if (s->radiance_bound == 0.0 && !s->use_v1 && (s->use_bvh || s->prims_class == 2)) s->exact = true;
    s->kernels = s->exact ? &kExactLaunchers : &kFastLaunchers;
    if (!s->use_bvh && (size_t)d->n_primitives * sizeof(rtdev::Prim) > rtapi::kLinearTableBytes)
        return fail(RT_ERR_UNSUPPORTED, "RT_HIT_LINEAR: the primitive table does not fit in LDS");

    // ---- the tree (its leaf size depends on the variant's occupancy) and the order of the device table that follows from it
    std::vector<int32_t> order((size_t)d->n_primitives); // description index of each device record
    for (size_t j = 0; j < order.size(); ++j) order[j] = (int32_t)j;
    rtdev::BvhBuild bvh;
    rtapi::LeafTable leaves;
    if (s->use_bvh) { // the primitive table is put in leaf order (a leaf is a contiguous run of records)
        bvh = choose_bvh(d, s);
        order.assign(bvh.prim_index.begin(), bvh.prim_index.end());
        std::vector<rtdev::Prim> ordered(prims.size());
        for (size_t j = 0; j < bvh.prim_index.size(); ++j) ordered[j] = prims[(size_t)bvh.prim_index[j]];
        prims.swap(ordered);
        leaves = rtapi::leaf_geometry(prims);
    } else {
        const rtapi::LinearGroups groups = rtapi::group_linear_table(prims, order);
        for (int g = 0; g < 3; ++g) s->rect_end[g] = groups.rect_end[g];
        s->sphere_end = groups.sphere_end;
        s->box_end = groups.box_end;
        const int n_rects = groups.rect_end[2];
        // The facing pairs of the rect groups, marked in the device copy of the table, in the field behind k that no rect
        // test reads (rt_rect_pairs.h); every other grouped rect gets "no pair" there, whatever its host record held.
        {
            std::vector<rtdev::RectGeo> geo;
            for (int j = 0; j < n_rects; ++j) {
                const rtdev::Prim &q = prims[(size_t)j];
                geo.push_back(rtdev::RectGeo{j < groups.rect_end[0] ? 2 : (j < groups.rect_end[1] ? 1 : 0), q.p[0], q.p[1], q.p[2], q.p[3], q.p[4]});
            }
            std::vector<uint64_t> field((size_t)n_rects);
            rt_pairs::mark_table(geo.data(), groups.rect_end, field.data());
            for (int j = 0; j < n_rects; ++j) memcpy(&prims[(size_t)j].p[5], &field[(size_t)j], sizeof(uint64_t));
        }
        // a table of plain rects only: what their own pixel rectangles are formed from on every render (rt_primary_bounds.h)
        if (n_rects == d->n_primitives && n_rects <= rtdev::RT_PRIMARY_RECTS)
            for (int j = 0; j < n_rects; ++j) {
                const rtdev::Prim &q = prims[(size_t)j];
                s->primary_rect_geo.push_back(rtdev::RectGeo{j < groups.rect_end[0] ? 2 : (j < groups.rect_end[1] ? 1 : 0), q.p[0], q.p[1], q.p[2], q.p[3], q.p[4]});
            }
    }
    const rtapi::LightTables lights = rtapi::light_tables(d, order, rtapi::kMaxLights);

    // ---- upload
    std::vector<rtdev::Image> images;
    if ((rc = upload_images(d, s, images)) != RT_OK) return rc;
    const std::vector<rtdev::Texture> textures = rtapi::pack_textures(d, images);
    if (s->use_bvh && (rc = upload_bvh(s, bvh, leaves)) != RT_OK) return rc;
    if ((rc = rtapi::build_light_list(s, lights)) != RT_OK) return rc;
    // what rt_scene_set_lights lists again from; rt_scene_light_weights of the list as created: the uniform pick's
    s->light_facts = rtapi::light_facts(d);
    s->table_order = order;
    s->pick_weights.assign(lights.lights.size(), lights.lights.empty() ? 0.0 : 1.0 / (double)lights.lights.size());
    if ((rc = upload(s->prims, prims)) != RT_OK) return rc;
    if ((rc = upload(s->textures, textures)) != RT_OK) return rc;
    if ((rc = upload(s->images, images)) != RT_OK) return rc;
    if ((rc = upload(s->perlins, perlins)) != RT_OK) return rc;
    s->n_prims = d->n_primitives;
    s->n_materials = d->n_materials;
    s->n_textures = d->n_textures;
    s->n_images = d->n_images;
    s->n_perlins = d->n_perlins;
    s->bg.kind = d->background.kind;
    for (int k = 0; k < 3; ++k) {
        s->bg.top[k] = d->background.top[k];
        s->bg.bottom[k] = d->background.bottom[k];
    }
    if ((rc = size_pool(s)) != RT_OK) return rc;
    if ((rc = acquire_render_buffers(s)) != RT_OK) return rc;
    *out = half_built.release();
    return RT_OK;
}

} // namespace

extern "C" {

void rt_scene_destroy(RtScene *s) {
    if (s) rtapi::scene_destroy(s); // rt_render_cache.h
}

void rt_release_cached_buffers(void) {
    (void)rtapi::guarded("rt_release_cached_buffers", [] { rtapi::render_cache_release_all(); return RT_OK; });
}

int rt_scene_create(const RtSceneDesc *d, int device, RtScene **out) {
    return rtapi::guarded("rt_scene_create", [&] { return scene_create(d, device, nullptr, out); });
}

int rt_scene_create_ex(const RtSceneDesc *d, int device, const RtSceneOptions *options, RtScene **out) {
    return rtapi::guarded("rt_scene_create_ex", [&] { return scene_create(d, device, options, out); });
}

int rtdev_scene_classify(const RtSceneDesc *d, int32_t out[4]) {
    return rtapi::guarded("rtdev_scene_classify", [&]() -> int {
        if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
        int rc = rtapi::validate_desc(d);
        if (rc != RT_OK) return rc;
        const rtapi::Selection sel = rtapi::select_variant(d);
        out[0] = sel.prims_class;
        out[1] = sel.textured;
        out[2] = sel.specular;
        out[3] = sel.has_moving;
        return RT_OK;
    });
}

int rtdev_scene_radiance_bound(const RtSceneDesc *d, double *bound) {
    return rtapi::guarded("rtdev_scene_radiance_bound", [&]() -> int {
        if (!bound) return fail(RT_ERR_INVALID_ARGUMENT, "bound is NULL");
        int rc = rtapi::validate_desc(d);
        if (rc != RT_OK) return rc;
        *bound = rtapi::scene_radiance_bound(d);
        return RT_OK;
    });
}

int rtdev_scene_variant(const RtScene *s, int32_t *out, int32_t n_out) {
    return rtapi::guarded("rtdev_scene_variant", [&]() -> int {
        if (!s || (!out && n_out > 0) || n_out < 0) return fail(RT_ERR_INVALID_ARGUMENT, "scene/out is NULL or n_out is negative");
        const int32_t v[RTDEV_VARIANT_FIELDS] = {
            s->use_v1 ? 1 : 0, s->prims_class, s->textured, s->specular, s->use_bvh, (int32_t)s->exact, s->bvh_nodes_in_lds ? 1 : 0,
            s->has_moving, (s->textured && s->n_perlins > 0 && s->perlin_identity) ? 1 : 0,
            s->use_v1 ? 0 : s->pool_static_lds, s->use_v1 ? 0 : (int32_t)s->pool_dyn_lds, s->use_v1 ? 0 : (int32_t)s->pool_dyn_lds_lens,
            s->pool_blocks_per_cu, s->pool_blocks_per_cu_lens, s->last_launch_blocks, s->last_launch_items};
        for (int32_t k = 0; k < n_out && k < RTDEV_VARIANT_FIELDS; ++k) out[k] = v[k];
        return RT_OK;
    });
}

} // extern "C"