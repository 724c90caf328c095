// rt_plan.cpp — the device-free rules of rt_plan.h: validation, kernel selection, the radiance bound and the error budget
// of the fixed-point sums, the device records and their permutations, the light list, the chunk plan (which fixes the
// order of every pixel's sum), launches, passes, the pixel grid and strips, the plans of a delivering call.  Host code for
// any C++17 compiler.
#include "rt_plan.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <string>

namespace rtapi {

// -------------------------------------------------------------------------------------------------------------- a scene

int validate_desc(const RtSceneDesc *d) {
    if (!d) return fail(RT_ERR_INVALID_ARGUMENT, "scene description is NULL");
    if (d->n_primitives < 0 || d->n_materials < 0 || d->n_textures < 0 || d->n_images < 0 || d->n_perlins < 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "negative table size");
    if ((d->n_primitives && !d->primitives) || (d->n_materials && !d->materials) ||
        (d->n_textures && !d->textures) || (d->n_images && !d->images) || (d->n_perlins && !d->perlins))
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL table with non-zero size");
    for (int i = 0; i < d->n_textures; ++i) {
        const RtTexture &t = d->textures[i];
        switch (t.kind) {
        case RT_TEX_SOLID_COLOR: break;
        case RT_TEX_CHECKERED:
            for (int c : {t.tex_even, t.tex_odd}) {
                if (c < 0 || c >= d->n_textures)
                    return fail(RT_ERR_SCENE_LOAD, "Checkered texture " + std::to_string(i) + " names a missing texture");
                if (d->textures[c].kind == RT_TEX_CHECKERED) // scene/yml.rs:212-243 resolves one level only
                    return fail(RT_ERR_UNSUPPORTED, "Checkered texture of a Checkered texture");
            }
            break;
        case RT_TEX_IMAGE:
            if (t.image < 0 || t.image >= d->n_images) return fail(RT_ERR_INVALID_ARGUMENT, "texture image index out of range");
            break;
        case RT_TEX_NOISE:
            if (t.perlin < 0 || t.perlin >= d->n_perlins) return fail(RT_ERR_INVALID_ARGUMENT, "texture perlin index out of range");
            if (t.depth < 0) return fail(RT_ERR_INVALID_ARGUMENT, "negative noise depth");
            break;
        default: return fail(RT_ERR_INVALID_ARGUMENT, "unknown texture kind");
        }
    }
    for (int i = 0; i < d->n_images; ++i)
        if (!d->images[i].rgba || d->images[i].width <= 0 || d->images[i].height <= 0)
            return fail(RT_ERR_FAILED_TO_OPEN_IMAGE, "image " + std::to_string(i) + " is empty");
    for (int i = 0; i < d->n_materials; ++i) {
        const RtMaterial &m = d->materials[i];
        if (m.kind < RT_MAT_LAMBERTIAN || m.kind > RT_MAT_DIFFUSE_LIGHT)
            return fail(RT_ERR_UNKNOWN_MATERIAL, "unknown material kind");
        if (m.kind != RT_MAT_DIELECTRIC && (m.texture < 0 || m.texture >= d->n_textures))
            return fail(RT_ERR_SCENE_LOAD, "material " + std::to_string(i) + " names a missing texture");
    }
    for (int i = 0; i < d->n_primitives; ++i) {
        const RtPrimitive &p = d->primitives[i];
        if (p.kind < RT_PRIM_SPHERE || p.kind > RT_PRIM_MOVING_SPHERE) return fail(RT_ERR_INVALID_ARGUMENT, "unknown primitive kind");
        if (p.kind == RT_PRIM_MOVING_SPHERE && (p.flags & (RT_PRIM_HAS_ROTATE_Y | RT_PRIM_HAS_TRANSLATE)))
            return fail(RT_ERR_UNSUPPORTED, "a MovingSphere cannot be wrapped in RotateY/Translate");
        if (p.material < 0 || p.material >= d->n_materials)
            return fail(RT_ERR_UNKNOWN_MATERIAL, "primitive " + std::to_string(i) + " names a missing material");
    }
    if (d->background.kind != RT_BG_SKY && d->background.kind != RT_BG_SOLID)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown background kind");
    return RT_OK;
}

int check_options(const RtSceneOptions *options, RtSceneOptions &opt) {
    memset(&opt, 0, sizeof opt);
    if (options) opt = *options;
    if (opt.closest_hit < RT_HIT_AUTO || opt.closest_hit > RT_HIT_BVH) return fail(RT_ERR_INVALID_ARGUMENT, "unknown closest_hit option");
    if (opt.kernel < RT_KERNEL_POOL || opt.kernel > RT_KERNEL_V1) return fail(RT_ERR_INVALID_ARGUMENT, "unknown kernel option");
    if (opt.arithmetic < RT_ARITH_FAST || opt.arithmetic > RT_ARITH_REFERENCE) return fail(RT_ERR_INVALID_ARGUMENT, "unknown arithmetic option");
    if (opt.gather < RT_GATHER_AUTO || opt.gather > RT_GATHER_STAGED) return fail(RT_ERR_INVALID_ARGUMENT, "unknown gather option");
    if (opt.launch_blocks < 0) return fail(RT_ERR_INVALID_ARGUMENT, "launch_blocks must not be negative (0: no cap)");
    for (int32_t r : opt._reserved)
        if (r != 0) return fail(RT_ERR_INVALID_ARGUMENT, "reserved option fields must be 0");
    return RT_OK;
}

Selection select_variant(const RtSceneDesc *d) {
    Selection sel{0, 0, 0, 0};
    bool only_rects = true, only_spheres = true;
    for (int i = 0; i < d->n_primitives; ++i) {
        const RtPrimitive &p = d->primitives[i];
        const bool wrapped = (p.flags & (RT_PRIM_HAS_ROTATE_Y | RT_PRIM_HAS_TRANSLATE)) != 0;
        const bool is_rect = p.kind == RT_PRIM_XY_RECT || p.kind == RT_PRIM_XZ_RECT || p.kind == RT_PRIM_YZ_RECT;
        if (wrapped || !is_rect) only_rects = false;
        if (wrapped || p.kind != RT_PRIM_SPHERE) only_spheres = false;
        if (p.kind == RT_PRIM_MOVING_SPHERE) sel.has_moving = 1;
    }
    sel.prims_class = only_rects ? 0 : (only_spheres ? 1 : 2);
    for (int i = 0; i < d->n_materials; ++i) {
        const RtMaterial &m = d->materials[i];
        if (m.kind == RT_MAT_METAL || m.kind == RT_MAT_DIELECTRIC) sel.specular = 1;
        if (m.kind != RT_MAT_DIELECTRIC && d->textures[m.texture].kind != RT_TEX_SOLID_COLOR) sel.textured = 1;
    }
    return sel;
}

// THE ERROR BUDGET OF THE FIXED-POINT SUMS (rt_device_types.h: sum_scale).  A sample's radiance T is rounded to a multiple
// of 2^(e-52): an ABSOLUTE error of at most 2^(e-53) per sample, hence in the pixel's mean.  The frame holds sqrt(mean),
// and |sqrt(a) - sqrt(b)| <= sqrt(|a - b|): a pixel of radiance near 0 comes out up to sqrt(2^(e-53)) from the f64 sum's
// value.  The 1e-3 per channel that RT_ARITH_FAST promises (rt_abi.h) therefore allows e <= 31 (4.9e-4, half the
// tolerance; e = 33 would be 9.8e-4, all of it).  A bound below 2^30 gives e <= 31 for chunks of up to 2048 samples; a
// scene whose bound is larger has none (RT_ARITH_REFERENCE copy, f64 sums), and a render whose longer chunks would push e
// past 31 is refused.
constexpr double kSumsBoundCap = 0x1p30;
constexpr int kSumsMaxExponent = 31;

// What a finished sample can be at most (RtScene.radiance_bound): the product of its path's attenuations times what the
// path ran into.  Attenuations are texture values (lambertian.rs:36, metal.rs:40) or 1 (dialectric.rs:26) — a
// SolidColor's colour, a Noise colour times 0.5 (1 + sin) <= the colour, an image texel <= 1 — so with every such colour
// in [0, 1] the bound is the largest of 1 (renderer.rs:48-55: white at depth 0), the emitted colours
// (diffuse_light.rs:33-35) and the background's.  A colour outside [0, 1] on a scattering material, or anything
// negative or not finite, leaves the scene without a bound (0): the pooled kernel then keeps f64 sums.  So does a bound
// of kSumsBoundCap or more (sum_exponent below: the error budget of the fixed-point sums).
double scene_radiance_bound(const RtSceneDesc *d) {
    bool bounded = true;
    double bound = 1.0;
    auto colours_of = [&](int ti, double &hi, double &lo) { // over the texture and, for a Checkered, its two sides
        auto one = [&](const RtTexture &t) {
            if (t.kind == RT_TEX_IMAGE) {
                hi = std::max(hi, 1.0);
                lo = std::min(lo, 0.0);
                return;
            }
            if (t.kind == RT_TEX_CHECKERED) return;
            for (int k = 0; k < 3; ++k) {
                if (!std::isfinite(t.color[k])) bounded = false;
                hi = std::max(hi, t.color[k]);
                lo = std::min(lo, t.color[k]);
            }
        };
        const RtTexture &t = d->textures[ti];
        one(t);
        if (t.kind == RT_TEX_CHECKERED) {
            one(d->textures[t.tex_even]);
            one(d->textures[t.tex_odd]);
            // (a Checkered inside a Checkered is not evaluated further by the kernels: texture_value_deferred returns its colour field)
            for (int side : {t.tex_even, t.tex_odd})
                if (d->textures[side].kind == RT_TEX_CHECKERED)
                    for (int k = 0; k < 3; ++k) {
                        if (!std::isfinite(d->textures[side].color[k])) bounded = false;
                        hi = std::max(hi, d->textures[side].color[k]);
                        lo = std::min(lo, d->textures[side].color[k]);
                    }
        }
    };
    for (int i = 0; i < d->n_materials; ++i) {
        const RtMaterial &m = d->materials[i];
        if (m.kind == RT_MAT_DIELECTRIC) continue;
        double hi = 0.0, lo = 0.0;
        colours_of(m.texture, hi, lo);
        if (lo < 0.0) bounded = false;
        if (m.kind == RT_MAT_DIFFUSE_LIGHT) bound = std::max(bound, hi);
        else if (hi > 1.0) bounded = false;
    }
    for (int k = 0; k < 3; ++k)
        for (double c : {d->background.top[k], d->background.bottom[k]}) {
            if (!std::isfinite(c) || c < 0.0) bounded = false;
            bound = std::max(bound, c);
        }
    return bounded && std::isfinite(bound) && bound < kSumsBoundCap ? bound : 0.0;
}

namespace {
bool texture_reads_uv(const RtSceneDesc *d, int ti) {
    const RtTexture &t = d->textures[ti];
    if (t.kind == RT_TEX_IMAGE) return true;
    if (t.kind == RT_TEX_CHECKERED)
        return d->textures[t.tex_even].kind == RT_TEX_IMAGE || d->textures[t.tex_odd].kind == RT_TEX_IMAGE;
    return false;
}
} // namespace

void scene_bounds(const RtSceneDesc *d, double box_mn[3], double box_mx[3]) {
    for (int k = 0; k < 3; ++k) {
        box_mn[k] = 1.0;
        box_mx[k] = -1.0;
    }
    for (int i = 0; i < d->n_primitives; ++i) {
        double mn[3], mx[3];
        rtdev::primitive_bounds(d->primitives[i], mn, mx);
        for (int k = 0; k < 3; ++k) { // (std::fmin would drop a NaN)
            if (i == 0 || std::isnan(mn[k]) || mn[k] < box_mn[k]) box_mn[k] = std::isnan(box_mn[k]) && i > 0 ? box_mn[k] : mn[k];
            if (i == 0 || std::isnan(mx[k]) || mx[k] > box_mx[k]) box_mx[k] = std::isnan(box_mx[k]) && i > 0 ? box_mx[k] : mx[k];
        }
    }
}

std::vector<rtdev::Prim> pack_prims(const RtSceneDesc *d) {
    std::vector<rtdev::Material> materials((size_t)d->n_materials);
    for (int i = 0; i < d->n_materials; ++i) {
        const RtMaterial &m = d->materials[i];
        rtdev::Material &q = materials[(size_t)i];
        memset(&q, 0, sizeof q);
        q.kind = m.kind;
        q.texture = m.texture;
        q.tex_kind = -1;
        q.fuzz = m.fuzz;
        q.ior = m.refraction_index;
        if (m.kind == RT_MAT_DIELECTRIC) { // rt_device_types.h: the per-hit quotients, once
            const double ior = m.refraction_index;
            q.color[0] = 1.0 / ior;
            const double front = (1.0 - q.color[0]) / (1.0 + q.color[0]), back = (1.0 - ior) / (1.0 + ior);
            q.color[1] = front * front;
            q.color[2] = back * back;
        }
        if (m.kind != RT_MAT_DIELECTRIC) {
            const RtTexture &t = d->textures[m.texture];
            q.tex_kind = t.kind;
            q.needs_uv = texture_reads_uv(d, m.texture) ? 1 : 0;
            for (int k = 0; k < 3; ++k) q.color[k] = t.color[k];
        }
    }
    std::vector<rtdev::Prim> prims((size_t)d->n_primitives);
    for (int i = 0; i < d->n_primitives; ++i) {
        const RtPrimitive &p = d->primitives[i];
        rtdev::Prim &q = prims[(size_t)i];
        memset(&q, 0, sizeof q);
        for (int k = 0; k < 6; ++k) q.p[k] = p.p[k];
        q.rot_sin = p.rot_sin;
        q.rot_cos = p.rot_cos;
        for (int k = 0; k < 3; ++k) q.tr[k] = p.translate[k];
        q.kind = p.kind;
        q.flags = p.flags & (RT_PRIM_HAS_ROTATE_Y | RT_PRIM_HAS_TRANSLATE);
        // an absent wrapper is the identity on the device (box_t subtracts the offset unconditionally)
        if (!(q.flags & RT_PRIM_HAS_TRANSLATE)) q.tr[0] = q.tr[1] = q.tr[2] = 0.0;
        if (!(q.flags & RT_PRIM_HAS_ROTATE_Y)) {
            q.rot_sin = 0.0;
            q.rot_cos = 1.0;
        }
        q.material = p.material;
        q.obj_id = p.obj_id;
        q.inv_radius = (p.kind == RT_PRIM_SPHERE || p.kind == RT_PRIM_MOVING_SPHERE) ? 1.0 / p.p[3] : 0.0;
        q.radius2 = p.p[3] * p.p[3];
        if (p.kind == RT_PRIM_MOVING_SPHERE) { // device packing: tr = pos_b - pos_a, rot_sin = time_a, rot_cos = 1/(time_b - time_a)
            for (int k = 0; k < 3; ++k) q.tr[k] = p.center_b[k] - p.p[k];
            q.rot_sin = p.time_a;
            q.rot_cos = 1.0 / (p.time_b - p.time_a);
        }
        q.mat = materials[(size_t)q.material];
    }
    return prims;
}

std::vector<rtdev::Texture> pack_textures(const RtSceneDesc *d, const std::vector<rtdev::Image> &images) {
    std::vector<rtdev::Texture> textures((size_t)d->n_textures);
    for (int i = 0; i < d->n_textures; ++i) {
        const RtTexture &t = d->textures[i];
        rtdev::Texture &q = textures[(size_t)i];
        memset(&q, 0, sizeof q);
        q.kind = t.kind;
        q.tex_even = t.tex_even;
        q.tex_odd = t.tex_odd;
        q.image = t.image;
        q.perlin = t.perlin;
        q.depth = t.depth;
        for (int k = 0; k < 3; ++k) q.color[k] = t.color[k];
        q.scale = t.scale;
        if (t.kind == RT_TEX_IMAGE) {
            q.img.rgba = images[(size_t)t.image].rgba;
            q.img.width = images[(size_t)t.image].width;
            q.img.height = images[(size_t)t.image].height;
        }
    }
    return textures;
}

std::vector<rtdev::Perlin> pack_perlins(const RtSceneDesc *d, int &identity) {
    std::vector<rtdev::Perlin> perlins((size_t)d->n_perlins);
    for (int i = 0; i < d->n_perlins; ++i) {
        static_assert(sizeof(rtdev::Perlin) == sizeof(RtPerlin), "Perlin layouts must match");
        memcpy(&perlins[(size_t)i], &d->perlins[i], sizeof(RtPerlin));
        for (int k = 0; k < 256; ++k)
            if (d->perlins[i].perm_x[k] != k || d->perlins[i].perm_y[k] != k || d->perlins[i].perm_z[k] != k) identity = 0;
    }
    return perlins;
}

LinearGroups group_linear_table(std::vector<rtdev::Prim> &prims, std::vector<int32_t> &order) {
    LinearGroups ends{};
    std::vector<rtdev::Prim> sorted;
    std::vector<int32_t> sorted_order;
    sorted.reserve(prims.size());
    auto group_of = [](const rtdev::Prim &q) {
        if (q.flags == 0 && q.kind == RT_PRIM_XY_RECT) return 0;
        if (q.flags == 0 && q.kind == RT_PRIM_XZ_RECT) return 1;
        if (q.flags == 0 && q.kind == RT_PRIM_YZ_RECT) return 2;
        if (q.flags == 0 && q.kind == RT_PRIM_SPHERE) return 3;
        if (q.kind == RT_PRIM_BOX) return 4; // bare or wrapped
        return 5;
    };
    for (int g = 0; g < 6; ++g) {
        for (size_t j = 0; j < prims.size(); ++j)
            if (group_of(prims[j]) == g) {
                sorted.push_back(prims[j]);
                sorted_order.push_back(order[j]);
            }
        if (g < 3) ends.rect_end[g] = (int)sorted.size();
        if (g == 3) ends.sphere_end = (int)sorted.size();
        if (g == 4) ends.box_end = (int)sorted.size();
    }
    prims.swap(sorted);
    order.swap(sorted_order);
    return ends;
}

LeafTable leaf_geometry(const std::vector<rtdev::Prim> &prims) {
    LeafTable leaves;
    leaves.geo.resize(prims.size());
    bool have_interval = false;
    for (size_t j = 0; j < prims.size(); ++j) {
        const rtdev::Prim &q = prims[j];
        rtdev::LeafGeo &g = leaves.geo[j];
        memset(&g, 0, sizeof g);
        g.tag = 1;
        if (q.flags != 0 || (q.kind != RT_PRIM_SPHERE && q.kind != RT_PRIM_MOVING_SPHERE)) continue;
        if (q.kind == RT_PRIM_MOVING_SPHERE) {
            // a MovingSphere with time_a == time_b degenerates by itself in the reference (moving_sphere.rs:37-39:
            // 0/0); its 1 / (time_b - time_a) = inf must not become the scene-wide interval, where it would turn
            // the centre of every plain Sphere (dc = 0) into inf * 0 = NaN: it keeps the general path (tag 1)
            if (!std::isfinite(q.rot_cos)) continue;
            if (!have_interval) {
                leaves.time_a = q.rot_sin;
                leaves.inv_dt = q.rot_cos;
                have_interval = true;
            }
            if (q.rot_sin != leaves.time_a || q.rot_cos != leaves.inv_dt) continue; // another interval: general path
            for (int k = 0; k < 3; ++k) g.dc[k] = q.tr[k];
        }
        for (int k = 0; k < 3; ++k) g.c0[k] = q.p[k];
        g.radius2 = q.radius2;
        g.tag = 0;
    }
    return leaves;
}

std::vector<LightFact> light_facts(const RtSceneDesc *d) {
    std::vector<LightFact> facts((size_t)d->n_primitives);
    for (int i = 0; i < d->n_primitives; ++i) {
        const RtPrimitive &p = d->primitives[i];
        LightFact &f = facts[(size_t)i];
        memset(&f, 0, sizeof f);
        f.kind = p.kind;
        f.flags = p.flags;
        for (int k = 0; k < 6; ++k) f.p[k] = p.p[k];
        f.tex_kind = -1;
        if (p.material < 0 || p.material >= d->n_materials) continue;
        const RtMaterial &m = d->materials[p.material];
        f.emitter = m.kind == RT_MAT_DIFFUSE_LIGHT ? 1 : 0;
        if (m.kind == RT_MAT_DIELECTRIC || m.texture < 0 || m.texture >= d->n_textures) continue;
        f.tex_kind = d->textures[m.texture].kind;
        for (int k = 0; k < 3; ++k) f.color[k] = d->textures[m.texture].color[k];
    }
    return facts;
}

int check_light_list_params(const RtLightListParams *p) {
    if (!p) return fail(RT_ERR_INVALID_ARGUMENT, "light list params is NULL");
    if (p->kinds < 0 || p->kinds > RT_LIGHTS_ALL) return fail(RT_ERR_INVALID_ARGUMENT, "light list kinds must be in 0..7");
    if (p->pick != RT_PICK_UNIFORM && p->pick != RT_PICK_POWER) return fail(RT_ERR_INVALID_ARGUMENT, "light list pick is not an RtLightPick");
    for (int32_t r : p->_reserved)
        if (r != 0) return fail(RT_ERR_INVALID_ARGUMENT, "light list _reserved must be 0");
    return RT_OK;
}

namespace {
bool is_rect(int kind) { return kind == RT_PRIM_XY_RECT || kind == RT_PRIM_XZ_RECT || kind == RT_PRIM_YZ_RECT; }
double box_area(const double *p) {
    const double a = std::fabs(p[3] - p[0]), b = std::fabs(p[4] - p[1]), c = std::fabs(p[5] - p[2]);
    return 2.0 * (a * b + b * c + c * a);
}
// Listed by today's rule (mask 0): an unwrapped Sphere of positive radius or an unwrapped rect of non-zero area, made of
// DiffuseLight; the mask adds wrapped ones, boxes and moving spheres (include/rt_abi.h: RtLightKinds)
bool listed(const LightFact &f, int kinds) {
    if (!f.emitter) return false;
    if (f.flags != 0 && !(kinds & RT_LIGHTS_WRAPPED)) return false;
    if (f.kind == RT_PRIM_SPHERE) return f.p[3] > 0.0;
    if (is_rect(f.kind)) return (f.p[1] - f.p[0]) * (f.p[3] - f.p[2]) != 0.0;
    if (f.kind == RT_PRIM_BOX) return (kinds & RT_LIGHTS_BOXES) != 0 && box_area(f.p) > 0.0;
    if (f.kind == RT_PRIM_MOVING_SPHERE) return (kinds & RT_LIGHTS_MOVING) != 0 && f.p[3] > 0.0;
    return false;
}
} // namespace

std::vector<int32_t> list_lights(const std::vector<LightFact> &facts, int kinds, int max_lights) {
    std::vector<int32_t> lights;
    for (size_t i = 0; i < facts.size() && (int)lights.size() < max_lights; ++i)
        if (listed(facts[i], kinds)) lights.push_back((int32_t)i);
    return lights;
}

LightTables light_tables_of(const std::vector<int32_t> &lights, const std::vector<int32_t> &order) {
    LightTables t;
    t.lights = lights;
    std::vector<int32_t> device_of(order.size(), -1);
    for (size_t j = 0; j < order.size(); ++j) device_of[(size_t)order[j]] = (int32_t)j;
    t.slot.assign(order.size(), -1);
    t.prim.resize(t.lights.size());
    for (size_t k = 0; k < t.lights.size(); ++k) {
        t.prim[k] = device_of[(size_t)t.lights[k]];
        t.slot[(size_t)t.prim[k]] = (int32_t)k;
    }
    return t;
}

LightTables light_tables(const RtSceneDesc *d, const std::vector<int32_t> &order, int max_lights) {
    return light_tables_of(list_lights(light_facts(d), RT_LIGHTS_PLAIN, max_lights), order);
}

bool light_is_plain(const LightFact &f) { return f.flags == 0 && (f.kind == RT_PRIM_SPHERE || is_rect(f.kind)); }

double light_weight(const LightFact &f) {
    const double PI = 3.14159265358979323846;
    double area;
    if (f.kind == RT_PRIM_SPHERE || f.kind == RT_PRIM_MOVING_SPHERE) area = 4.0 * PI * (f.p[3] * f.p[3]);
    else if (f.kind == RT_PRIM_BOX) area = box_area(f.p);
    else area = std::fabs((f.p[1] - f.p[0]) * (f.p[3] - f.p[2]));
    double L = 1.0;
    if (f.tex_kind == RT_TEX_SOLID_COLOR) {
        L = f.color[0]; // (comparisons, not std::fmax: a NaN component must not be dropped)
        for (int k = 1; k < 3; ++k)
            if (std::isnan(f.color[k]) || f.color[k] > L) L = std::isnan(L) ? L : f.color[k];
        if (!std::isfinite(L) || L < 0.0) L = 0.0;
    }
    return area * L;
}

LightPick light_pick(const std::vector<LightFact> &facts, const std::vector<int32_t> &lights, int n, int pick) {
    LightPick lp;
    if (n > (int)lights.size()) n = (int)lights.size();
    if (n <= 0) return lp;
    std::vector<double> w((size_t)n);
    double total = 0.0;
    for (int k = 0; k < n; ++k) total += (w[(size_t)k] = light_weight(facts[(size_t)lights[(size_t)k]]));
    lp.uniform = pick != RT_PICK_POWER || !(total > 0.0) || !std::isfinite(total);
    lp.p.resize((size_t)n);
    lp.cdf.resize((size_t)n);
    double run = 0.0;
    for (int k = 0; k < n; ++k) {
        if (lp.uniform) {
            lp.p[(size_t)k] = 1.0 / (double)n;
            lp.cdf[(size_t)k] = (double)(k + 1) / (double)n;
        } else {
            run += w[(size_t)k];
            lp.p[(size_t)k] = w[(size_t)k] / total;
            lp.cdf[(size_t)k] = run / total;
        }
    }
    lp.cdf[(size_t)n - 1] = 1.0;
    return lp;
}

// ------------------------------------------------------------------------------------------------------------- a render
int check_params(const RtCamera *camera, const RtRenderParams *p) {
    if (!camera || !p) return fail(RT_ERR_INVALID_ARGUMENT, "camera/params is NULL");
    // cpu.rs:36,40 divide by (W - 1) and (H - 1): a one-pixel dimension is a division by zero in the
    // reference (inf/NaN rays, an undefined picture); it is refused here instead of imitated
    if (p->width < 2 || p->height < 2) return fail(RT_ERR_INVALID_ARGUMENT, "width and height must be at least 2");
    if (p->samples <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "samples must be positive");
    if (p->max_depth < 0 || p->max_depth >= (1 << 24)) return fail(RT_ERR_INVALID_ARGUMENT, "max_depth out of range");
    if ((uint64_t)p->width * (uint64_t)p->height > 0xFFFFFFFFull) return fail(RT_ERR_INVALID_ARGUMENT, "image too large for the pixel counter");
    if (p->scale < 0) return fail(RT_ERR_INVALID_ARGUMENT, "scale must not be negative");
    if (p->scale > 1 && p->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "the preview scale cannot be combined with strips");
    if (p->strip_count > 1) {
        if (p->strip_rows <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "strip_rows must be positive when strip_count > 1");
        if (p->strip_index < 0 || p->strip_index >= p->strip_count) return fail(RT_ERR_INVALID_ARGUMENT, "strip_index out of range");
    }
    return RT_OK;
}

// SAMPLE CHUNKS.  A work item of the pooled kernel is a tile x a chunk of its samples, and the order in which a
// pixel's samples are summed follows the chunk boundaries, so they depend on the sample count ONLY (never on
// tiling, strips, batches or the device): the frame is bit-identical for every GPU count.
// Returns the start sample of every chunk plus the total (size = chunks + 1).
// * About sixteen full-length chunks per frame: every item ends in a tail of ~20 iterations in which its last
//   deep paths die out at a handful of lanes (7.5 % of C3's iterations with chunks of 32), so long chunks pay -
//   until items become too few and too long for the end of a launch to balance, which a rank's share of a
//   multi-GPU frame reaches first.  Measured on the 1080p frames with the taper below in place
//   (tools/perf_ab.sh RT_POOL_CHUNK=.., tools/strip_share.py), ms per frame / slowest of 8 shares: C3 (1024 spp)
//   full chunks of 44: 94.4 / 13.4, 64: 93.4 / 13.6, 88: 92.9 / 13.8, 128: 92.5 / 14.4 (round 1's fixed 32 without
//   taper: 96.6 / 13.9); C2 (256 spp) 16: 18.5, 24: 18.3, 32: 18.6; C4 (512 spp) 24: 59.8, 32: 59.4, 44: 59.4, 64: 59.8.
//   spp / 16, at least 24, serves one GPU and eight.
// * The last one to two chunk lengths of samples are cut into ever shorter chunks (halving down to 4 samples): items
//   are queued chunk-major, so a launch ends on small items and its waves finish together.
std::vector<int> chunk_plan(int samples) {
    int full = ((samples + 15) / 16 + 3) / 4 * 4;
    if (full < 24) full = 24;
#ifdef RT_DEVELOPER_KNOBS // changes the summation order: never in the product build
    if (const char *k = getenv("RT_POOL_CHUNK"))
        if (atoi(k) > 0) full = atoi(k);
#endif
    std::vector<int> starts;
    int at = 0;
    while (samples - at >= 2 * full && (int)starts.size() < rtdev::RT_MAX_CHUNKS - 8) {
        starts.push_back(at);
        at += full;
    }
#ifdef RT_DEVELOPER_KNOBS
    const bool taper = getenv("RT_POOL_NO_TAPER") == nullptr;
#else
    const bool taper = true;
#endif
    while (samples - at > 8 && taper) {
        starts.push_back(at);
        const int rest = samples - at;
        at += rest >= 2 * full ? full : (rest / 2 + 3) / 4 * 4; // more than 2 x full only when the chunk table is full
        if ((int)starts.size() >= rtdev::RT_MAX_CHUNKS - 1) break;
    }
    if (at < samples) starts.push_back(at);
    starts.push_back(samples);
    return starts;
}

void set_chunk_table(rtdev::TraceArgs &a, const std::vector<int> &starts) {
    const int total_chunks = (int)starts.size() - 1;
    for (int c = 0; c <= total_chunks; ++c) a.chunk_start[c] = starts[(size_t)c];
    a.chunk_samples = starts[1] - starts[0];
    a.total_chunks = total_chunks;
}

// The exponent e of the fixed-point sums (sum_scale = 2^(52-e)) for a radiance bound and a sample count, or 0: f64 sums
// (no bound, or one of kSumsBoundCap or more).  A sample's radiance is at most bound < 2^e, so T * 2^(52 - e) < 2^52 —
// what the kernel's conversion can hold — and 2048 of them, the samples of the longest chunk (or the scale halves), stay
// below 2^63.  RT_ERR_UNSUPPORTED: the halving would take e past the budget (kSumsMaxExponent).
int sum_exponent(double bound, int samples, int *e_out) {
    *e_out = 0;
    if (samples <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "samples must be positive");
    if (bound == 0.0 || !(bound < kSumsBoundCap)) return RT_OK; // (NaN and infinity included)
    // every sample can be the white of an exhausted depth: scene_radiance_bound never returns less than 1
    if (!(bound >= 1.0)) return fail(RT_ERR_INVALID_ARGUMENT, "a radiance bound is 0 or at least 1");
    int e = 0;
    // bound < 2^e, with room for the last bits a sample may exceed the bound by (a sky blend or a Noise factor an ulp
    // above 1, twenty bounces deep): a bound within 1e-6 of the power of two takes the next one
    if (frexp(bound, &e) > 1.0 - 1e-6) ++e;
    const std::vector<int> plan = chunk_plan(samples);
    int longest = 1;
    for (size_t k = 0; k + 1 < plan.size(); ++k) longest = std::max(longest, plan[k + 1] - plan[k]);
    for (; longest > 2048; longest = (longest + 1) / 2) ++e;
    if (e > kSumsMaxExponent)
        return fail(RT_ERR_UNSUPPORTED, "this many samples per pixel would coarsen the fixed-point sums of a scene this bright "
                                        "beyond the 1e-3 tolerance: render it with RT_ARITH_REFERENCE");
    *e_out = e;
    return RT_OK;
}

std::vector<Launch> plan_launches(const std::vector<int> &starts, int batch) {
    const int total_chunks = (int)starts.size() - 1;
    std::vector<Launch> plan;
    for (int c = 0; c < total_chunks;) {
        Launch l{c, 0};
        while (c < total_chunks && (l.n_chunks == 0 || starts[(size_t)c] - starts[(size_t)l.first_chunk] < batch)) {
            ++l.n_chunks;
            ++c;
        }
        plan.push_back(l);
    }
    return plan;
}

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

PreviewGrid preview_grid(const RtRenderParams *p) {
    PreviewGrid g{1, 1, p->width, p->height};
    if (p->scale > 1) { // CpuRendererScaled::new (cpu_scaled.rs:33-41) + raytrace's scaled grid (:50-52)
        auto highest_divisible = [](int value, int div) { // cpu_scaled.rs:18-24
            while (value % div != 0) --div;
            return div;
        };
        const int tw = p->tiles_w > 0 ? p->tiles_w : 1, th = p->tiles_h > 0 ? p->tiles_h : 1;
        g.step_x = highest_divisible(p->width / tw, p->scale);
        g.step_y = highest_divisible(p->height / th, p->scale);
        g.cover_w = (p->width / g.step_x) * g.step_x;
        g.cover_h = (p->height / g.step_y) * g.step_y;
    }
    return g;
}

PreviewPhase preview_phase(const PreviewGrid &g, int64_t frame_index) {
    const int64_t n = (int64_t)g.step_x * (int64_t)g.step_y;
    auto gcd = [](int64_t a, int64_t b) {
        while (b != 0) {
            const int64_t r = a % b;
            a = b;
            b = r;
        }
        return a;
    };
    int64_t stride = std::max<int64_t>(1, (5 * n + 4) / 8);
    while (gcd(stride, n) != 1) ++stride; // (n + 1 is coprime to n: the loop ends)
    const int64_t i = ((frame_index % n) * (stride % n)) % n;
    return PreviewPhase{(int)(i % g.step_x), (int)(i / g.step_x)};
}

RtCamera preview_phase_camera(const RtCamera &camera, int width, int height, int jx, int jy) {
    RtCamera out = camera;
    if (jx == 0 && jy == 0) return out; // (-0.0 + 0.0 would not be the same bits)
    const double fx = (double)jx / (double)(width - 1), fy = (double)jy / (double)(height - 1);
    for (int c = 0; c < 3; ++c) out.upper_left_corner[c] += fx * camera.horizontal[c] - fy * camera.vertical[c];
    return out;
}

void fill_grid(const RtRenderParams *p, rtdev::TraceArgs &a) {
    a.width = p->width;
    a.height = p->height;
    a.samples = p->samples;
    a.max_depth = p->max_depth;
    a.sample_begin = 0;
    a.sample_end = p->samples;
    if (p->strip_count > 1) {
        a.strip_rows = p->strip_rows;
        a.strip_count = p->strip_count;
        a.strip_index = p->strip_index;
        a.owned_rows = owned_rows_of(p);
    } else {
        a.strip_rows = p->height;
        a.strip_count = 1;
        a.strip_index = 0;
        a.owned_rows = p->height;
    }
    const PreviewGrid g = preview_grid(p);
    a.step_x = g.step_x;
    a.step_y = g.step_y;
    a.cover_w = g.cover_w;
    a.cover_h = g.cover_h;
    if (p->scale > 1) a.owned_rows = p->height / a.step_y; // grid rows
    a.seed_lo = (uint32_t)(p->seed & 0xffffffffull);
    a.seed_hi = (uint32_t)(p->seed >> 32);
    a.inv_width_m1 = 1.0 / (double)(p->width - 1);
    a.inv_height_m1 = 1.0 / (double)(p->height - 1);
}

int owned_rows_of(const RtRenderParams *p) {
    if (p->strip_count <= 1) return p->height;
    int owned_strips = 0; // strips j with first row (j*count + index)*rows inside the image
    for (long long j = 0; (j * p->strip_count + p->strip_index) * (long long)p->strip_rows < p->height; ++j) ++owned_strips;
    return owned_strips * p->strip_rows;
}

int deal_strips(const RtRenderParams *p, int n, int &strip_rows, std::vector<RtRenderParams> &params) {
    if (p->strip_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, "params->strip_* must be unset: the call assigns strips itself");
    if (p->scale > 1) return fail(RT_ERR_INVALID_ARGUMENT, "the preview scale cannot be combined with strips");
    if (strip_rows < 0) return fail(RT_ERR_INVALID_ARGUMENT, "strip_rows must not be negative");
    if (strip_rows == 0) strip_rows = 8;
    params.assign((size_t)n, *p);
    if (n > 1)
        for (int i = 0; i < n; ++i) {
            params[(size_t)i].strip_rows = strip_rows;
            params[(size_t)i].strip_count = n;
            params[(size_t)i].strip_index = i;
        }
    return RT_OK;
}

// ----------------------------------------------------------------------------------------------------------- a delivery
std::vector<rtdev::Region> frame_bands(int tile_rows, int tiles_x, int chunk_count) {
    // How many bands?  The launch ends on the LAST band's last chunks — (tiles of the band) x (a few chunks) items for
    // thousands of resident waves — so a small last band costs an unbalanced tail of about one item's duration,
    // while a large one costs the copy of its rows after the GPU is done.  Items are short when a frame has many
    // chunks (C3: 19 chunks, 0.2 ms items: 32 bands, +0.8 ms in all) and long when it has few (64 spp of a
    // 485-sphere scene: 4 chunks, 1.6 ms items: 32 bands cost +3.5 ms, 8 bands +0.7): two bands per chunk.
    int bands = tile_rows / 2; // at least two tile rows each
    const int by_chunks = 2 * chunk_count;
    if (bands > by_chunks) bands = by_chunks < 4 ? 4 : by_chunks;
    if (bands > rtdev::RT_MAX_REGIONS) bands = rtdev::RT_MAX_REGIONS;
    if (bands > tile_rows) bands = tile_rows;
    if (bands < 1) bands = 1;
    std::vector<rtdev::Region> regions;
    for (int b = 0; b < bands; ++b) {
        const int ty0 = (int)((long long)tile_rows * b / bands), ty1 = (int)((long long)tile_rows * (b + 1) / bands);
        if (ty1 > ty0) regions.push_back(rtdev::Region{0, 0, tiles_x, ty0, ty1 - ty0});
    }
    return regions;
}

// A pixel's sum depends on the order its samples meet in LDS, i.e. on which 8x8 item tile it sits in, so the
// regions are cut on the whole-frame item grid: the window of tile columns [a, b) is the pixel range
// [up8(x_a), up8(x_b)) (first from 0, last to the image edge) and holds exactly the item tiles of the
// whole-frame render; tile column k is complete once the windows up to its own are (up8(x_k+1) >= x_k+1).
// More than RT_MAX_REGIONS tile columns share regions.  A window may be empty.
StreamWindows stream_windows(int width, int tiles_w, int tile_rows) {
    const int width_step = width / tiles_w;
    auto window_begin = [&](int ws) {
        if (ws <= 0) return 0;
        if (ws >= tiles_w) return width;
        const int x = (width_step * ws + 7) & ~7;
        return x < width ? x : width;
    };
    const int per_region = (tiles_w + rtdev::RT_MAX_REGIONS - 1) / rtdev::RT_MAX_REGIONS;
    StreamWindows win;
    for (int a = 0; a < tiles_w; a += per_region) {
        const int b = a + per_region < tiles_w ? a + per_region : tiles_w;
        const int x0 = window_begin(a), x1 = window_begin(b);
        if (x1 > x0) {
            win.regions.push_back(rtdev::Region{0, x0 / 8, tiles_across(x1) - x0 / 8, 0, tile_rows});
            win.columns_after.push_back(b);
        } else if (!win.columns_after.empty()) {
            win.columns_after.back() = b; // nothing of its own to wait for
        }
    }
    if (!win.columns_after.empty()) win.columns_after.back() = tiles_w;
    if (tile_rows <= 0) win.regions.clear(); // (the share owns no rows and is not launched)
    return win;
}

int queue_order(const std::vector<rtdev::Region> &regions, int tiles_x, int n_tiles, int chunks_per_tile,
                rtdev::Region out[rtdev::RT_MAX_REGIONS], int &n_out) {
    if (regions.empty() || (int)regions.size() > rtdev::RT_MAX_REGIONS) return fail(RT_ERR_INVALID_ARGUMENT, "bad region list");
    n_out = (int)regions.size();
    uint64_t at = 0;
    for (int r = 0; r < n_out; ++r) {
        rtdev::Region reg = regions[(size_t)r];
        if (reg.ntx <= 0 || reg.nty <= 0 || reg.tx0 < 0 || reg.ty0 < 0 || reg.tx0 + reg.ntx > tiles_x ||
            (reg.ty0 + reg.nty) * tiles_x > n_tiles)
            return fail(RT_ERR_INVALID_ARGUMENT, "region outside the tile grid");
        reg.item_begin = (uint32_t)at;
        at += (uint64_t)reg.ntx * (uint64_t)reg.nty * (uint64_t)chunks_per_tile;
        out[r] = reg;
    }
    if (at != (uint64_t)n_tiles * (uint64_t)chunks_per_tile) return fail(RT_ERR_INVALID_ARGUMENT, "the regions do not tile the grid");
    return RT_OK;
}

std::vector<RowRun> copy_runs(const RtRenderParams *p, const rtdev::Region &band, int height) {
    const int owned = owned_rows_of(p);
    int vr = band.ty0 * 8, vr_end = (band.ty0 + band.nty) * 8;
    if (vr_end > owned) vr_end = owned;
    std::vector<RowRun> runs;
    while (vr < vr_end) {
        const int row = owned_row_to_image_row(p, vr);
        int run = 1;
        while (vr + run < vr_end && owned_row_to_image_row(p, vr + run) == row + run) ++run;
        if (row < height) runs.push_back(RowRun{row, row + run <= height ? run : height - row});
        vr += run;
    }
    return runs;
}

} // namespace rtapi
