// Answers questions about the device-free rules of racer-tracer_amd/csrc/rt_plan.h, one command per line on standard input:
//   chunks N                       -> chunk_plan(N), the boundaries on one line
//   passes N P                     -> pass_ends over chunk_plan(N) as samples done per pass (what rtdev_progressive_passes gives)
//   sumexp BOUND N                 -> "rc e" of sum_exponent (BOUND in any of strtod's forms)
//   select FILE                    -> "rc prims_class textured specular has_moving bound" (bound as a hexadecimal float)
//   tables FILE MAX_LIGHTS         -> the linear-loop tables of a description, seven lines:
//                                     ends: rect_end[3] sphere_end box_end / order / obj_id of every record / whether every
//                                     record is pack_prims' record of order[j] / lights / slot / prim
//   leaves FILE                    -> leaf_geometry of the packed table in description order: the tags, then "time_a inv_dt"
//   grid W H STRIP_ROWS STRIP_COUNT STRIP_INDEX SCALE TILES_W TILES_H
//                                  -> fill_grid: "owned_rows owned_rows_of step_x step_y cover_w cover_h strip_rows
//                                     strip_count strip_index", then owned_row_to_image_row of every owned row
// FILE holds a description as the library gets it: the bytes of an RtSceneDesc, then its primitive, material, texture,
// image and Perlin tables (n_* records each); the pointers are set here.  Host code only: rt_plan.cpp, rt_error.cpp and
// rt_bvh.cpp need no HIP (tests/test_plan_cpu.py compiles them with g++, tests/test_host_sanitizers.py under sanitizers).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rt_plan.h"

namespace {

struct Desc {
    RtSceneDesc d;
    std::vector<RtPrimitive> primitives;
    std::vector<RtMaterial> materials;
    std::vector<RtTexture> textures;
    std::vector<RtImage> images;
    std::vector<RtPerlin> perlins;
};

template <class T> bool read_table(FILE *f, std::vector<T> &table, int32_t n, const T *&ptr) {
    if (n < 0) return false;
    table.resize((size_t)n);
    if (n > 0 && fread(table.data(), sizeof(T), (size_t)n, f) != (size_t)n) return false;
    ptr = n > 0 ? table.data() : nullptr;
    return true;
}

bool load(const char *path, Desc &s) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    bool ok = fread(&s.d, sizeof s.d, 1, f) == 1 && read_table(f, s.primitives, s.d.n_primitives, s.d.primitives) &&
              read_table(f, s.materials, s.d.n_materials, s.d.materials) && read_table(f, s.textures, s.d.n_textures, s.d.textures) &&
              read_table(f, s.images, s.d.n_images, s.d.images) && read_table(f, s.perlins, s.d.n_perlins, s.d.perlins);
    ok = ok && fgetc(f) == EOF; // (nothing may be left over)
    fclose(f);
    return ok;
}

void print(const char *label, const std::vector<int32_t> &v) {
    printf("%s", label);
    for (int32_t x : v) printf(" %d", x);
    printf("\n");
}

} // namespace

int main() {
    char line[4096], cmd[32], path[4000];
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%31s", cmd) != 1) continue;
        const char *rest = line + strlen(cmd);
        int a = 0, b = 0;
        if (!strcmp(cmd, "chunks") && sscanf(rest, "%d", &a) == 1) {
            print("chunks", rtapi::chunk_plan(a));
        } else if (!strcmp(cmd, "passes") && sscanf(rest, "%d %d", &a, &b) == 2) {
            const std::vector<int> starts = rtapi::chunk_plan(a);
            std::vector<int32_t> done;
            for (int e : rtapi::pass_ends(starts, b)) done.push_back(starts[(size_t)e]);
            print("passes", done);
        } else if (!strcmp(cmd, "sumexp")) {
            char *end = nullptr;
            const double bound = strtod(rest, &end);
            if (end == rest || sscanf(end, "%d", &a) != 1) return 2;
            int e = -1;
            const int rc = rtapi::sum_exponent(bound, a, &e);
            printf("sumexp %d %d\n", rc, e);
        } else if (!strcmp(cmd, "select") && sscanf(rest, "%3999s", path) == 1) {
            Desc s;
            if (!load(path, s)) return 3;
            const int rc = rtapi::validate_desc(&s.d);
            if (rc != RT_OK) {
                printf("select %d\n", rc);
                continue;
            }
            const rtapi::Selection sel = rtapi::select_variant(&s.d);
            printf("select 0 %d %d %d %d %a\n", sel.prims_class, sel.textured, sel.specular, sel.has_moving, rtapi::scene_radiance_bound(&s.d));
        } else if (!strcmp(cmd, "tables") && sscanf(rest, "%3999s %d", path, &a) == 2) {
            Desc s;
            if (!load(path, s) || rtapi::validate_desc(&s.d) != RT_OK) return 3;
            const std::vector<rtdev::Prim> packed = rtapi::pack_prims(&s.d);
            std::vector<rtdev::Prim> prims = packed;
            std::vector<int32_t> order(prims.size());
            for (size_t j = 0; j < order.size(); ++j) order[j] = (int32_t)j;
            const rtapi::LinearGroups g = rtapi::group_linear_table(prims, order);
            printf("ends %d %d %d %d %d\n", g.rect_end[0], g.rect_end[1], g.rect_end[2], g.sphere_end, g.box_end);
            print("order", order);
            std::vector<int32_t> ids, same;
            for (size_t j = 0; j < prims.size(); ++j) {
                ids.push_back(prims[j].obj_id);
                const bool in_range = order[j] >= 0 && (size_t)order[j] < packed.size();
                same.push_back(in_range && memcmp(&prims[j], &packed[(size_t)order[j]], sizeof(rtdev::Prim)) == 0);
            }
            print("obj_id", ids);
            print("same", same);
            const rtapi::LightTables t = rtapi::light_tables(&s.d, order, a);
            print("lights", t.lights);
            print("slot", t.slot);
            print("prim", t.prim);
        } else if (!strcmp(cmd, "leaves") && sscanf(rest, "%3999s", path) == 1) {
            Desc s;
            if (!load(path, s) || rtapi::validate_desc(&s.d) != RT_OK) return 3;
            const rtapi::LeafTable t = rtapi::leaf_geometry(rtapi::pack_prims(&s.d));
            std::vector<int32_t> tags;
            for (const rtdev::LeafGeo &g : t.geo) tags.push_back((int32_t)g.tag);
            print("tags", tags);
            printf("interval %a %a\n", t.time_a, t.inv_dt);
        } else if (!strcmp(cmd, "grid")) {
            RtRenderParams p;
            memset(&p, 0, sizeof p);
            p.samples = 1;
            if (sscanf(rest, "%d %d %d %d %d %d %d %d", &p.width, &p.height, &p.strip_rows, &p.strip_count, &p.strip_index, &p.scale,
                       &p.tiles_w, &p.tiles_h) != 8)
                return 2;
            RtCamera camera;
            memset(&camera, 0, sizeof camera);
            if (rtapi::check_params(&camera, &p) != RT_OK) return 4;
            rtdev::TraceArgs args;
            memset(&args, 0, sizeof args);
            rtapi::fill_grid(&p, args);
            printf("grid %d %d %d %d %d %d %d %d %d\n", args.owned_rows, rtapi::owned_rows_of(&p), args.step_x, args.step_y, args.cover_w,
                   args.cover_h, args.strip_rows, args.strip_count, args.strip_index);
            std::vector<int32_t> rows;
            for (int vr = 0; vr < args.owned_rows; ++vr) rows.push_back(rtapi::owned_row_to_image_row(&p, vr));
            print("rows", rows);
        } else {
            return 2; // an unknown or malformed command
        }
    }
    return 0;
}
