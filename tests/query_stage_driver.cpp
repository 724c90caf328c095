// query_stage_driver.cpp — the chunked host form of the ray queries (racer-tracer_amd/csrc/rt_query_stage.h: stage_query) as
// a stand-alone host program, for tests/test_query_stage_cpu.py.  It is NOT linked against the HIP runtime: the runtime
// functions the header calls are defined here.  Device memory is malloc's, a copy is memcpy and fails the case when its
// device-side range does not lie inside a live device allocation, synchronisations are counted, and the j-th call can be
// made to fail.  A fake launcher stands in for the kernels: it finds every chunk ray's global index in origin.x, checks the
// planes it is handed and writes f(global ray, slot, plane, component) into each.  The staging planes hold 16 entries, so
// a multi-hit call stages 2 rays per chunk.
//
// Prints one "ok <case>" line per case and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "rt_query_stage.h"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, context); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

namespace {
char context[200] = ""; // the case at hand, for CHECK
}

// ---------------------------------------------------------------------------------------------------- the fake runtime
namespace fake {
std::map<char *, size_t> device; // live device allocations, with their bytes
long mallocs = 0, syncs = 0, copies = 0;
long calls = 0;    // hipMalloc + hipMemcpyAsync + hipStreamSynchronize since arm()
long fail_at = 0;  // that call (1-based) fails; 0: none
bool failed = false, went_on = false; // a call failed; something was called or launched behind it

void arm(long k) {
    calls = 0;
    fail_at = k;
    failed = went_on = false;
}
// true: this call is the one to fail
bool called() {
    if (failed) went_on = true;
    ++calls;
    if (fail_at && calls == fail_at) failed = true;
    return fail_at && calls == fail_at;
}
bool on_device(const void *p, size_t bytes) {
    for (const auto &a : device)
        if ((const char *)p >= a.first && (const char *)p + bytes <= a.first + a.second) return true;
    return false;
}
bool touches_device(const void *p, size_t bytes) {
    for (const auto &a : device)
        if ((const char *)p < a.first + a.second && (const char *)p + bytes > a.first) return true;
    return false;
}
} // namespace fake

extern "C" {
hipError_t hipMalloc(void **ptr, size_t size) {
    if (fake::called()) {
        *ptr = (void *)0x1; // a runtime may leave anything behind on failure: the owners must not keep it
        return hipErrorOutOfMemory;
    }
    ++fake::mallocs;
    char *p = (char *)malloc(size ? size : 1);
    memset(p, 0xA5, size);
    fake::device[p] = size;
    *ptr = p;
    return hipSuccess;
}
hipError_t hipFree(void *ptr) {
    if (!fake::device.count((char *)ptr)) {
        fprintf(stderr, "hipFree of %p that is not live\n", ptr);
        abort();
    }
    fake::device.erase((char *)ptr);
    free(ptr);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    if (fake::called()) return hipErrorInvalidValue;
    ++fake::copies;
    const bool up = kind == hipMemcpyHostToDevice;
    CHECK(up || kind == hipMemcpyDeviceToHost);
    CHECK(stream != nullptr && bytes > 0);
    CHECK(fake::on_device(up ? dst : src, bytes));        // the device side: inside ONE live allocation
    CHECK(!fake::touches_device(up ? src : dst, bytes));  // the host side: the caller's memory
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    if (fake::called()) return hipErrorInvalidValue;
    CHECK(stream != nullptr);
    ++fake::syncs;
    return hipSuccess;
}
// (what the owners of rt_resources.h need beside these; a RenderBuffers here holds one stream and device memory)
hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int) {
    *stream = (hipStream_t)malloc(1);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) {
    free((void *)stream);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **, size_t, unsigned int) { abort(); }
hipError_t hipHostFree(void *) { abort(); }
hipError_t hipEventCreateWithFlags(hipEvent_t *, unsigned) { abort(); }
hipError_t hipEventDestroy(hipEvent_t) { abort(); }
hipError_t hipSetDevice(int) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "the fake runtime says no"; }
}

// ------------------------------------------------------------------------------------------------------------ the cases
namespace {
using rtapi::RenderBuffers;

const size_t kPlane = 16, kGuard = 5;
const double kUntouchedF = -77.5;
const int32_t kUntouchedI = -7777;
const int kWidth[7] = {1, 3, 3, 2, 1, 1, 1}; // t, point, normal, uv | prim, obj_id, front_face

// what the launcher writes: exact in a double and in an int32 for every ray, slot, plane and component of the cases
double f(size_t ray, size_t slot, int plane, int c) { return (double)(((ray * 8 + slot) * 8 + (size_t)plane) * 4 + (size_t)c + 1); }
int32_t per_ray_value(size_t ray) { return (int32_t)(900000 + ray); }
// what the caller's rays hold
double ray_value(int plane, size_t ray, int c) { return plane == 0 && c == 0 ? (double)ray : 1000.0 * (plane + 1) + 4.0 * (double)ray + c + 0.25; }

// A caller's plane of `count` entries between two guard regions.
template <class T> struct Guarded {
    std::vector<T> v;
    T untouched;
    Guarded(size_t count, T fill) : v(count + 2 * kGuard, fill), untouched(fill) {}
    T *data() { return v.data() + kGuard; }
    size_t size() const { return v.size() - 2 * kGuard; }
    bool guards_untouched() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (v[i] != untouched || v[v.size() - 1 - i] != untouched) return false;
        return true;
    }
};

struct Case {
    size_t n, k, slots;
    unsigned hit_mask;   // bit p: hit plane p is given (0 with has_hits: an RtRayHits of NULLs)
    bool has_hits;       // false: no RtRayHits at all (occlusion)
    unsigned ray_mask;   // bit 0 t_min, 1 t_max, 2 time
    bool per_ray;
};

struct Launches {
    const Case *c = nullptr;
    const RenderBuffers *b = nullptr;
    size_t next = 0; // the global index the next chunk begins with
    long count = 0;
};

// The fake kernel launch of one chunk.
hipError_t launch(Launches &l, const RtRays &dr, const RtRayHits &dh, int32_t *ints, int m_) {
    if (fake::failed) fake::went_on = true;
    const Case &c = *l.c;
    const size_t m = (size_t)m_, chunk = kPlane / c.slots;
    ++l.count;
    CHECK(m_ > 0 && m <= chunk && l.next + m <= c.n && (m == chunk || l.next + m == c.n));
    const double *ray_planes[5] = {dr.origin, dr.direction, dr.t_min, dr.t_max, dr.time};
    for (int p = 0; p < 5; ++p) {
        const bool given = p < 2 || (c.ray_mask >> (p - 2) & 1);
        CHECK((ray_planes[p] != nullptr) == given);
        if (!given) continue;
        const int width = p < 2 ? 3 : 1;
        CHECK(fake::on_device(ray_planes[p], m * width * sizeof(double)));
        for (size_t i = 0; i < m; ++i)
            for (int comp = 0; comp < width; ++comp) CHECK(ray_planes[p][i * width + comp] == ray_value(p, l.next + i, comp));
    }
    void *hit_planes[7] = {dh.t, dh.point, dh.normal, dh.uv, dh.prim, dh.obj_id, dh.front_face};
    for (int p = 0; p < 7; ++p) {
        const bool given = c.has_hits && (c.hit_mask >> p & 1);
        CHECK((hit_planes[p] != nullptr) == given);
        if (!given) continue;
        const size_t width = (size_t)kWidth[p];
        CHECK(fake::on_device(hit_planes[p], c.k * m * width * (p < 4 ? sizeof(double) : sizeof(int32_t))));
        for (size_t j = 0; j < c.k; ++j)
            for (size_t i = 0; i < m; ++i)
                for (size_t comp = 0; comp < width; ++comp) {
                    const size_t e = (j * m + i) * width + comp; // slot-major over the chunk's own rays
                    const double value = f((size_t)dr.origin[3 * i], j, p, (int)comp);
                    if (p < 4) ((double *)hit_planes[p])[e] = value;
                    else ((int32_t *)hit_planes[p])[e] = (int32_t)value;
                }
    }
    CHECK((ints != nullptr) == c.per_ray);
    if (ints) {
        CHECK(fake::on_device(ints, m * sizeof(int32_t)));
        for (size_t i = 0; i < m; ++i) ints[i] = per_ray_value((size_t)dr.origin[3 * i]);
    }
    l.next += m;
    return hipSuccess;
}

// One call of stage_query for `c` on `b`, every answer checked -> the calls it made of the runtime.  With fail_at > 0 that
// runtime call fails: the error must come back and nothing may be called or launched behind it.
long run(RenderBuffers &b, const Case &c, long fail_at = 0) {
    snprintf(context, sizeof context, "n %zu k %zu slots %zu hits %d mask %#x rays %#x per_ray %d fail_at %ld", c.n, c.k, c.slots, (int)c.has_hits,
             c.hit_mask, c.ray_mask, (int)c.per_ray, fail_at);
    std::vector<Guarded<double>> ray_planes;
    for (int p = 0; p < 5; ++p) {
        ray_planes.emplace_back(c.n * (p < 2 ? 3 : 1), kUntouchedF);
        for (size_t r = 0; r < c.n; ++r)
            for (int comp = 0; comp < (p < 2 ? 3 : 1); ++comp) ray_planes[p].data()[r * (p < 2 ? 3 : 1) + comp] = ray_value(p, r, comp);
    }
    RtRays rays = {ray_planes[0].data(), ray_planes[1].data(), c.ray_mask & 1 ? ray_planes[2].data() : nullptr,
                   c.ray_mask & 2 ? ray_planes[3].data() : nullptr, c.ray_mask & 4 ? ray_planes[4].data() : nullptr};
    std::vector<Guarded<double>> doubles;
    std::vector<Guarded<int32_t>> ints;
    for (int p = 0; p < 4; ++p) doubles.emplace_back(c.k * c.n * kWidth[p], kUntouchedF);
    for (int p = 4; p < 7; ++p) ints.emplace_back(c.k * c.n, kUntouchedI);
    auto given = [&](int p) { return c.has_hits && (c.hit_mask >> p & 1); };
    RtRayHits hits = {given(0) ? doubles[0].data() : nullptr, given(1) ? doubles[1].data() : nullptr, given(2) ? doubles[2].data() : nullptr,
                      given(3) ? doubles[3].data() : nullptr, given(4) ? ints[0].data() : nullptr,   given(5) ? ints[1].data() : nullptr,
                      given(6) ? ints[2].data() : nullptr};
    Guarded<int32_t> per_ray(c.n, kUntouchedI);

    Launches l;
    l.c = &c;
    l.b = &b;
    const long syncs = fake::syncs;
    fake::arm(fail_at);
    const int rc = rtapi::stage_query(b, kPlane, &rays, c.n, c.has_hits ? &hits : nullptr, c.k, c.slots, c.per_ray ? per_ray.data() : nullptr,
                                      [&](const RtRays &dr, const RtRayHits &dh, int32_t *dev_ints, int m) { return launch(l, dr, dh, dev_ints, m); });
    const long calls = fake::calls;
    fake::fail_at = 0;
    // whatever happened: nothing outside the caller's planes, and the rays as they were
    for (int p = 0; p < 5; ++p) {
        CHECK(ray_planes[p].guards_untouched());
        for (size_t r = 0; r < c.n; ++r) CHECK(ray_planes[p].data()[r * (p < 2 ? 3 : 1)] == ray_value(p, r, 0));
    }
    for (auto &g : doubles) CHECK(g.guards_untouched());
    for (auto &g : ints) CHECK(g.guards_untouched());
    CHECK(per_ray.guards_untouched());
    if (fail_at) {
        CHECK(fake::failed && !fake::went_on && rc == RT_ERR_HIP);
        return calls;
    }
    CHECK(rc == RT_OK && !fake::failed);
    const size_t chunk = kPlane / c.slots;
    CHECK(l.next == c.n && l.count == (long)((c.n + chunk - 1) / chunk));
    CHECK(fake::syncs == syncs + 1); // ONE synchronisation per call
    for (int p = 0; p < 7; ++p)
        for (size_t e = 0; e < c.k * c.n * (size_t)kWidth[p]; ++e) {
            const size_t comp = e % kWidth[p], r = e / kWidth[p] % c.n, j = e / kWidth[p] / c.n; // slot-major: entry j * n + r
            if (p < 4) CHECK(doubles[p].data()[e] == (given(p) ? f(r, j, p, (int)comp) : kUntouchedF));
            else CHECK(ints[p - 4].data()[e] == (given(p) ? (int32_t)f(r, j, p, (int)comp) : kUntouchedI));
        }
    for (size_t r = 0; r < c.n; ++r) CHECK(per_ray.data()[r] == (c.per_ray ? per_ray_value(r) : kUntouchedI));
    return calls;
}

const unsigned kHitSets[3] = {0x7f, 0x21, 0x00}; // every plane; t and obj_id; none
const unsigned kRaySets[3] = {0x7, 0x0, 0x4};    // t_min, t_max and time; none; time alone

void ok(const char *name) {
    CHECK(fake::device.empty()); // every case leaves nothing behind
    printf("ok %s\n", name);
}

void make_stream(RenderBuffers &b) {
    context[0] = 0;
    CHECK(b.stream.ensure(hipStreamNonBlocking) == hipSuccess);
}
} // namespace

int main() {
    const size_t sizes[5] = {1, 15, 16, 17, 35};
    {
        RenderBuffers b;
        make_stream(b);
        for (size_t n : sizes)
            for (unsigned hit_mask : kHitSets)
                for (unsigned ray_mask : kRaySets) run(b, Case{n, 1, 1, hit_mask, true, ray_mask, false});
        // what rt_trace_rays has always reserved, once
        CHECK(fake::mallocs == 3 && b.rays_in.count == 9 * kPlane && b.rays_out.count == 9 * kPlane && b.rays_ids.count == 3 * kPlane);
    }
    ok("closest");
    {
        RenderBuffers b;
        make_stream(b);
        const long mallocs = fake::mallocs;
        for (size_t n : sizes)
            for (unsigned ray_mask : kRaySets) run(b, Case{n, 1, 1, 0, false, ray_mask, true});
        // no hit planes: rays_out is not reserved
        CHECK(fake::mallocs == mallocs + 2 && b.rays_in.count == 9 * kPlane && b.rays_out.ptr == nullptr && b.rays_ids.count == 3 * kPlane);
    }
    ok("occlusion");
    {
        RenderBuffers b;
        make_stream(b);
        const long mallocs = fake::mallocs;
        const size_t ns[4] = {1, 2, 3, 5}, ks[3] = {1, 3, 8};
        for (size_t n : ns)
            for (size_t k : ks)
                for (int with_count = 0; with_count < 2; ++with_count)
                    for (unsigned hit_mask : kHitSets)
                        for (unsigned ray_mask : kRaySets) run(b, Case{n, k, 8, hit_mask, true, ray_mask, with_count != 0});
        // exactly what rt_trace_rays reserves: the counts found room behind the rays' planes
        CHECK(fake::mallocs == mallocs + 3 && b.rays_in.count == 9 * kPlane && b.rays_out.count == 9 * kPlane && b.rays_ids.count == 3 * kPlane);
    }
    ok("multihit");
    {
        // the three queries on one scene's buffers, in the order that reserves least first: each later call finds what it
        // needs or adds the one buffer it lacks, and a second round allocates nothing and moves nothing
        RenderBuffers b;
        make_stream(b);
        const Case occlusion{17, 1, 1, 0, false, 0x7, true}, multi{5, 8, 8, 0x7f, true, 0x4, true}, closest{35, 1, 1, 0x7f, true, 0x0, false};
        long mallocs = fake::mallocs;
        run(b, occlusion);
        CHECK(fake::mallocs == mallocs + 2);
        run(b, multi);
        CHECK(fake::mallocs == mallocs + 3);
        run(b, closest);
        CHECK(fake::mallocs == mallocs + 3);
        const void *in = b.rays_in.ptr, *out = b.rays_out.ptr, *ids = b.rays_ids.ptr;
        run(b, occlusion);
        run(b, multi);
        run(b, closest);
        CHECK(fake::mallocs == mallocs + 3 && b.rays_in.ptr == in && b.rays_out.ptr == out && b.rays_ids.ptr == ids);
    }
    ok("second_call_allocates_nothing");
    {
        // every runtime call of a call over three chunks fails in turn, the three allocations of fresh buffers included
        const Case c{5, 3, 8, 0x7f, true, 0x7, true};
        long total = 0;
        {
            RenderBuffers b;
            make_stream(b);
            total = run(b, c);
        }
        CHECK(total == 3 + 3 * (5 + 7 * 3 + 1) + 1);
        for (long j = 1; j <= total; ++j) {
            RenderBuffers b;
            make_stream(b);
            CHECK(run(b, c, j) == j);
            context[0] = 0;
            CHECK(b.rays_in.ptr != (double *)0x1 && b.rays_out.ptr != (double *)0x1 && b.rays_ids.ptr != (int32_t *)0x1);
        }
        // ... and of an occlusion call on buffers it finds made
        RenderBuffers b;
        make_stream(b);
        const Case o{17, 1, 1, 0, false, 0x0, true};
        total = run(b, o);
        CHECK(total == 2 + 2 * (2 + 1) + 1);
        for (long j = 1; j <= total - 2; ++j) CHECK(run(b, o, j) == j);
        run(b, o); // usable after every failure
    }
    ok("failing_runtime_call");
    return 0;
}
