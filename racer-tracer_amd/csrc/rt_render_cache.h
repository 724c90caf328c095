// rt_render_cache.h — the render-buffer cache between rt_scene_destroy and rt_scene_create, and the steps of
// rt_scene_destroy around it.  Everything a render call allocates on first use (rt_scene.h: RenderBuffers) is kept per
// device across the two calls.  Measured on 1 x MI355X at 1080p (tools/time_scene_create.py,
// profiles/r04_scene_create.txt): rt_scene_create itself is 0.3 - 1.4 ms, but the first render of a new scene paid 3 ms of
// hipMalloc / hipHostMalloc (50 MB pinned frame, slices, counters) and the destroy before it 1 - 4 ms of hipFree /
// hipHostFree — on every object event of the reference's interactive loop.  At most two sets per device are kept (two
// scenes alive at a time is the pattern of `rebuild, then drop the old one`); rt_release_cached_buffers gives the memory
// back.  The sets are moved in and out whole, never copied.
//
// Host code without a kernel, inline so that a plain host compiler reaches it (tests/resources_driver.cpp); used by
// rt_scene_create.hip alone.  Private to the library.
#pragma once
#include <mutex>
#include <utility>
#include <vector>
#include "rt_scene.h"

namespace rtapi {

struct RenderCache {
    std::mutex mutex;
    std::vector<RenderBuffers> sets;
};
const size_t kCachedSetsPerDevice = 2;

// The one cache of the process, NEVER destroyed: it is made on first use and deliberately leaked.  Its sets own device
// memory, streams and events; as a static object it would be destroyed at process exit, and its members would call hipFree
// and hipStreamDestroy into a runtime that is being torn down (or is gone) by then.  What is still cached at exit goes with
// the process, without one runtime call.
inline RenderCache &render_cache() {
    static RenderCache *const cache = new RenderCache();
    return *cache;
}

// rt_scene_destroy: the set goes to the cache, or is freed at once when its device's slots are taken or the scene never got
// as far as creating its streams.  The slot is reserved BEFORE the set moves: should that throw, `buf` still owns everything
// and frees it, once, where it is destroyed.
inline void render_cache_put(RenderBuffers &buf) {
    if (buf.complete()) {
        RenderCache &c = render_cache();
        std::lock_guard<std::mutex> lock(c.mutex);
        size_t held = 0;
        for (const RenderBuffers &b : c.sets) held += b.device == buf.device;
        if (held < kCachedSetsPerDevice) {
            c.sets.reserve(c.sets.size() + 1);
            c.sets.push_back(std::move(buf));
            return;
        }
    }
    RenderBuffers doomed(std::move(buf)); // freed here, on its device
}

// rt_scene_create: take over a cached set of this device (the one with the largest slices), if there is one
inline bool render_cache_take(int device, RenderBuffers &into) {
    RenderCache &c = render_cache();
    std::lock_guard<std::mutex> lock(c.mutex);
    int best = -1;
    for (size_t i = 0; i < c.sets.size(); ++i)
        if (c.sets[i].device == device && (best < 0 || c.sets[i].partial.count > c.sets[(size_t)best].partial.count)) best = (int)i;
    if (best < 0) return false;
    into = std::move(c.sets[(size_t)best]);
    c.sets.erase(c.sets.begin() + best);
    return true;
}

// rt_release_cached_buffers: every cached set is freed, outside the lock
inline void render_cache_release_all() {
    std::vector<RenderBuffers> all;
    {
        RenderCache &c = render_cache();
        std::lock_guard<std::mutex> lock(c.mutex);
        all.swap(c.sets);
    }
}

// rt_scene_destroy behind its NULL check: the scene's device is made current, its two streams are idle, and what a render
// allocated — slices, frames, pinned memory, counters, streams, events — outlives the scene: the reference rebuilds its
// scene on every object event (main.rs:174-189), and the next rt_scene_create on this device takes these over instead of
// paying hipMalloc / hipHostMalloc again.  Should the cache throw, they are freed with the scene.  The scene's own tables
// free themselves.
inline void scene_destroy(RtScene *s) {
    (void)hipSetDevice(s->device);
    if (s->buf.stream) (void)hipStreamSynchronize(s->buf.stream);
    if (s->buf.stream_ctl) (void)hipStreamSynchronize(s->buf.stream_ctl);
    (void)guarded("rt_scene_destroy", [&] { render_cache_put(s->buf); return RT_OK; });
    delete s;
}

} // namespace rtapi
