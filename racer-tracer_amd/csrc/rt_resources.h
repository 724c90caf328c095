// rt_resources.h — the owning types of the library's host side: device memory, pinned host memory, a stream, an event,
// and the device a set of them lives on.  Each frees what it holds in its destructor, none can be copied, and a moved-from
// object owns nothing — so a struct of them (RenderBuffers, RtScene, RtTemporal: rt_scene.h, rt_temporal_state.h) needs no
// release list and can be moved whole.  The ONLY place in the library that allocates or frees through the HIP runtime.
// Needs nothing beyond the runtime API; private to the library.
//
// The grow rule of every buffer that a render makes on first use, once: reserve(n) grows when too small, never shrinks,
// and does not keep the contents.  With enough held already it makes no runtime call.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <utility>

namespace rtapi {

// Device memory: `count` elements at `ptr`, or nullptr and 0.
template <class T> struct DevBuf {
    T *ptr = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), count(std::exchange(o.count, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            ptr = std::exchange(o.ptr, nullptr);
            count = std::exchange(o.count, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // exactly n elements, whatever was held (the uploads of rt_scene_create.hip); empty for n == 0 and after a failure
    hipError_t alloc(size_t n) {
        release();
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc((void **)&ptr, n * sizeof(T));
        if (e == hipSuccess) count = n;
        else ptr = nullptr;
        return e;
    }
    // at least n elements (the grow rule above); *grew: the block is a new one
    hipError_t reserve(size_t n, bool *grew = nullptr) {
        if (grew) *grew = count < n;
        return count < n ? alloc(n) : hipSuccess;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
};

// Pinned host memory, the same; the hipHostMalloc* flags are given at the call.
template <class T> struct PinnedBuf {
    T *ptr = nullptr;
    size_t count = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), count(std::exchange(o.count, 0)) {}
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) {
            release();
            ptr = std::exchange(o.ptr, nullptr);
            count = std::exchange(o.count, 0);
        }
        return *this;
    }
    ~PinnedBuf() { release(); }
    hipError_t alloc(size_t n, unsigned flags) {
        release();
        if (n == 0) return hipSuccess;
        hipError_t e = hipHostMalloc((void **)&ptr, n * sizeof(T), flags);
        if (e == hipSuccess) count = n;
        else ptr = nullptr;
        return e;
    }
    hipError_t reserve(size_t n, unsigned flags, bool *grew = nullptr) {
        if (grew) *grew = count < n;
        return count < n ? alloc(n, flags) : hipSuccess;
    }
    void release() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        count = 0;
    }
};

// A stream, made by the first ensure() with that call's flags; reads as the raw handle (nullptr: not made yet).
struct Stream {
    hipStream_t handle = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : handle(std::exchange(o.handle, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept {
        if (this != &o) {
            release();
            handle = std::exchange(o.handle, nullptr);
        }
        return *this;
    }
    ~Stream() { release(); }
    hipError_t ensure(unsigned flags) {
        if (handle) return hipSuccess;
        hipError_t e = hipStreamCreateWithFlags(&handle, flags);
        if (e != hipSuccess) handle = nullptr;
        return e;
    }
    operator hipStream_t() const { return handle; }
    void release() {
        if (handle) (void)hipStreamDestroy(handle);
        handle = nullptr;
    }
};

// An event, the same.  hipEventDefault is a timing event: what hipEventElapsedTime can read.
struct Event {
    hipEvent_t handle = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : handle(std::exchange(o.handle, nullptr)) {}
    Event &operator=(Event &&o) noexcept {
        if (this != &o) {
            release();
            handle = std::exchange(o.handle, nullptr);
        }
        return *this;
    }
    ~Event() { release(); }
    hipError_t ensure(unsigned flags = hipEventDefault) {
        if (handle) return hipSuccess;
        hipError_t e = hipEventCreateWithFlags(&handle, flags);
        if (e != hipSuccess) handle = nullptr;
        return e;
    }
    operator hipEvent_t() const { return handle; }
    void release() {
        if (handle) (void)hipEventDestroy(handle);
        handle = nullptr;
    }
};

// The device the owners beside it live on, or -1: none — what a fresh set has and what a move leaves behind, so that the
// destructor of a struct that holds one makes the device current only when there may be something to free:
//     ~RenderBuffers() { device.make_current(); }     (the body runs before the members go)
struct OwnersDevice {
    int id = -1;
    OwnersDevice() = default;
    OwnersDevice(OwnersDevice &&o) noexcept : id(std::exchange(o.id, -1)) {}
    OwnersDevice &operator=(OwnersDevice &&o) noexcept {
        id = std::exchange(o.id, -1);
        return *this;
    }
    OwnersDevice &operator=(int device) {
        id = device;
        return *this;
    }
    operator int() const { return id; }
    void make_current() const {
        if (id >= 0) (void)hipSetDevice(id);
    }
};

} // namespace rtapi
