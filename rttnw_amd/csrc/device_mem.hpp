// device_mem.hpp — who frees what on the device: one owning buffer type (DevBuf), events and streams that destroy themselves, and a
// guard that makes the current device current again.  Host code of the HIP translation units only: tests/hostsim compiles
// bvh_build.hpp, scene_lower.hpp and scene_handle.hpp without HIP, so none of those includes this.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

namespace rt {

// The current device on entry, made current again on exit.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { (void)hipGetDevice(&prev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

struct DeviceFree { // frees on the device the buffer lives on
    int device;
    void operator()(void* p) const {
        if (!p) return;
        DeviceGuard restore;
        if (restore.prev != device) (void)hipSetDevice(device);
        (void)hipFree(p);
    }
};

// A device buffer, owned by `mem`: freed on the device it was made on once the last owner lets go.  A buffer made elsewhere on the
// device (a device-built tree, bvh_build.hpp DeviceTree) is adopted by sharing its owner, and a copy of a DevBuf is one more owner,
// never a second free.  `p` is the buffer, `n` its elements.  Every call that replaces the buffer lets go of the old one first.
template <typename T> struct DevBuf {
    std::shared_ptr<void> mem;
    T* p = nullptr;
    size_t n = 0;

    hipError_t alloc(size_t count) { return alloc_bytes(std::max<size_t>(count, 1) * sizeof(T), count); }
    template <typename A> hipError_t upload(const std::vector<T, A>& v) {
        // (the size rounded up to 32 bytes: the LDS staging of small record arrays copies whole 32-byte units)
        hipError_t e = alloc_bytes((std::max<size_t>(v.size(), 1) * sizeof(T) + 31) / 32 * 32, v.size());
        if (e == hipSuccess && !v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    // A workspace kept at its high-water mark (n = bytes)
    hipError_t grow(size_t bytes) {
        static_assert(sizeof(T) == 1, "grow() sizes byte buffers");
        if (p && n >= bytes) return hipSuccess;
        return alloc_bytes(std::max<size_t>(bytes, 16), bytes);
    }
    void adopt(std::shared_ptr<void> buf, size_t count) {
        p = static_cast<T*>(buf.get());
        n = count;
        mem = std::move(buf);
    }

  private:
    hipError_t alloc_bytes(size_t bytes, size_t count) {
        *this = DevBuf();
        int device = -1;
        void* q = nullptr;
        hipError_t e = hipGetDevice(&device);
        if (e == hipSuccess) e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        mem = std::shared_ptr<void>(q, DeviceFree{device});
        p = static_cast<T*>(q);
        n = count;
        return hipSuccess;
    }
};

// A caller's host array to a fresh buffer of exactly `count` elements (DevBuf::upload is the padded form for record vectors)
template <typename T> hipError_t upload(DevBuf<T>& b, const T* src, size_t count) {
    hipError_t e = b.alloc(count);
    if (e == hipSuccess) e = hipMemcpy(b.p, src, count * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

inline hipError_t create_event(Event& out, unsigned flags = hipEventDefault) {
    hipEvent_t e = nullptr;
    const hipError_t r = hipEventCreateWithFlags(&e, flags);
    if (r == hipSuccess) out.reset(e);
    return r;
}
inline hipError_t create_stream(Stream& out, unsigned flags) {
    hipStream_t s = nullptr;
    const hipError_t r = hipStreamCreateWithFlags(&s, flags);
    if (r == hipSuccess) out.reset(s);
    return r;
}

} // namespace rt
