// dev_raii.h -- owners of device memory and of events: HIPCHK, DevBuf<T>, DevEvent, DevTimer.  Nothing else belongs here (no allocator, no pool, no generic handle).
// A DevBuf or a DevEvent must NEVER sit in an object with static or thread_local storage: its destructor would call HIP while the process exits, behind the
// runtime's own teardown, and that is the known exit crash.  calib.hip's monitor map and plan.hip's per-thread objects therefore keep raw handles.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace rvc {

// a failed call also stays behind as HIP's "last error"; taken off here, a refused allocation does not fail the next call's HIPCHK(hipGetLastError())
static inline hipError_t forget_failure(hipError_t rc) { if (rc != hipSuccess) (void)hipGetLastError(); return rc; }

// one hipMalloc allocation of T elements
template <typename T> class DevBuf {
public:
    DevBuf() = default;
    explicit DevBuf(T *adopted) : p_(adopted) {}
    DevBuf(DevBuf &&o) noexcept : p_(o.release()) {}
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.release(); } return *this; }
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    // n elements in place of what the buffer held; throws, and then holds nothing
    void alloc(size_t n) { reset(); T *p = nullptr; HIPCHK(forget_failure(hipMalloc(&p, n * sizeof(T)))); p_ = p; }
    T *get() const { return p_; }
    T *release() { T *p = p_; p_ = nullptr; return p; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    explicit operator bool() const { return p_ != nullptr; }
private:
    T *p_ = nullptr;
};

// an event, created on first use
class DevEvent {
public:
    DevEvent() = default;
    DevEvent(DevEvent &&o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
    DevEvent &operator=(DevEvent &&o) noexcept { if (this != &o) { destroy(); ev_ = o.ev_; o.ev_ = nullptr; } return *this; }
    DevEvent(const DevEvent &) = delete; DevEvent &operator=(const DevEvent &) = delete;
    ~DevEvent() { destroy(); }
    hipEvent_t get() { if (!ev_) HIPCHK(hipEventCreate(&ev_)); return ev_; }
    void record(hipStream_t s) { HIPCHK(hipEventRecord(get(), s)); }
private:
    void destroy() { if (ev_) (void)hipEventDestroy(ev_); ev_ = nullptr; }
    hipEvent_t ev_ = nullptr;
};

// device time between two points of a stream; ms() once both events have completed
struct DevTimer {
    DevEvent a, b;
    void start(hipStream_t s) { a.record(s); }
    void stop(hipStream_t s) { b.record(s); }
    float ms() { float v = 0.f; HIPCHK(hipEventElapsedTime(&v, a.get(), b.get())); return v; }
};

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && std::is_nothrow_move_constructible<DevBuf<float>>::value, "DevBuf moves, never copies");
static_assert(!std::is_copy_constructible<DevEvent>::value && std::is_nothrow_move_constructible<DevEvent>::value, "DevEvent moves, never copies");

}  // namespace rvc
