// hip_buffer.h — host only: HIP_OK, the owned buffers of the host driver (device memory, pinned host memory, mapped host memory) and its owned event pair.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../../include/rustlight_amd.h"

void rl_set_error(const std::string& s);

#define HIP_OK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            rl_set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                           \
            (void)hipGetLastError();   /* the error is reported here; do not leave it for the next call */ \
            return RL_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)

namespace rl {

// Pinned and Mapped are host memory, zeroed whenever they are (re)allocated; Mapped is also visible to the device (coherent) at device_ptr().
enum class Mem { Device, Pinned, Mapped };

// One allocation of T's, freed with the buffer (on the calling thread's current device).  ensure(n) keeps it when it holds at least n elements, else frees it
// first and allocates max(n, 1): capacity() is then n, and 0 until an allocation has succeeded.
template <typename T, Mem M = Mem::Device>
class HipBuffer {
public:
    HipBuffer() = default;
    HipBuffer(HipBuffer&& o) noexcept : p_(o.p_), d_(o.d_), n_(o.n_) { o.p_ = o.d_ = nullptr; o.n_ = 0; }
    HipBuffer& operator=(HipBuffer&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; d_ = o.d_; n_ = o.n_; o.p_ = o.d_ = nullptr; o.n_ = 0; }
        return *this;
    }
    HipBuffer(const HipBuffer&) = delete;
    HipBuffer& operator=(const HipBuffer&) = delete;
    ~HipBuffer() { reset(); }

    int ensure(size_t n) {
        if (n_ >= n && p_) return RL_OK;
        reset();
        T** p = &p_;
        if (M == Mem::Device) {
            HIP_OK(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)));
        } else {
            HIP_OK(hipHostMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T), M == Mem::Mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault));
            std::memset(p_, 0, std::max<size_t>(n, 1) * sizeof(T));
            if (M == Mem::Mapped) HIP_OK(hipHostGetDevicePointer((void**)&d_, p_, 0));
        }
        n_ = n;
        return RL_OK;
    }
    void reset() {
        if (p_) { if (M == Mem::Device) (void)hipFree(p_); else (void)hipHostFree(p_); }
        p_ = d_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    T* device_ptr() const { return d_; }
    size_t capacity() const { return n_; }

private:
    T* p_ = nullptr;
    T* d_ = nullptr;     // Mapped: the device's address of p_
    size_t n_ = 0;
};

// Two events around the launches of a call that has no RenderFrame.  After open(false) every member does nothing; add(), after a synchronisation, adds the time to ms.
struct __attribute__((visibility("hidden"))) EventPair {      // (host-internal, like the driver's other helpers: not a symbol of the library)
    hipEvent_t e[2] = {nullptr, nullptr};
    float ms = 0.0f;
    int open(bool timing) {
        if (timing) { HIP_OK(hipEventCreate(&e[0])); HIP_OK(hipEventCreate(&e[1])); }
        return RL_OK;
    }
    void begin(hipStream_t st) { if (e[0]) (void)hipEventRecord(e[0], st); }
    void end(hipStream_t st) { if (e[1]) (void)hipEventRecord(e[1], st); }
    void add() { float t = 0.0f; if (e[1] && hipEventElapsedTime(&t, e[0], e[1]) == hipSuccess) ms += t; (void)hipGetLastError(); }
    ~EventPair() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); (void)hipGetLastError(); }
};

}  // namespace rl
