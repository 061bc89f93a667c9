// qpsk_hip_host.h -- what the library's host code shares around the HIP
// runtime: owning handles for device memory, pinned host memory, events and
// streams, the device-index check and the `err` out-parameter.  Every hipFree,
// hipHostFree, hipEventDestroy and hipStreamDestroy of the library is in this
// file: a context's members release themselves, in reverse order of their
// declaration, so no translation unit keeps a release list.
// Host only, and never included from qpsk_rx.hip: an edit here leaves
// qpsk_kernel_hash() alone.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

#include <atomic>

#include "qpsk_batch.h"
#include "qpsk_herr.h"

// Handles alive in the process (tests: a destroyed or half-created context
// leaves none behind).  Internal, not part of the C-ABI in include/.
extern "C" long qpsk_hip_live_handles(void);

namespace qhip {

// bumped by every successful allocation or creation below, dropped by its release
inline std::atomic<long> g_live{0};

inline hipError_t dev_alloc(void** p, size_t n) { return hipMalloc(p, n); }
inline hipError_t dev_free(void* p) { return hipFree(p); }
inline hipError_t pin_alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
inline hipError_t pin_free(void* p) { return hipHostFree(p); }

// Memory of cap() T's, device (DevBuf) or pinned host (PinBuf), that only grows
template <class T, hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { (void)release(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }
    // At least n elements.  A buffer that has to grow is released first (the
    // contents are not kept; the caller has waited for whatever still uses
    // them), and a failed allocation leaves it empty.
    hipError_t reserve(size_t n) {
        if (n <= cap_) return hipSuccess;
        (void)release();
        const hipError_t e = Alloc(reinterpret_cast<void**>(&p_), sizeof(T) * n);
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = n, g_live++;
        return e;
    }
    hipError_t release() {
        const hipError_t e = p_ ? Free(p_) : hipSuccess;
        if (p_) g_live--;
        p_ = nullptr;
        cap_ = 0;
        return e;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <class T> using DevBuf = Buf<T, dev_alloc, dev_free>;
template <class T> using PinBuf = Buf<T, pin_alloc, pin_free>;

// An event or a stream, null until create()
template <class H, hipError_t (*Destroy)(H)>
class Handle {
public:
    Handle() = default;
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() { if (h_) (void)Destroy(h_), g_live--; }
    operator H() const { return h_; }

protected:
    hipError_t made(hipError_t e) {
        if (e != hipSuccess) h_ = nullptr;
        else g_live++;
        return e;
    }
    H h_ = nullptr;
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { return made(hipEventCreateWithFlags(&h_, flags)); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {   // non-blocking
    hipError_t create() { return made(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking)); }
};

// `device` names a HIP device of this machine (else: QPSK_ENODEV)
inline bool device_ok(int device) {
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev;
}

// A create function's `int* err` out-parameter, which the caller may leave
// null; fail() returns nullptr, so a failure is `return fail(err, QPSK_E...)`.
inline void set_err(int* err, int code) { if (err) *err = code; }
inline std::nullptr_t fail(int* err, int code) { return set_err(err, code), nullptr; }

}  // namespace qhip
