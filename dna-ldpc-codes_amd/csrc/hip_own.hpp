// hip_own.hpp -- owning handles for the HIP objects of the host code: device
// and pinned host memory, events, streams.  Each is a std::unique_ptr with a
// deleter; the helpers (allocation, the blocking copies up and down, a kernel
// launch) return LDPC_* codes and set the thread-local error as LDPC_HIP does.
// No device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ldpc_amd.h"

namespace ldpc {

// thread-local error string behind ldpc_last_error()
void set_error(const std::string& msg);
const char* last_error();

#define LDPC_HIP(call)                                                                           \
    do {                                                                                         \
        hipError_t _e = (call);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            ::ldpc::set_error(std::string(#call) + ": " + hipGetErrorString(_e));                \
            return LDPC_ERR_DEVICE;                                                              \
        }                                                                                        \
    } while (0)

struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinnedFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };

template <typename T>
using dev_ptr = std::unique_ptr<T[], DevFree>;
template <typename T>
using pinned_ptr = std::unique_ptr<T[], PinnedFree>;
// (hipEvent_t / hipStream_t are pointers to opaque structs)
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

// n elements of device memory on the current device (n = 0: still a valid
// allocation, so that no kernel argument is null)
template <typename T>
int dev_alloc(dev_ptr<T>& out, size_t n)
{
    T* p = nullptr;
    LDPC_HIP(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)));
    out.reset(p);
    return LDPC_OK;
}

// n elements of pinned host memory
template <typename T>
int pinned_alloc(pinned_ptr<T>& out, size_t n, unsigned flags = hipHostMallocDefault)
{
    T* p = nullptr;
    LDPC_HIP(hipHostMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T), flags));
    out.reset(p);
    return LDPC_OK;
}

// a device copy of src[0, n) (blocking)
template <typename T>
int upload(dev_ptr<T>& out, const T* src, size_t n)
{
    int rc = dev_alloc(out, n);
    if (rc) return rc;
    if (n) LDPC_HIP(hipMemcpy(out.get(), src, n * sizeof(T), hipMemcpyHostToDevice));
    return LDPC_OK;
}
template <typename T>
int upload(dev_ptr<T>& out, const std::vector<T>& v)
{
    return upload(out, v.data(), v.size());
}

// src[0, n) of device memory into dst (blocking)
template <typename T>
int download(T* dst, const T* src, size_t n)
{
    if (n) LDPC_HIP(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
    return LDPC_OK;
}

#if defined(__HIPCC__)
// kernel<<<grid, block, lds_bytes, stream>>>(args...) and the launch's error
template <typename F, typename... A>
int launch(F kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const A&... args)
{
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
    LDPC_HIP(hipGetLastError());
    return LDPC_OK;
}
#endif

inline int make_event(Event& out, unsigned flags = hipEventDisableTiming)
{
    hipEvent_t e = nullptr;
    LDPC_HIP(hipEventCreateWithFlags(&e, flags));
    out.reset(e);
    return LDPC_OK;
}

inline int make_stream(Stream& out, unsigned flags = hipStreamNonBlocking)
{
    hipStream_t s = nullptr;
    LDPC_HIP(hipStreamCreateWithFlags(&s, flags));
    out.reset(s);
    return LDPC_OK;
}

// make `device` the calling thread's device; `who` names the caller in the message
inline int select_device(const char* who, int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
        set_error(std::string(who) + ": no HIP device");
        return LDPC_ERR_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_error(std::string(who) + ": device ordinal out of range");
        return LDPC_ERR_DEVICE;
    }
    LDPC_HIP(hipSetDevice(device));
    return LDPC_OK;
}

}  // namespace ldpc
