// Host-side plumbing shared by the device paths beside the hot path: vc_align.hip, vc_large.hip, vc_overlap.hip, vc_scrub.hip and vc_cluster.hip.
// Host code only: the device buffers of a scope, checked copies, the check that a batch of launches ran, the device check and the
// knobs in MiB.  The hipcub sorts and sums are in vc_devscan.h, so a file that includes this one alone compiles without hipcub.
// Every file keeps its own thread_local error text and its own fail(): the *_last_error entries are separate by contract.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "vechat_hip.h"

namespace vc_dev {

// the device allocations of one scope, freed when it ends (or one by one with drop)
struct DevMem {
    std::vector<void*> held;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { for (void* q : held) (void)hipFree(q); }
    // n elements (at least one), filled from src where there is one; false: the allocation or the copy failed
    template <class T> bool alloc(T** p, uint64_t n, const std::remove_const_t<T>* src = nullptr) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<uint64_t>(n, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return false; }
        held.push_back(q);
        *p = (T*)q;
        return !src || n == 0 || hipMemcpy(q, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    }
    void drop(const void* p) {
        for (size_t i = 0; i < held.size(); ++i) if (held[i] == p) { (void)hipFree(held[i]); held.erase(held.begin() + (long)i); return; }
    }
};

// checked copies of n elements; nothing is copied for n == 0
template <class T> bool to_device(T* d, const T* h, uint64_t n) { return n == 0 || hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess; }
template <class T> bool to_host(T* h, const T* d, uint64_t n) { return n == 0 || hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess; }
template <class T> bool to_host(std::vector<T>& h, const T* d, uint64_t n) { h.resize(n); return to_host(h.data(), d, n); }

// every launch so far has run, and none of them failed
inline bool ran() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess; }

inline uint32_t grid(uint64_t n, uint32_t block = 256) { return (uint32_t)((n + block - 1) / block); }

// a knob in MiB as bytes (fractions allowed); 0: not set
inline uint64_t env_mib(const char* name) {
    const char* v = getenv(name);
    const double x = v ? std::atof(v) : 0.0;
    return x > 0 ? std::max<uint64_t>((uint64_t)(x * 1048576.0), 1) : 0;
}

// VC_OK, or the code of a device the kernels cannot run on with its text in msg; `who` ("the scrubber") names the caller.
// The device is not made current: that stays with the caller.
inline int check_device(int32_t device, const char* who, std::string& msg) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        msg = std::string("no HIP device visible; ") + who + " has no CPU fallback";
        return VC_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { msg = "no HIP device with this ordinal"; return VC_ERR_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { msg = "hipGetDeviceProperties failed"; return VC_ERR_HIP; }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { msg = "the kernels are built for gfx950 only"; return VC_ERR_NO_DEVICE; }
    return VC_OK;
}

}  // namespace vc_dev
