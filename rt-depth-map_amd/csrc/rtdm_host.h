// rtdm_host.h -- what the files of the C ABI layer (api_*.hip) share on the host side: the last-error string, the HIPC
// macro, device selection, the drain guard of the host entry points, the one host row copy (rtdm_rows.h: copy_rows), and the two
// helpers every create / destroy pair is written with (AllocList, create_failed).  Host only and private to csrc/.
#pragma once
#include "../../include/rtdm.h"
#include "rtdm_rows.h"
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

namespace rtdm {

extern thread_local std::string g_hip_err;   // rtdm_last_hip_error (one definition: api_core.hip)

#define HIPC(expr)                                                                               \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            rtdm::g_hip_err = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
            return RTDM_ERR_HIP;                                                                 \
        }                                                                                        \
    } while (0)

inline int use_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RTDM_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return RTDM_ERR_NO_DEVICE;
    HIPC(hipSetDevice(device));
    return RTDM_OK;
}

// host memory the GPU can DMA from / to directly (hipHostMalloc, hipHostRegister)?
inline bool page_locked(const void* q)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }   // plain malloc memory: an error, not a fault
    return a.type == hipMemoryTypeHost;
}

// Host entry points hand the caller's (possibly page-locked) planes to async copies: whatever way they leave, nothing may
// still be in flight from / to those planes.  Success paths synchronise themselves and disarm the guard.
struct DrainOnError {
    hipStream_t s[3];              // a handle's own streams (never the null stream); unused ones are null
    bool armed = true;
    explicit DrainOnError(hipStream_t a, hipStream_t b = nullptr, hipStream_t c = nullptr) : s{a, b, c} {}
    ~DrainOnError()
    {
        if (!armed) return;
        const std::string first = g_hip_err;
        for (hipStream_t q : s) if (q) (void)hipStreamSynchronize(q);
        (void)hipGetLastError();
        g_hip_err = first;
    }
};

// The device and page-locked memory a handle owns.  Requests are made in order; after the first failure (or with `err` set by
// the caller to an earlier failure of its own) nothing more is allocated and `err` keeps that error.  Zero-sized requests are
// skipped.  dev() and host() say whether all is well so far; release() frees what was allocated: destroy functions keep no lists.
struct AllocList {
    struct Item { void* p; bool host; };
    std::vector<Item> items;
    hipError_t err = hipSuccess;

    template <class T> bool dev(T** p, size_t bytes) { return get((void**)p, bytes, false, 0); }
    template <class T> bool host(T** p, size_t bytes, unsigned flags = hipHostMallocDefault) { return get((void**)p, bytes, true, flags); }
    void release()
    {
        for (const Item& b : items) (void)(b.host ? hipHostFree(b.p) : hipFree(b.p));
        items.clear();
    }
private:
    bool get(void** p, size_t bytes, bool host, unsigned flags)
    {
        if (err != hipSuccess || !bytes) return err == hipSuccess;
        err = host ? hipHostMalloc(p, bytes, flags) : hipMalloc(p, bytes);
        if (err == hipSuccess) items.push_back(Item{*p, host});
        else *p = nullptr;
        return err == hipSuccess;
    }
};

// The end of a create function that failed with `e` (and destroys the handle itself): message, sticky error cleared, status.
inline int create_failed(const char* where, hipError_t e)
{
    g_hip_err = std::string(where) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP;
}

}  // namespace rtdm
