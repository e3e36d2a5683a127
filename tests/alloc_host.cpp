// alloc_host.cpp -- stand-alone host program around rt-depth-map_amd/csrc/rtdm_host.h for tests/test_alloc_cpu.py: the chain of
// requests a create function makes of its AllocList, with a failure in it.  Without a HIP device every request fails, so the
// first one is the failure; with a device two small requests succeed and an absurd third one fails.  Either way: the first
// error stays, nothing is attempted after it, release() frees exactly what was allocated, and create_failed maps the error.
// Prints one line per failed check and returns their number.
#include "rtdm_host.h"

#include <cstdio>

thread_local std::string rtdm::g_hip_err;   // (the library's own definition is in api_core.hip)
using namespace rtdm;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

struct Handle { uint8_t *a, *z, *again; int16_t* b; void* c; int32_t* late; AllocList mem; };

int main()
{
    int ndev = 0;
    const bool gpu = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    (void)hipGetLastError();
    Handle h{};
    AllocList& m = h.mem;
    const bool a = m.dev(&h.a, 4096), b = m.host(&h.b, 4096);
    CHECK(a == gpu && b == gpu && (h.a != nullptr) == gpu && (h.b != nullptr) == gpu);
    CHECK(m.dev(&h.z, 0) == gpu && h.z == nullptr);                   // zero-sized: skipped, no error of its own
    CHECK(m.items.size() == (gpu ? 2u : 0u) && (m.err == hipSuccess) == gpu);
    CHECK(!m.dev(&h.c, (size_t)1 << 60) && h.c == nullptr && m.err != hipSuccess);
    const hipError_t first = m.err;
    const size_t held = m.items.size();
    h.late = (int32_t*)&h;                                            // after a failure a request does not even touch its pointer
    CHECK(!m.host(&h.late, 64, hipHostMallocMapped) && h.late == (int32_t*)&h && m.err == first && m.items.size() == held);
    CHECK(create_failed("x_create", first) == (first == hipErrorOutOfMemory ? RTDM_ERR_NOMEM : RTDM_ERR_HIP));
    CHECK(g_hip_err == std::string("x_create: ") + hipGetErrorString(first));
    if (gpu) CHECK(hipGetLastError() == hipSuccess);                  // create_failed has cleared the sticky error
    CHECK(create_failed("x_create", hipErrorOutOfMemory) == RTDM_ERR_NOMEM && create_failed("x_create", hipErrorInvalidValue) == RTDM_ERR_HIP);
    m.err = hipSuccess;                                               // what a caller that allocates lazily does before it asks again
    CHECK(m.dev(&h.again, 256) == gpu && m.items.size() == held + (gpu ? 1u : 0u));
    m.release();
    CHECK(m.items.empty());
    m.release();                                                      // (a second release frees nothing twice)
    g_hip_err = "the first message";
    { DrainOnError drain(nullptr); }                                  // armed, no stream to wait for: the message survives
    CHECK(g_hip_err == "the first message");
    printf("%s: %d failed checks (HIP devices: %d)\n", failures ? "FAILED" : "ok", failures, gpu ? ndev : 0);
    return failures;
}
