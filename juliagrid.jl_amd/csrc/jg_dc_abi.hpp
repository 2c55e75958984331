// jg_dc_abi.hpp -- internal: the prologue every extern "C" entry point of the DC files shares (handle cast, null check, hipSetDevice, return through
// jg::api_fail, HIP-call check -- both from jg_engine.hpp) and the HIP-event timing loop of their *_time_kernel exports.  Codes: 1 bad argument / null handle, 2 HIP error, 4 a call
// out of order, 5 memory budget.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "jg_engine.hpp"

namespace jg {

// `reps` timings of what `enqueue` puts on `stream` (it returns a status; not 0: its text is in `error` already), one pair of HIP events around each.  The
// first error wins and goes to `error`; the events are destroyed on every path.
template <typename F>
int time_events(hipStream_t stream, int reps, double* ms, std::string& error, F&& enqueue) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) { rc = 2; error = std::string(what) + ": " + hipGetErrorString(e); } return e == hipSuccess; };
    if (hip(hipEventCreate(&e0), "hipEventCreate") && hip(hipEventCreate(&e1), "hipEventCreate"))
        for (int r = 0; r < reps && !rc; ++r) {
            if (!hip(hipEventRecord(e0, stream), "hipEventRecord")) break;
            rc = enqueue();
            float t = 0.f;
            if (rc || !hip(hipGetLastError(), "launch") || !hip(hipEventRecord(e1, stream), "hipEventRecord") || !hip(hipEventSynchronize(e1), "hipEventSynchronize") ||
                !hip(hipEventElapsedTime(&t, e0, e1), "hipEventElapsedTime")) break;
            ms[r] = (double)t;
        }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

}  // namespace jg

#define DC_API_ENTER(Handle, null_text, h)                                              \
    Handle* d = reinterpret_cast<Handle*>(static_cast<intptr_t>(h));                    \
    if (!d) return jg::api_fail(1, null_text);                                          \
    if (hipSetDevice(d->device) != hipSuccess) return jg::api_fail(2, "hipSetDevice failed")
#define DC_ENTER(h) DC_API_ENTER(jg::DcHandle, "null DC handle", h)
#define SE_ENTER(h) DC_API_ENTER(jg::DcseHandle, "null DC state estimation handle", h)
#define DC_RET(expr) do { const int rc__ = (expr); if (rc__) return jg::api_fail(rc__, d->error); } while (0)
#define DC_API_HIP JG_API_HIP
