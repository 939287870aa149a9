// pe_host.hpp -- the host helpers every translation unit with HIP calls shares: the error
// return (pe_last_error()'s text is recorded by plantos_batch.hip's pe_internal_set_error) and the
// device binder of one API call.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "pe_handle.hpp"

namespace {

int fail(int code, const std::string& msg) { return pe_internal_set_error(code, msg.c_str()); }

int hip_fail(hipError_t e, const char* what) {
  return fail(PE_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// Binds a handle's device for one API call and restores the caller's device afterwards (the
// library never leaves the calling thread on another device).  rc: PE_OK, or the error of the
// failed hipGetDevice / hipSetDevice with pe_last_error() set.
struct DeviceGuard {
  int prev = -1;
  int rc = PE_OK;
  explicit DeviceGuard(const pe_handle* h) : DeviceGuard(h->device) {}
  explicit DeviceGuard(int device) {
    // hipGetLastError() reports the last failed runtime call of this thread, whoever made it
    // (torch probes, the caller's own calls): drop such a stale error so that the launch checks
    // of this call see only its own launches.
    (void)hipGetLastError();
    int cur = -1;
    hipError_t e = hipGetDevice(&cur);
    if (e != hipSuccess) {
      rc = hip_fail(e, "hipGetDevice");
    } else if (cur != device) {
      e = hipSetDevice(device);
      if (e != hipSuccess)
        rc = hip_fail(e, "hipSetDevice");
      else
        prev = cur;
    }
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace
