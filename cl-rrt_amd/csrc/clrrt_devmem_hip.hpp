// clrrt_devmem_hip.hpp -- the memory owner's policy bound to the HIP runtime (clrrt_devmem.hpp): the one place in csrc
// that names the runtime's allocation calls.  Internal linkage: each library instantiates its own owner.
#pragma once
#include <hip/hip_runtime.h>

#include "clrrt_devmem.hpp"

namespace {
struct HipMem {
  using err_t = hipError_t;
  static constexpr hipError_t ok = hipSuccess, refused = hipErrorInvalidValue;
  static hipError_t dev_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t dev_free(void* p) { return hipFree(p); }
  static hipError_t host_alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
  static hipError_t host_free(void* p) { return hipHostFree(p); }
  // the guard bands' verbs (clrrt::MemGuard; never called while the guard is off)
  static hipError_t dev_fill(void* p, int byte, size_t bytes) { return hipMemset(p, byte, bytes); }
  static hipError_t copy_out(void* host_dst, const void* src, size_t bytes) {
    const hipError_t e = hipDeviceSynchronize();
    return e != hipSuccess ? e : hipMemcpy(host_dst, src, bytes, hipMemcpyDefault);
  }
};
template <typename T>
using Scratch = clrrt::DevScratch<HipMem, T>;  // call-lifetime device scratch of the entry points and selftests
}  // namespace
