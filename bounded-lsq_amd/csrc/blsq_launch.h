// The one launch path of the kernels that use dynamic LDS (every kernel translation unit includes this).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace blsq {

static constexpr size_t LDS_MAX_BYTES = 160 * 1024;   // LDS of one workgroup (CDNA4)

// launch<kernel>(grid, block, lds, stream, args...): more dynamic LDS than a workgroup can have is refused before the
// runtime sees it; dynamic LDS above 64 KB has to be granted per kernel and device, which happens here whenever `lds`
// exceeds what this kernel has been granted on the current device (a racing second grant is harmless).  `granted` is
// one table per kernel: the kernel is the template key.
template <auto Kernel, class... A>
static hipError_t launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
  if (lds > LDS_MAX_BYTES) return hipErrorInvalidValue;
  static std::atomic<size_t> granted_dev[64];
  int dev = 0;
  (void)hipGetDevice(&dev);                      // the attribute is per device
  std::atomic<size_t>& granted = granted_dev[dev & 63];
  if (lds > granted.load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    granted.store(lds, std::memory_order_release);
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
  return hipGetLastError();
}

}  // namespace blsq
