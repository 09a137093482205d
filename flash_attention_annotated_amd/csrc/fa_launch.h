// fa_launch.h — one kernel launch of the forward and backward entry points (fa_fwd_api.hip, fa_bwd_api.hip).
#pragma once
#include "fa_fwd.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

namespace fa {

// Launch `Kernel` with `smem` bytes of dynamic LDS on `stream`.  More than 64 KiB needs an opt-in, which is a per-device
// attribute of the kernel: it is set once per (kernel, device ordinal), one bit per device.  Returns FA_OK or FA_ERR_LAUNCH.
template <auto Kernel, typename Params>
int launch_kernel(int smem, int64_t grid, int threads, hipStream_t stream, const Params &params) {
    static std::atomic<uint64_t> attr_set{0};
    if (smem > 65536) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const uint64_t bit = uint64_t(1) << (dev & 63);
        if (!(attr_set.load(std::memory_order_acquire) & bit)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) {
                (void)hipGetLastError();
                return FA_ERR_LAUNCH;
            }
            attr_set.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(threads), smem, stream, params);
    return hipGetLastError() == hipSuccess ? FA_OK : FA_ERR_LAUNCH;
}

}  // namespace fa
