// gswm_host.h -- the host prelude of the codec family (gswm_kernels.hip with its .inc files, gswm_trace.hip, gswm_keyed.hip, gswm_tamper.hip), the matmul
// engine (gswm_mm.hip) and the convolution front end (gswm_conv.hip): the HIP error path, the CU count and the dynamic-LDS opt-in.  Host code only; include after
// <hip/hip_runtime.h> and include/gswm.h.
#pragma once

extern __attribute__((visibility("hidden"))) thread_local int g_last_hip_error;   // gswm_kernels.hip; read by gsw_last_hip_error()

static inline int hip_fail(hipError_t e) {
    g_last_hip_error = (int)e;
    return GSW_ERR_HIP;
}
#define GSW_HIP(call) do { hipError_t _e = (call); if (_e != hipSuccess) return hip_fail(_e); } while (0)

// compute units of the current device; 256 (MI355X) when the query fails.  Asked once per translation unit.
static inline int device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
        else cus = 256;
    }
    return cus;
}

// A launch that needs more than `threshold` bytes of dynamic LDS asks for them first: 48 KiB, less for a kernel with much static LDS.
static inline hipError_t allow_dynamic_lds(const void* kernel, uint32_t lds, uint32_t threshold = 48u * 1024u) {
    return lds > threshold ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}
