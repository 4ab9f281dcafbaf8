// One element of a tensor that crosses the C ABI in the caller's dtype (MDPT_DT_* of mdpt_kernels.h): images, raw weights, depth maps.
#pragma once
#include "mdpt_kernels.h"

__device__ __forceinline__ float ld_dt(const void* p, size_t i, int dt) {
    if (dt == MDPT_DT_BF16) return (float)((const __bf16*)p)[i];
    if (dt == MDPT_DT_F16) return (float)((const _Float16*)p)[i];
    return ((const float*)p)[i];
}

__device__ __forceinline__ void st_dt(void* p, size_t i, float v, int dt) {
    if (dt == MDPT_DT_BF16) ((__bf16*)p)[i] = (__bf16)v;
    else if (dt == MDPT_DT_F16) ((_Float16*)p)[i] = (_Float16)v;
    else ((float*)p)[i] = v;
}

// the value once stored in dtype dt
__device__ __forceinline__ float round_dt(float v, int dt) {
    if (dt == MDPT_DT_BF16) return (float)(__bf16)v;
    if (dt == MDPT_DT_F16) return (float)(_Float16)v;
    return v;
}
