// Device helpers shared by the two fp8 quantisers (quant_f8.hip, quant_mx8.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldnn {

// Four fp32 -> four codes in one dword with the hardware's packed converts (round to nearest even).
// FMT: 0 = e4m3fn, 1 = e5m2.
template <int FMT>
__device__ __forceinline__ uint32_t cvt4(float a, float b, float c, float d) {
  int w = 0;
  if constexpr (FMT == 0) {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
  }
  return (uint32_t)w;
}

// (compares, not fminf / fmaxf: a NaN stays a NaN)
__device__ __forceinline__ float clampf(float v, float mx) { return v > mx ? mx : (v < -mx ? -mx : v); }

}  // namespace ldnn
