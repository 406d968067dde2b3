// fp32 <-> bf16 bit conversions shared by the kernels that store bf16 (gradclip.hip,
// wire.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tgpipe {

// Round to nearest even; NaN stays a (quiet) NaN.  A finite value past the largest bf16
// carries into the exponent and becomes inf.
__device__ __forceinline__ uint32_t to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

// Two floats into one 32-bit word of two bf16 (lo at the lower address).
__device__ __forceinline__ uint32_t to_bf16x2(float lo, float hi) {
  return to_bf16(lo) | (to_bf16(hi) << 16);
}

}  // namespace tgpipe
