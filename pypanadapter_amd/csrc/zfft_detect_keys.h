// zfft_detect_keys.h -- the order-preserving key map the row detector's kernels share
// (detect_kernels.hip, detect_local_kernels.hip).  Device code only; not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace zfft {

// float bits -> uint32 in the floats' order: negative values complemented, the others with the
// top bit set.  -inf and the NaNs with the sign bit fall below kKeyFiniteLo, +inf and the other
// NaNs at or above kKeyFiniteHi; the finite values lie between, -0.0 just below 0.0.
constexpr uint32_t kKeyFiniteLo = 0x00800000u, kKeyFiniteHi = 0xFF800000u;
constexpr uint32_t kKeyPad = 0xFFFFFFFFu;  // a NaN: the columns beyond row_len, never on, never counted

__device__ __forceinline__ uint32_t det_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float det_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

}  // namespace zfft
