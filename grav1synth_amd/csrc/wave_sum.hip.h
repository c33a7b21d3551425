// wave_sum.hip.h -- integer sums across the 64 lanes of a wave in the VALU (DPP), every lane taking part: what the binned
// kernels (km_measure, lag_pass and km_measure_s in measure.hip, k_nlf in nlf.hip) hand a bin's sums on with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// full-wave integer sum in the VALU (DPP), every lane taking part; the total is read from lane 63
__device__ __forceinline__ int wave_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);  // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);  // row_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast31 -> rows 2, 3
  return __builtin_amdgcn_readlane(v, 63);
}
// the same for lane values up to 2^31 in size: v = (v >> 16) 2^16 + (v & 0xffff), the halves summed apart
__device__ __forceinline__ long long wave_sum_wide(int v) {
  const int lo = wave_sum(v & 0xffff), hi = wave_sum(v >> 16);
  return (long long)hi * 65536 + lo;
}
// the same for unsigned lane values below 2^57: two 16-bit pieces and the rest, summed apart
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
  const int lo = wave_sum((int)(v & 0xffffu)), mid = wave_sum((int)((v >> 16) & 0xffffu)), hi = wave_sum((int)(v >> 32));
  return ((unsigned long long)(unsigned)hi << 32) + ((unsigned long long)(unsigned)mid << 16) + (unsigned)lo;
}
