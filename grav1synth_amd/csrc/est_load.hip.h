// est_load.hip.h -- the word of a plane's row that a lane of a 3 x 3 stencil kernel holds (k_estimate in estimate.hip, the
// noise-level kernels in nlf.hip): 8 samples from column x0, read with the widest loads the address allows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the 8 samples of a word, widened; outside the plane: zeros (never used by an output pixel that counts)
template <int BPS>
__device__ __forceinline__ void est_load(const uint8_t *row, int x0, int W, bool row_ok, int (&p)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = 0;
  if (!row_ok || x0 >= W || x0 + 8 <= 0) return;
  if (x0 >= 0 && x0 + 8 <= W) {
    if (BPS == 2) {
      // (rows of a frame are at least 2-byte aligned; a word is read with the widest loads its address allows)
      const uint8_t *a = row + (size_t)x0 * 2;
      uint32_t w[4];
      if (((uintptr_t)a & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else if (((uintptr_t)a & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = reinterpret_cast<const uint32_t *>(a)[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = (uint32_t)reinterpret_cast<const uint16_t *>(a)[2 * k] | ((uint32_t)reinterpret_cast<const uint16_t *>(a)[2 * k + 1] << 16);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p[2 * k] = (int)(w[k] & 0xffffu);
        p[2 * k + 1] = (int)(w[k] >> 16);
      }
    } else {
      const uint8_t *a = row + x0;
      uint32_t w[2];
      if (((uintptr_t)a & 7) == 0) {
        const uint2 v = *reinterpret_cast<const uint2 *>(a);
        w[0] = v.x, w[1] = v.y;
      } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) w[k] = (uint32_t)a[4 * k] | ((uint32_t)a[4 * k + 1] << 8) | ((uint32_t)a[4 * k + 2] << 16) | ((uint32_t)a[4 * k + 3] << 24);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) p[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // a word over the right (or left) edge of the plane
    const int x = x0 + k;
    if (x >= 0 && x < W) p[k] = BPS == 2 ? (int)reinterpret_cast<const uint16_t *>(row)[x] : (int)row[x];
  }
}
