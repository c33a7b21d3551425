// strip_walk.hip.h -- what the 3 x 3 stencil kernels share (k_estimate in estimate.hip; k_nlf and k_nlf_t in nlf.hip): a wave
// owns 62 x 8 output columns of a strip of 32 rows and walks it top to bottom with the three rows of the stencil in
// registers, a word of 8 samples a lane, the neighbours of a word's ends from the adjacent lanes.  Here: the strip's
// constants, a wave's coordinates in it, the word of a row (est_load: the widest loads the address allows), the three-row
// window of a plane, the stencil on nine samples, and averageLuma under a word of chroma.  k_estimate_pk (estimate.hip)
// takes the constants and the coordinates and has a packed pipeline of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

constexpr int kEdgeThreshold = 50;  // the estimator's EDGE_THRESHOLD
constexpr int kStripRows = 32;      // output rows per wave strip (+ 2 halo rows)
constexpr int kWavesPerWg = 4, kStripThreads = 64 * kWavesPerWg;
constexpr int kColsPerWave = 62 * 8;

// Strip `strip` of a plane `ph` rows high, as lane `lane` of its wave sees it.  Column strips are the fast index: the waves
// of a workgroup read adjacent kilobytes of the same rows.  The wave's output columns are [cs * 496, cs * 496 + 496) (less
// the plane's first and last column); lane l holds the word at x0 = cs * 496 - 8 + 8 l -- a multiple of 8 samples: aligned
// 16-byte loads -- and lanes 0 and 63 hold the halo words.  Output rows: [y_first, y_last).
struct StripCoords {
  int cs, rs, x0, y_first, y_last;
  bool out_lane;
};
__device__ __forceinline__ StripCoords strip_coords(int strip, int col_strips, int lane, int ph, int strip_rows = kStripRows) {
  StripCoords s;
  s.cs = strip % col_strips, s.rs = strip / col_strips;
  s.x0 = s.cs * kColsPerWave - 8 + 8 * lane;
  s.y_first = 1 + s.rs * strip_rows, s.y_last = min(s.y_first + strip_rows, ph - 1);
  s.out_lane = lane >= 1 && lane <= 62;
  return s;
}

// (global address space: a pointer read from memory is `flat` to the compiler otherwise, and flat loads wait on the LDS counter too)
#define EST_GLOBAL __attribute__((address_space(1)))
typedef const EST_GLOBAL uint8_t *est_gptr;
typedef uint32_t est_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t est_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ est_gptr est_global(const uint8_t *p) { return (est_gptr)(uintptr_t)p; }

// the 8 samples of a word, widened; outside the plane: zeros (never used by an output pixel that counts)
template <int BPS>
__device__ __forceinline__ void est_load(const uint8_t *row_, int x0, int W, bool row_ok, int (&p)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = 0;
  if (!row_ok || x0 >= W || x0 + 8 <= 0) return;
  const est_gptr row = est_global(row_);
  if (x0 >= 0 && x0 + 8 <= W) {
    if (BPS == 2) {
      // (rows of a frame are at least 2-byte aligned; a word is read with the widest loads its address allows)
      const est_gptr a = row + (size_t)x0 * 2;
      uint32_t w[4];
      if (((uintptr_t)a & 15) == 0) {
        const est_u32x4 v = *(const EST_GLOBAL est_u32x4 *)a;
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else if (((uintptr_t)a & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = ((const EST_GLOBAL uint32_t *)a)[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = (uint32_t)((const EST_GLOBAL uint16_t *)a)[2 * k] | ((uint32_t)((const EST_GLOBAL uint16_t *)a)[2 * k + 1] << 16);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p[2 * k] = (int)(w[k] & 0xffffu);
        p[2 * k + 1] = (int)(w[k] >> 16);
      }
    } else {
      const est_gptr a = row + x0;
      uint32_t w[2];
      if (((uintptr_t)a & 7) == 0) {
        const est_u32x2 v = *(const EST_GLOBAL est_u32x2 *)a;
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
    if (x >= 0 && x < W) p[k] = BPS == 2 ? (int)((const EST_GLOBAL uint16_t *)row)[x] : (int)row[x];
  }
}

// a 3 x 3 neighbourhood, m[row][column]
struct Nine {
  int m00, m01, m02, m10, m11, m12, m20, m21, m22;
};

// The lane's words of rows y - 1, y, y + 1 of a plane pw x ph, and beside them the column left of the word (the neighbour
// lane's last sample) and right of it (its first).  A strip: prime(y_first); then for every output row y: load(y), fetch(),
// at<0..7>(), rotate().
template <int BPS>
struct RowWindow {
  const uint8_t *plane;
  uint32_t stride;
  int x0, pw, ph;
  int a[8], b[8], c[8];
  int al, bl, cl, ar, br, cr;
  __device__ __forceinline__ void prime(const uint8_t *plane_, uint32_t stride_, int x0_, int pw_, int ph_, int y_first) {
    plane = plane_, stride = stride_, x0 = x0_, pw = pw_, ph = ph_;
    est_load<BPS>(plane + (size_t)(y_first - 1) * stride, x0, pw, true, a);
    est_load<BPS>(plane + (size_t)y_first * stride, x0, pw, y_first < ph, b);
  }
  // row y + 1, the last of output row y's three
  __device__ __forceinline__ void load(int y) { est_load<BPS>(plane + (size_t)(y + 1) * stride, x0, pw, y + 1 < ph, c); }
  __device__ __forceinline__ void fetch() {
    al = __shfl_up(a[7], 1), bl = __shfl_up(b[7], 1), cl = __shfl_up(c[7], 1);
    ar = __shfl_down(a[0], 1), br = __shfl_down(b[0], 1), cr = __shfl_down(c[0], 1);
  }
  // the neighbourhood of the word's sample K (a constant: which of them come from the neighbour lanes is decided here)
  template <int K>
  __device__ __forceinline__ Nine at() const {
    constexpr int L = K ? K - 1 : 0, R = K < 7 ? K + 1 : 7;
    return {K ? a[L] : al, a[K], K < 7 ? a[R] : ar, K ? b[L] : bl, b[K], K < 7 ? b[R] : br, K ? c[L] : cl, c[K], K < 7 ? c[R] : cr};
  }
  __device__ __forceinline__ void rotate() {
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = b[k], b[k] = c[k];
  }
};

// f(K) for K = 0 .. 7 as constants: the samples of a word in turn
template <class F>
__device__ __forceinline__ void each_of_word(F &&f) {
  f(std::integral_constant<int, 0>()), f(std::integral_constant<int, 1>()), f(std::integral_constant<int, 2>()), f(std::integral_constant<int, 3>());
  f(std::integral_constant<int, 4>()), f(std::integral_constant<int, 5>()), f(std::integral_constant<int, 6>()), f(std::integral_constant<int, 7>());
}

// The stencil on nine samples.  The gate: the Sobel gradient |Gx| + |Gy| rounded to 8-bit scale (smooth below
// kEdgeThreshold); the box sum; the Laplacian.
__device__ __forceinline__ int stencil_gate(const Nine &m, int half, int shift) {
  const int gx = (m.m00 - m.m02) + (m.m20 - m.m22) + 2 * (m.m10 - m.m12);
  const int gy = (m.m00 - m.m20) + (m.m02 - m.m22) + 2 * (m.m01 - m.m21);
  return (abs(gx) + abs(gy) + half) >> shift;
}
__device__ __forceinline__ int stencil_box(const Nine &m) { return (m.m00 + m.m01 + m.m02) + (m.m10 + m.m11 + m.m12) + (m.m20 + m.m21 + m.m22); }
__device__ __forceinline__ int stencil_laplacian(const Nine &m) {
  return 4 * m.m11 - 2 * (m.m01 + m.m21 + m.m10 + m.m12) + (m.m00 + m.m02 + m.m20 + m.m22);
}

// a[k] += `measure`'s averageLuma (rule 2) of the lane's 8 chroma samples from column x0, the luma row being lrow
template <int BPS>
__device__ __forceinline__ void add_average_luma(const uint8_t *lrow, int x0, int W, int xdec, bool out_lane, int (&a)[8]) {
  int l0[8], l1[8];
  const int lx0 = xdec ? 2 * x0 : x0;
  est_load<BPS>(lrow, lx0, W, out_lane, l0);
  est_load<BPS>(lrow, lx0 + 8, W, out_lane && xdec, l1);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (xdec) {
      const int e = 2 * k, i0 = e < 8 ? l0[e & 7] : l1[e & 7], i1 = e < 8 ? l0[(e + 1) & 7] : l1[(e + 1) & 7];
      a[k] += (i0 + (((x0 + k) << 1) + 1 < W ? i1 : i0) + 1) >> 1;
    } else {
      a[k] += l0[k];
    }
  }
}
