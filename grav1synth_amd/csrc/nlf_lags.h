// nlf_lags.h -- what nlf.hip (the meter) and nlf_lags.hip (the lag kernels) share: the jobs a noise-level kernel is launched
// with, and the lag launches of a batch of pairs (include/g1s_diff.h, "lagged noise levels", rules L1 - L5).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "meter_op.h"

// a frame's planes as a noise-level kernel reads them
struct NlfJob {
  const uint8_t *p[3];
  uint32_t stride[3];  // bytes
};
// frame t and frame t - 1 of a pair
struct NlfTJob {
  NlfJob now, before;
};

namespace g1s_nlf_lags {

// A workgroup's tile of a plane: kTileW columns; kTileRowsLuma rows in the luma launch, kTileRowsChroma in the chroma launch
// (which also stages the luma under its tile).  A tile leaves one partial record of kEntries 64-bit words.
constexpr int kTileW = 64, kTileRowsLuma = 32, kTileRowsChroma = 16;
constexpr int kLags = 46, kCross = 25;
constexpr int kEntries = 2 * kLags + 1 + 2 * kCross + 3;  // n[46], r[46], s, xn[25], xr[25], ln, ls, l2

// a frame's tiles, plane after plane
void cut(const g1s_op::PlaneGeom &g, g1s_op::Units &tiles);
// the launch of a plane class (luma; both chroma planes) for the `pairs` jobs at d_jobs: a partial record a tile
hipError_t launch(bool chroma, const NlfTJob *d_jobs, uint32_t pairs, unsigned long long *partials, const g1s_op::PlaneGeom &g, const g1s_op::Units &tiles,
                  uint32_t bit_depth, hipStream_t stream);
// the summing kernel (grid (plane, pair)) and its block size: every word of a g1s_nlf_lrecord_t is written
void (*tail())(g1s_op::TailParams);
constexpr unsigned kTailThreads = 1024;

}  // namespace g1s_nlf_lags
