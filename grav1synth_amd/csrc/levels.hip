// levels.hip -- kd_down, kd_lowres, kd_add: the three streaming kernels around a coarse level of `denoise`
// (include/g1s_diff.h, rules 25 - 27; what a lane does: levels_row.hip.h).
//
// A coarse level filters the 2 x 2 box mean of a frame and its result takes the place of the low frequencies of the
// full-resolution result.  kd_down makes the coarse planes of a batch's input frames, kd_lowres the signed difference d
// between the coarse level's output and the box mean of the fine output, kd_add puts d back onto the fine output through
// the 9-3-3-1 kernel, in place.  All three walk the coarse plane the same way: one launch covers the frames of a batch,
// grid (tiles, planes, frames) over a job array; a workgroup takes 256 x 8 coarse samples of one plane of one frame, a
// lane 8 of them in a row -- two rows of 16 fine samples.  The tiles are counted on the luma plane; a workgroup beyond a
// chroma plane leaves at once.  No LDS, no barrier: the overlap of neighbouring lanes' reads of d is the cache's job.
// Bound by HBM.  Row times stride is formed in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "levels_row.hip.h"

namespace g1s_lv {

namespace {

struct LevelParams {
  const LevelJob *jobs;
  int W[3], H[3];  // the fine planes
  int tiles_x;     // of the coarse luma plane
  int maxv;        // kd_add: 2^B - 1
};

// the lane's place: plane c of frame blockIdx.z, coarse samples cx0 .. cx0 + 7 of coarse row cy; false: outside the plane
__device__ inline bool lane_place(const LevelParams &p, int *c, int *cx0, int *cy) {
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
  *c = (int)blockIdx.y;
  *cx0 = tx * kTileW + ((int)threadIdx.x % kTileLanes) * kLaneCoarse, *cy = ty * kTileRows + (int)threadIdx.x / kTileLanes;
  return *cx0 < ((p.W[*c] + 1) >> 1) && *cy < ((p.H[*c] + 1) >> 1);
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void kd_down(LevelParams p) {
  int c, cx0, cy;
  if (!lane_place(p, &c, &cx0, &cy)) return;
  const LevelJob &j = p.jobs[blockIdx.z];
  box_lane<false, BPS>(j.fine[c], j.fine_stride[c], p.W[c], p.H[c], nullptr, 0, j.coarse[c], j.coarse_stride[c], cx0, cy);
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void kd_lowres(LevelParams p) {
  int c, cx0, cy;
  if (!lane_place(p, &c, &cx0, &cy)) return;
  const LevelJob &j = p.jobs[blockIdx.z];
  box_lane<true, BPS>(j.fine[c], j.fine_stride[c], p.W[c], p.H[c], j.coarse[c], j.coarse_stride[c], j.d[c], j.d_stride[c], cx0, cy);
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void kd_add(LevelParams p) {
  int c, cx0, cy;
  if (!lane_place(p, &c, &cx0, &cy)) return;
  const LevelJob &j = p.jobs[blockIdx.z];
  add_lane<BPS>(j.fine[c], j.fine_stride[c], p.W[c], p.H[c], j.d[c], j.d_stride[c], cx0, cy, p.maxv);
}

enum class Which { kDown, kLowres, kAdd };

hipError_t launch(Which which, int bps, int maxv, const LevelJob *jobs, uint32_t nframes, int nplanes, const int W[3], const int H[3], hipStream_t st) {
  if (!nframes) return hipSuccess;
  if ((bps != 1 && bps != 2) || nplanes < 1 || nplanes > 3 || nframes > 65535u) return hipErrorInvalidValue;
  LevelParams p{};
  p.jobs = jobs, p.maxv = maxv;
  for (int c = 0; c < nplanes; ++c) p.W[c] = W[c], p.H[c] = H[c];
  const int cw = (W[0] + 1) >> 1, ch = (H[0] + 1) >> 1;
  p.tiles_x = (cw + kTileW - 1) / kTileW;
  const dim3 grid((unsigned)(p.tiles_x * ((ch + kTileRows - 1) / kTileRows)), (unsigned)nplanes, nframes);
  if (which == Which::kDown) {
    if (bps == 1) hipLaunchKernelGGL(kd_down<1>, grid, dim3(kThreads), 0, st, p);
    else hipLaunchKernelGGL(kd_down<2>, grid, dim3(kThreads), 0, st, p);
  } else if (which == Which::kLowres) {
    if (bps == 1) hipLaunchKernelGGL(kd_lowres<1>, grid, dim3(kThreads), 0, st, p);
    else hipLaunchKernelGGL(kd_lowres<2>, grid, dim3(kThreads), 0, st, p);
  } else {
    if (bps == 1) hipLaunchKernelGGL(kd_add<1>, grid, dim3(kThreads), 0, st, p);
    else hipLaunchKernelGGL(kd_add<2>, grid, dim3(kThreads), 0, st, p);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_down(int bps, const LevelJob *jobs, uint32_t nframes, int nplanes, const int W[3], const int H[3], hipStream_t st) {
  return launch(Which::kDown, bps, 0, jobs, nframes, nplanes, W, H, st);
}
hipError_t launch_lowres(int bps, const LevelJob *jobs, uint32_t nframes, int nplanes, const int W[3], const int H[3], hipStream_t st) {
  return launch(Which::kLowres, bps, 0, jobs, nframes, nplanes, W, H, st);
}
hipError_t launch_add(int bps, int bit_depth, const LevelJob *jobs, uint32_t nframes, int nplanes, const int W[3], const int H[3], hipStream_t st) {
  return launch(Which::kAdd, bps, (1 << bit_depth) - 1, jobs, nframes, nplanes, W, H, st);
}

}  // namespace g1s_lv
