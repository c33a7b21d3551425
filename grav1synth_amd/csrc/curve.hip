// curve.hip -- kd_curve: a plane through a lookup table, sample by sample (include/g1s_diff.h, rule 14).
//
// `denoise` with a grain prior filters luma in a domain where the prior's grain has one size at every intensity: the
// forward curve takes the clip's samples (u8 or u16) to 12-bit u16 samples in front of the luma launch, the inverse brings
// the filtered plane back behind it.  Both are out(p) = LUT[min(in(p), last)], bound by HBM.  One launch covers the frames
// of a batch: a workgroup takes kStripRows consecutive rows of one frame, stages the table (at most 8 KB) into LDS once,
// and then a wave takes a row at a time, its lanes along the row as curve_row.hip.h's curve_row has them -- 16 samples a lane and
// step as 16-byte loads and stores where both rows are 16-byte aligned (uniform over the wave: base and pitch decide),
// sample by sample otherwise.  The lookups are data dependent; two lanes that want the same dword are served by one read,
// and grain spreads a wave's samples over a few tens of entries, so bank conflicts are bounded by the spread, not by 64.
// No byte outside the rows' samples is written.  Row times stride is formed in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve_row.hip.h"

namespace g1s_cv {

namespace {

constexpr int kWaves = 4, kThreads = (int)kLanes * kWaves;
constexpr uint32_t kStripRows = 32;  // rows a workgroup: 8 a wave

struct CurveParams {
  const CurveJob *jobs;
  const uint16_t *lut;
  uint32_t entries;  // 256, 1024 or 4096: the table; a sample above entries - 1 reads the last one
  uint32_t W, H;
};

template <int BYTES_IN, int BYTES_OUT>
__global__ __launch_bounds__(kThreads) void kd_curve(CurveParams p) {
  __shared__ __attribute__((aligned(16))) uint16_t s_lut[kMaxEntries];
  for (uint32_t i = threadIdx.x; i < p.entries / 2; i += kThreads) reinterpret_cast<uint32_t *>(s_lut)[i] = reinterpret_cast<const uint32_t *>(p.lut)[i];
  __syncthreads();
  const CurveJob &job = p.jobs[blockIdx.y];
  const uint32_t lane = threadIdx.x & (kLanes - 1), wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kLanes));
  for (uint32_t k = 0; k < kStripRows / kWaves; ++k) {
    const uint32_t y = blockIdx.x * kStripRows + k * kWaves + wave;  // (uniform over the wave)
    if (y >= p.H) break;
    curve_row<BYTES_IN, BYTES_OUT>(s_lut, p.entries - 1, job.src + (size_t)y * job.src_stride, job.dst + (size_t)y * job.dst_stride, p.W, lane);
  }
}

}  // namespace

hipError_t launch_curve(int bytes_in, int bytes_out, const CurveJob *jobs, uint32_t nframes, const uint16_t *lut, uint32_t entries, uint32_t W, uint32_t H,
                        hipStream_t st) {
  if (!nframes || !W || !H) return hipSuccess;
  if ((entries != 256 && entries != 1024 && entries != kMaxEntries) || nframes > 65535u) return hipErrorInvalidValue;
  const CurveParams p{jobs, lut, entries, W, H};
  const dim3 grid((H + kStripRows - 1) / kStripRows, nframes);
  if (bytes_in == 1 && bytes_out == 2) hipLaunchKernelGGL((kd_curve<1, 2>), grid, dim3(kThreads), 0, st, p);
  else if (bytes_in == 2 && bytes_out == 2) hipLaunchKernelGGL((kd_curve<2, 2>), grid, dim3(kThreads), 0, st, p);
  else if (bytes_in == 2 && bytes_out == 1) hipLaunchKernelGGL((kd_curve<2, 1>), grid, dim3(kThreads), 0, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace g1s_cv
