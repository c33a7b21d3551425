// estimate.hip -- N4: the single-source noise estimator of `grav1synth estimate` (feature "unstable").
//
// The command (/root/reference/src/main.rs:534-608) calls av1_grain::estimate_plane_noise(&frame.y_plane, bit_depth) on
// every frame and writes "filmgrn1" and one "{:.3}" line per frame (-1 for None).  The estimator is av1-grain's port of
// libaom's av1_estimate_noise_from_single_plane: over the interior pixels of the luma plane, a Sobel gradient decides
// whether the pixel is smooth (|Gx| + |Gy|, rounded down to 8-bit scale, below 50); the smooth pixels' |Laplacian|
// (rounded to 8-bit scale) is averaged: sigma = accum / (6 count) * sqrt(pi / 2), None when fewer than 16 pixels are
// smooth.  One pass over one plane, a 3x3 stencil and two integer sums: HBM bound (2 bytes per luma pixel at 10 bit).
//
// Kernel (k_estimate, the 32-bit form, from the pieces of strip_walk.hip.h that the noise-level kernels in nlf.hip are built
// from too): a wave owns 62 x 8 output columns of a strip of rows and walks the strip top to bottom with the three rows
// of the stencil in registers (each row is loaded once per strip, as one 8-sample word per lane: 16-byte loads at
// 10 bit); lanes 0 and 63 only carry halo columns, the horizontal neighbours of a lane's word come from the adjacent
// lanes.  Exact integers: the two sums of a frame are the same for any strip / wave / batch partition; the host turns
// them into the f64 with the reference's three operations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "strip_walk.hip.h"
#include "estimate_plan.h"
#include "frame_op.h"

namespace {

struct EstFrame {
  const uint8_t *y;
  uint32_t stride;  // bytes
};

struct EstParams {
  const EstFrame *frames;
  unsigned long long *sums;  // [frames][2]: accum, count
  int W, H, bps, shift;
  int col_strips, row_strips, strip_rows;
};

template <int BPS>
__global__ __launch_bounds__(kStripThreads) void k_estimate(EstParams ep) {
  const int frame = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strip = blockIdx.x * kWavesPerWg + wave;
  if (strip >= ep.col_strips * ep.row_strips) return;
  const StripCoords s = strip_coords(strip, ep.col_strips, lane, ep.H);
  const EstFrame fr = ep.frames[frame];
  const int W = ep.W, shift = ep.shift, half = shift ? 1 << (shift - 1) : 0;
  RowWindow<BPS> w;
  w.prime(fr.y, fr.stride, s.x0, W, ep.H, s.y_first);
  uint32_t accum = 0, count = 0;
  for (int y = s.y_first; y < s.y_last; ++y) {
    w.load(y);
    w.fetch();
    if (s.out_lane)
      each_of_word([&](auto K) __attribute__((always_inline)) {
        const Nine m = w.template at<decltype(K)::value>();
        const int x = s.x0 + K;
        const int ga = stencil_gate(m, half, shift), v = stencil_laplacian(m);
        const bool on = (x >= 1) & (x < W - 1) & (ga < kEdgeThreshold);  // (`&`: no branch a condition)
        accum += on ? (uint32_t)((abs(v) + half) >> shift) : 0u;
        count += on ? 1u : 0u;
      });
    w.rotate();
  }
  // wave sums -> one pair of atomics per wave
  for (int o = 32; o; o >>= 1) {
    accum += __shfl_down(accum, o);
    count += __shfl_down(count, o);
  }
  if (lane == 0 && (accum | count)) {
    atomicAdd(&ep.sums[2 * frame], (unsigned long long)accum);
    atomicAdd(&ep.sums[2 * frame + 1], (unsigned long long)count);
  }
}

// ---------------------------------------------------------------------------------
// k_estimate_pk: the same sums in packed 16-bit arithmetic, for depths 8 .. 12 (every intermediate fits 16 bits:
// |Gx|, |Gy| <= 4 * 4095, their sum + rounding <= 32768 as u16, |Laplacian| <= 8 * 4095).  Only the simplest
// 32-bit VALU operations issue at two cycles a wave on gfx950 (v_sub, v_and, shifts); everything else -- v_max,
// three-operand forms, every v_pk_* -- takes four (tools/valu_rate.hip), so a packed operation is two pixels
// for the price of one.  Both stencils are separable and the horizontal parts are carried down the strip:
//   per input row    H = l - r,  S = l + 2 c + r,  T = l - 2 c + r        (l, r: the row shifted by one sample)
//   per output row   Gx = H0 + 2 H1 + H2,  Gy = S0 - S2,  Laplacian = T0 - 2 T1 + T2
// 27 packed operations per pixel pair and row instead of ~34 scalar ones per pixel.  The smooth-pixel mask is
// a 0/1 per half (sign bit of ga - 50), the masked sum is one v_dot2_u32_u16.  Exact integers: same sums as
// k_estimate (compared on every test case).  A lane holds one 8-sample word (4 dwords) of the row; the sample
// left / right of the word comes from the neighbouring lane (DPP wave shifts).
// ---------------------------------------------------------------------------------
// (EST_GLOBAL, est_gptr, est_global and the load vectors est_u32x2, est_u32x4: strip_walk.hip.h)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 as_u(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ i16x2 as_i(uint32_t v) { return __builtin_bit_cast(i16x2, v); }
__device__ __forceinline__ uint32_t bits(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t bits(i16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t pk_abs(uint32_t v) {
  const i16x2 a = as_i(v), z = {0, 0};
  return bits(__builtin_elementwise_max(a, (i16x2)(z - a)));
}

// a * k + c per 16-bit half, k an inline constant (one instruction where the compiler writes a shift and an add)
__device__ __forceinline__ uint32_t pk_mad2(uint32_t a, uint32_t c) {
  uint32_t r;
  asm("v_pk_mad_u16 %0, %1, 2, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(c));
  return r;
}
__device__ __forceinline__ uint32_t pk_madm2(uint32_t a, uint32_t c) {
  uint32_t r;
  asm("v_pk_mad_i16 %0, %1, -2, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(c));
  return r;
}

struct EstRow {
  uint32_t H[4], S[4], T[4];
};

// the lane's word of row y as 4 dwords of packed 16-bit samples (zeros outside the plane)
template <int BPS>
__device__ __forceinline__ void est_load_pk(const EstFrame &fr, int y, int x0, int W, int H, bool fast, uint32_t (&w)[4]) {
  w[0] = w[1] = w[2] = w[3] = 0u;
  if (y < 0 || y >= H || x0 >= W || x0 + 8 <= 0) return;
  est_gptr row = est_global(fr.y) + (size_t)y * fr.stride;
  if (fast && x0 >= 0 && x0 + 8 <= W) {
    if (BPS == 2) {
      const est_u32x4 v = *(const EST_GLOBAL est_u32x4 *)(row + (size_t)x0 * 2);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
      const est_u32x2 v = *(const EST_GLOBAL est_u32x2 *)(row + x0);
      w[0] = __builtin_amdgcn_perm(0u, v.x, 0x0c010c00u);
      w[1] = __builtin_amdgcn_perm(0u, v.x, 0x0c030c02u);
      w[2] = __builtin_amdgcn_perm(0u, v.y, 0x0c010c00u);
      w[3] = __builtin_amdgcn_perm(0u, v.y, 0x0c030c02u);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // unaligned planes, words over an edge of the plane
    const int x = x0 + k;
    if (x >= 0 && x < W) {
      const uint32_t v = BPS == 2 ? (uint32_t)((const EST_GLOBAL uint16_t *)row)[x] : (uint32_t)row[x];
      w[k >> 1] |= v << (16 * (k & 1));
    }
  }
}

__device__ __forceinline__ void est_derive(const uint32_t (&c)[4], EstRow &r) {
  const uint32_t prev = (uint32_t)__builtin_amdgcn_mov_dpp((int)c[3], 0x138, 0xf, 0xf, true);  // wave_shr:1: lane - 1's last dword
  const uint32_t next = (uint32_t)__builtin_amdgcn_mov_dpp((int)c[0], 0x130, 0xf, 0xf, true);  // wave_shl:1: lane + 1's first
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t P = q ? c[q - 1] : prev, N = q < 3 ? c[q + 1] : next;
    const uint32_t l = __builtin_amdgcn_alignbyte(c[q], P, 2), rr = __builtin_amdgcn_alignbyte(N, c[q], 2);
    const uint32_t lr = bits((u16x2)(as_u(l) + as_u(rr)));
    r.H[q] = bits((u16x2)(as_u(l) - as_u(rr)));
    r.S[q] = pk_mad2(c[q], lr);
    r.T[q] = pk_madm2(c[q], lr);
  }
}

// Output rows per wave strip: chosen by the host (estimate_plan.h: whole resident rounds, at most kPkMaxStripRows rows -- the
// two 16-bit pixel counters of a lane hold 4 * rows each)
using g1s_est::kPkMaxStripRows;
static_assert(g1s_est::kPlanWavesPerWg == kWavesPerWg && g1s_est::kPlanColsPerWave == kColsPerWave, "estimate_plan.h restates strip_walk.hip.h");

// the fast form: the lane's word lies inside the plane's rows or wholly outside (then any in-plane word will do: every
// pixel it could reach is masked), the rows are 16-byte (8-byte) aligned: one unconditional vector load, nothing to wait for
// at the load -- the request for row y + 2 is in flight while row y is worked on
template <int BPS>
__device__ __forceinline__ void est_load_fast(est_gptr base, uint32_t stride, int y, uint32_t xoff, uint32_t (&w)[4]) {
  est_gptr p = base + (size_t)y * stride + xoff;
  if (BPS == 2) {
    const est_u32x4 v = *(const EST_GLOBAL est_u32x4 *)p;
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
    const est_u32x2 v = *(const EST_GLOBAL est_u32x2 *)p;
    w[0] = __builtin_amdgcn_perm(0u, v.x, 0x0c010c00u);
    w[1] = __builtin_amdgcn_perm(0u, v.x, 0x0c030c02u);
    w[2] = __builtin_amdgcn_perm(0u, v.y, 0x0c010c00u);
    w[3] = __builtin_amdgcn_perm(0u, v.y, 0x0c030c02u);
  }
}

template <int BPS, bool FAST>
__device__ __forceinline__ void est_strip(const EstFrame &fr, int W, int H, int shift, int x0, int y_first, int y_last, int lane,
                                          uint32_t &accum, uint32_t &count) {
  const uint32_t halfpk = shift ? 0x00010001u << (shift - 1) : 0u;
  // smooth: (|Gx| + |Gy| + half) >> shift < 50  <=>  |Gx| + |Gy| < (50 << shift) - half
  const uint32_t thrpk = 0x00010001u * (uint32_t)((kEdgeThreshold << shift) - (shift ? 1 << (shift - 1) : 0));
  const u16x2 sh = {(unsigned short)shift, (unsigned short)shift};
  // output columns of this lane: 1 <= x < W - 1, lanes 1 .. 62 (lanes 0 and 63 carry the halo columns)
  uint32_t cm[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int x = x0 + 2 * q;
    const bool ok = lane >= 1 && lane <= 62;
    cm[q] = (ok && x >= 1 && x < W - 1 ? 1u : 0u) | (ok && x + 1 >= 1 && x + 1 < W - 1 ? 0x10000u : 0u);
  }
  // (rows are wave-uniform: the row address is scalar arithmetic, the lane adds its column offset)
  const est_gptr base = est_global(fr.y);
  const uint32_t xoff = (uint32_t)(min(max(x0, 0), max(W - 8, 0)) * BPS);  // (FAST: W is a multiple of 8, >= 8)
  auto load = [&](int y, uint32_t (&w)[4]) __attribute__((always_inline)) {
    if (FAST) est_load_fast<BPS>(base, fr.stride, min(y, H - 1), xoff, w);
    else est_load_pk<BPS>(fr, y, x0, W, H, false, w);
  };
  uint32_t cnt = 0;
  const u16x2 fifteen = {15, 15};
  auto output = [&](const EstRow &a, const EstRow &b, const EstRow &c) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t gx = pk_mad2(b.H[q], bits((i16x2)(as_i(a.H[q]) + as_i(c.H[q]))));
      const uint32_t gy = bits((i16x2)(as_i(a.S[q]) - as_i(c.S[q])));
      const u16x2 g = as_u(pk_abs(gx)) + as_u(pk_abs(gy));  // <= 32760
      const uint32_t on = bits((u16x2)((u16x2)(g - as_u(thrpk)) >> fifteen)) & cm[q];
      const uint32_t v = pk_madm2(b.T[q], bits((i16x2)(as_i(a.T[q]) + as_i(c.T[q]))));
      const u16x2 lv = (u16x2)(as_u(pk_abs(v)) + as_u(halfpk)) >> sh;
      accum = __builtin_amdgcn_udot2(lv, as_u(on), accum, false);
      cnt += on;  // (two 16-bit counters: at most 4 * kPkMaxStripRows each)
    }
  };
  uint32_t w0[4], w1[4], w2[4];
  EstRow r0, r1, r2;
  load(y_first - 1, w0);
  est_derive(w0, r0);
  load(y_first, w0);
  est_derive(w0, r1);
  load(y_first + 1, w0);
  load(y_first + 2, w1);
  // three output rows a turn: the rows rotate through the names, not through registers; loads two rows ahead of their use
  // (the rows past the strip's last are requested and dropped)
  int y = y_first;
  for (; y + 3 <= y_last; y += 3) {
    load(y + 3, w2);
    est_derive(w0, r2);
    output(r0, r1, r2);
    load(y + 4, w0);
    est_derive(w1, r0);
    output(r1, r2, r0);
    load(y + 5, w1);
    est_derive(w2, r1);
    output(r2, r0, r1);
  }
  if (y < y_last) {
    est_derive(w0, r2);
    output(r0, r1, r2);
    if (y + 1 < y_last) {
      est_derive(w1, r0);
      output(r1, r2, r0);
    }
  }
  count = (cnt & 0xffffu) + (cnt >> 16);
}

template <int BPS>
__global__ __launch_bounds__(kStripThreads) void k_estimate_pk(EstParams ep) {
  const int frame = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int strip = blockIdx.x * kWavesPerWg + wave;
  if (strip >= ep.col_strips * ep.row_strips) return;
  const EstFrame fr = ep.frames[frame];
  const int W = ep.W, H = ep.H;
  const bool fast = (((uintptr_t)fr.y | fr.stride) & (BPS == 2 ? 15 : 7)) == 0 && (W & 7) == 0;  // (uniform)
  const StripCoords s = strip_coords(strip, ep.col_strips, lane, H, ep.strip_rows);
  uint32_t accum = 0, count = 0;
  if (fast) est_strip<BPS, true>(fr, W, H, ep.shift, s.x0, s.y_first, s.y_last, lane, accum, count);
  else est_strip<BPS, false>(fr, W, H, ep.shift, s.x0, s.y_first, s.y_last, lane, accum, count);
  for (int o = 32; o; o >>= 1) {
    accum += __shfl_down(accum, o);
    count += __shfl_down(count, o);
  }
  if (lane == 0 && (accum | count)) {
    atomicAdd(&ep.sums[2 * frame], (unsigned long long)accum);
    atomicAdd(&ep.sums[2 * frame + 1], (unsigned long long)count);
  }
}

constexpr double kSqrtPiBy2 = 1.2533141373155003;  // SQRT_PI_BY_2

}  // namespace

using namespace g1s_op;

struct g1s_estimate {
  Stream stream;  // (first: it goes last, after what was used on it)
  int device = 0;
  uint32_t bit_depth = 8;
  uint32_t W = 0, H = 0, bps = 0;
  uint32_t batch = 32;
  std::vector<EstFrame> h_frames;  // the batch being filled
  DevBuf<EstFrame> d_frames;
  DevBuf<unsigned long long> d_sums;
  PinnedBuf<unsigned long long> h_sums;
  DevBuf<uint8_t> d_stage;         // device copies of host frames: rows as in the staging layout, no gap between frames
  size_t stage_row = 0;
  std::vector<double> estimates;   // one per frame: sigma, or -1 (None)
  std::vector<uint64_t> sums;      // beside them, from the same words: accum, count per frame
  g1s_estimate_launch_t last = {};  // the last batch's launch (g1s_estimate_last_launch)
  std::string err;
  uint64_t frames_kernel = 0;
  double ms_kernel = 0;
  bool timing = false;
  Event ev0, ev1;

  int fail(int code, const std::string &m) {
    err = m;
    return code;
  }
  int flush();
};

int g1s_estimate::flush() {
  const uint32_t B = (uint32_t)h_frames.size();
  if (!B) return G1S_OK;
  G1S_OP_TRY(hipMemcpyAsync(d_frames, h_frames.data(), sizeof(EstFrame) * B, hipMemcpyHostToDevice, stream));
  G1S_OP_TRY(hipMemsetAsync(d_sums, 0, sizeof(unsigned long long) * 2 * B, stream));
  EstParams ep;
  ep.frames = d_frames;
  ep.sums = d_sums;
  ep.W = (int)W;
  ep.H = (int)H;
  ep.bps = (int)bps;
  ep.shift = (int)bit_depth - 8;
  // depths up to 12 bits: the packed 16-bit kernel; deeper samples (or G1S_ESTIMATE=wide, a test aid): 32-bit arithmetic
  const char *mode = getenv("G1S_ESTIMATE");
  const bool packed = bit_depth <= 12 && !(mode && std::strcmp(mode, "wide") == 0);
  ep.col_strips = g1s_est::plan_col_strips((int)W);
  ep.strip_rows = kStripRows;
  ep.row_strips = ((int)H - 2 + kStripRows - 1) / kStripRows;
  // a plane without interior pixels (one or two samples wide or high; one sample wide: no column strip at all) launches nothing
  const bool launch = W >= 3 && H >= 3;
  int cus = 256, wgs_per_cu = 0;
  if (packed && launch) {
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (bps == 2) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs_per_cu, k_estimate_pk<2>, kStripThreads, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs_per_cu, k_estimate_pk<1>, kStripThreads, 0);
    // G1S_ESTIMATE_ROWS=N (a test and measurement aid, read at every batch): the packed launch takes strips of N rows, not the
    // plan's; an N outside 8 .. 256 is clamped into that range (0 or no number: the plan's).  The 32-bit kernel's stay kStripRows.
    const char *rows_env = getenv("G1S_ESTIMATE_ROWS");
    const int forced = rows_env ? std::atoi(rows_env) : 0;
    const g1s_est::StripPlan plan = g1s_est::plan_strips((int)H, ep.col_strips, (int)B, cus, wgs_per_cu, forced);
    ep.strip_rows = plan.strip_rows;
    ep.row_strips = plan.row_strips;
  }
  last.strip_rows = (uint32_t)ep.strip_rows;
  last.row_strips = (uint32_t)std::max(ep.row_strips, 0);
  last.packed = packed;
  last.launched = launch;
  last.cus = packed && launch ? cus : 0;
  last.wgs_per_cu = packed && launch ? wgs_per_cu : 0;
  if (launch) {
    const dim3 grid((ep.col_strips * ep.row_strips + kWavesPerWg - 1) / kWavesPerWg, B);
    if (timing) G1S_OP_TRY(hipEventRecord(ev0, stream));
    if (packed && bps == 2) hipLaunchKernelGGL(k_estimate_pk<2>, grid, dim3(kStripThreads), 0, stream, ep);
    else if (packed) hipLaunchKernelGGL(k_estimate_pk<1>, grid, dim3(kStripThreads), 0, stream, ep);
    else if (bps == 2) hipLaunchKernelGGL(k_estimate<2>, grid, dim3(kStripThreads), 0, stream, ep);
    else hipLaunchKernelGGL(k_estimate<1>, grid, dim3(kStripThreads), 0, stream, ep);
    if (timing) G1S_OP_TRY(hipEventRecord(ev1, stream));
  }
  G1S_OP_TRY(hipMemcpyAsync(h_sums, d_sums, sizeof(unsigned long long) * 2 * B, hipMemcpyDeviceToHost, stream));
  G1S_OP_TRY(hipStreamSynchronize(stream));
  G1S_OP_TRY(hipGetLastError());
  if (timing && launch) {
    float ms = 0;
    G1S_OP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    ms_kernel += ms;
    frames_kernel += B;
  }
  for (uint32_t i = 0; i < B; ++i) {
    const unsigned long long accum = h_sums[2 * i], count = h_sums[2 * i + 1];
    // (count < 16) ? None : accum as f64 / (6 * count) as f64 * SQRT_PI_BY_2
    estimates.push_back(count < 16 ? -1.0 : (double)accum / (double)(6 * count) * kSqrtPiBy2);
    sums.push_back(accum);
    sums.push_back(count);
  }
  h_frames.clear();
  return G1S_OK;
}

extern "C" {

g1s_estimate_t *g1s_estimate_new(uint32_t bit_depth, int32_t device, uint32_t batch_frames) {
  if (bit_depth < 8 || bit_depth > 16) return nullptr;
  if (!pick_device(device, "estimate", &device).empty()) return nullptr;  // (no global error: the caller sees only the null)
  g1s_estimate *e = new g1s_estimate;
  e->device = device;
  e->bit_depth = bit_depth;
  e->bps = bit_depth > 8 ? 2 : 1;
  e->batch = batch_of(batch_frames);
  if (!open_stream(device, e->stream) || hipMalloc((void **)&e->d_frames.p, sizeof(EstFrame) * e->batch) != hipSuccess ||
      hipMalloc((void **)&e->d_sums.p, sizeof(unsigned long long) * 2 * e->batch) != hipSuccess ||
      hipHostMalloc((void **)&e->h_sums.p, sizeof(unsigned long long) * 2 * e->batch, hipHostMallocDefault) != hipSuccess ||
      hipEventCreate(&e->ev0.p) != hipSuccess || hipEventCreate(&e->ev1.p) != hipSuccess) {
    g1s_estimate_free(e);
    return nullptr;
  }
  return e;
}

int g1s_estimate_frame(g1s_estimate_t *e, const g1s_frame_t *f) {
  if (!e || !f || !f->data[0]) return G1S_ERR_INVALID;
  (void)hipSetDevice(e->device);
  if ((f->bytes_per_sample == 1) != (e->bit_depth == 8) || (f->bytes_per_sample != 1 && f->bytes_per_sample != 2))
    return e->fail(G1S_ERR_INVALID, "bytes_per_sample does not match the bit depth given to g1s_estimate_new");
  if (f->width < 1 || f->height < 1) return e->fail(G1S_ERR_INVALID, "empty frame");
  if (!e->W) {
    e->W = f->width;
    e->H = f->height;
    e->stage_row = align_up((size_t)e->W * e->bps, kStageRowAlign);
  } else if (e->W != f->width || e->H != f->height) {
    return e->fail(G1S_ERR_DIM_MISMATCH, "frame geometry changed mid-stream");
  }
  EstFrame ef;
  if (f->on_device == 1) {
    ef.y = static_cast<const uint8_t *>(f->data[0]);
    ef.stride = (uint32_t)f->stride_bytes[0];
  } else {  // host planes: copied before the call returns (the `&frame.y_plane` borrow)
    const size_t row = e->stage_row, stage_frame = row * e->H;
    if (!e->d_stage && hipMalloc((void **)&e->d_stage.p, stage_frame * e->batch) != hipSuccess)
      return e->fail(G1S_ERR_HIP, "hipMalloc of the staging buffer failed");
    uint8_t *dst = e->d_stage + stage_frame * e->h_frames.size();
    if (hipMemcpy2D(dst, row, f->data[0], f->stride_bytes[0], (size_t)e->W * e->bps, e->H, hipMemcpyHostToDevice) != hipSuccess)
      return e->fail(G1S_ERR_HIP, "hipMemcpy2D of a host frame failed");
    ef.y = dst;
    ef.stride = (uint32_t)row;
  }
  e->h_frames.push_back(ef);
  return e->h_frames.size() == e->batch ? e->flush() : G1S_OK;
}

int g1s_estimate_finish(g1s_estimate_t *e, double *out, size_t cap, size_t *n_out) {
  if (!e) return G1S_ERR_INVALID;
  (void)hipSetDevice(e->device);
  const int rc = e->flush();
  if (rc) return rc;
  if (n_out) *n_out = e->estimates.size();
  if (e->estimates.size() > cap || (!out && !e->estimates.empty())) return e->fail(G1S_ERR_CAPACITY, "estimate buffer too small");
  if (!e->estimates.empty()) std::memcpy(out, e->estimates.data(), sizeof(double) * e->estimates.size());
  return G1S_OK;
}

int g1s_estimate_set_timing(g1s_estimate_t *e, int enable, double *ms_kernel, uint64_t *frames) {
  if (!e) return G1S_ERR_INVALID;
  e->timing = enable != 0;
  if (ms_kernel) *ms_kernel = e->ms_kernel;
  if (frames) *frames = e->frames_kernel;
  return G1S_OK;
}

int g1s_estimate_last_launch(g1s_estimate_t *e, g1s_estimate_launch_t *launch, uint64_t *sums, size_t cap, size_t *n_out) {
  if (!e) return G1S_ERR_INVALID;
  if (launch) *launch = e->last;
  const size_t n = e->sums.size() / 2;
  if (n_out) *n_out = n;
  if (!sums && !cap) return G1S_OK;  // the launch alone
  if (n > cap || (!sums && n)) return e->fail(G1S_ERR_CAPACITY, "sums buffer too small");
  if (n) std::memcpy(sums, e->sums.data(), sizeof(uint64_t) * 2 * n);
  return G1S_OK;
}

const char *g1s_estimate_last_error(const g1s_estimate_t *e) { return e ? e->err.c_str() : ""; }

void g1s_estimate_free(g1s_estimate_t *e) { free_op(e); }

long g1s_format_estimates(const double *estimates, size_t n, char *buf, size_t cap) {
  // writeln!("filmgrn1"), then writeln!("{:.3}", estimate.unwrap_or(-1f64)) per frame (src/main.rs:597-600)
  std::string s = "filmgrn1\n";
  char line[64];
  for (size_t i = 0; i < n; ++i) {
    snprintf(line, sizeof(line), "%.3f\n", estimates[i]);
    s += line;
  }
  if (s.size() > cap) return G1S_ERR_CAPACITY;
  std::memcpy(buf, s.data(), s.size());
  return (long)s.size();
}

}  // extern "C"
