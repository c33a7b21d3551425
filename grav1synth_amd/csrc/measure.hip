// measure.hip -- `measure` and `check`: exact grain statistics of a frame pair on the device.
//
// The statistics are defined in include/g1s_diff.h ("measure", rules 1 - 6); tests/measure_ref.py restates them in numpy.
// Two kernels:
//
//   km_measure<BPS>  a workgroup per (tile, plane of the class, frame pair).  The tile's d = a - b goes into LDS as int16
//                    with a halo of 3 columns either side and 3 rows above (zeros outside the plane: a product with a
//                    sample outside it is skipped by being 0), the tile's bins beside it as bytes.  A wave walks 32 rows
//                    of the tile top to bottom, a lane a column, with the 4 x 7 window of rule 4 in registers: 7 LDS
//                    reads and 25 multiply-adds a sample.  Every sample of a and b comes from HBM once, apart from halos
//                    (and the clean luma a chroma sample is binned by).  The workgroup's partial record goes out with
//                    plain stores.
//   km_tail          a workgroup per (plane, frame pair) sums the partial records into the pair's record.
// A temporal meter (rules 7 - 11) runs km_measure_t and km_tail<4> behind them: they stand below km_tail with their own notes.
// A cross meter (rules 12 - 17) runs km_measure_x and km_tail<4> behind those: below km_measure_t.
// A scales meter (rules 18 - 23) runs km_measure_s and km_tail_s behind those: below km_measure_x, with their own notes.
// What the kernels share stands in front of them: the parameters of a launch over a plane class (ClassParams) and the bin of a
// sample (clean_bin); km_tail is one template for the plain and the temporal layout.  lag_pass, the 5 x 5 row loop of
// km_measure_x's three pairings, stands before km_measure_t, which has the same loop written out: calling lag_pass from it,
// and one epilogue helper for the waves' accumulators, gave km_measure, km_measure_s and km_measure_t other code than what
// was measured before, and timing rows above it (profiles/measure_refactor.txt).  The kernels compile to that code again.  The host engine below them keeps a RecordLane (meter_op.h, shared with the noise levels) a record kind.  What is done
// with the records on the host -- the sums and the four reports -- needs no device and is in measure_report.cpp; the file
// commands (`measure`, `check`) stand above the per-frame calls in measure_file.cpp.
//
// The 32-bit sums and why they hold at 12 bits (|d| <= 4095, a product below 2^24):
//   * a lane's 25 lag sums take one product a row and are handed on after the wave's 32 rows: below 2^29.  Across the
//     lanes they are added as two 16-bit halves (each wave sum below 2^23), put together in 64 bits.
//   * a lane's bin sums run while its column stays in one bin, 32 rows at the most: n <= 32, |s1| < 2^17, s2 < 2^29;
//     across the lanes s2 goes as two halves like the lag sums.
// The bins: a lane keeps the sums of the bin its column is in and hands them on when the bin changes.  Handing on is
// done by the wave, not by the lane: for every distinct bin among the lanes that hand on, one masked DPP reduction and one
// LDS update by one lane -- a frame of one intensity costs a wave one such update a tile, not 64 additions to one word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/g1s_diff.h"
#include "meter_op.h"
#include "wave_sum.hip.h"

namespace {

using g1s_op::TailParams;

constexpr int kTW = 64, kTH = 128, kHalo = 3;
constexpr int kLW = kTW + 2 * kHalo, kLH = kTH + kHalo;  // the LDS tile: halo left, right and above
constexpr int kWaves = 4, kThreads = 64 * kWaves, kRowsPerWave = kTH / kWaves;
constexpr int kBins = 32, kLags = 25;
constexpr int kEntries = 3 * kBins + kLags;  // a partial record: n[32], s1[32], s2[32], r[25]
constexpr int kNoBin = 0xff;
constexpr int kTailThreads = 512;
static_assert(kRowsPerWave <= 127, "a 32-bit lag sum holds 127 products of 12-bit residuals");
static_assert(sizeof(g1s_measure_record_t) == 8 * 3 * kEntries, "km_tail<3> writes the record as 64-bit words");

struct MeasureJob {
  const uint8_t *a[3], *b[3];
  uint32_t a_stride[3], b_stride[3];  // bytes
};

// A launch over a plane class (km_measure, km_measure_t; km_measure_s has ScaleParams, the same with the luma height): luma
// alone, or both chroma planes as grid.y.  A workgroup takes a unit of a plane -- a tile, or km_measure_s's strip of tiles --
// for job blockIdx.z.
template <class Job>
struct ClassParams {
  const Job *jobs;
  unsigned long long *partials;  // [job][units_frame][the kernel's entries]
  int pw, ph, units_x;           // the class's plane size, the units across it
  int plane0;                    // first plane of the class: 0 luma, 1 chroma
  int W, xdec, ydec, shift;      // luma width, chroma decimation, B - 5
  uint32_t units_frame, unit_base, units_plane;
};

template <int BPS>
__device__ __forceinline__ int sample(const uint8_t *plane, uint32_t stride, int x, int y) {
  const uint8_t *row = plane + (size_t)y * stride;
  return BPS == 2 ? (int)reinterpret_cast<const uint16_t *>(row)[x] : (int)row[x];
}

// (clean_bin takes a launch's parameters as values, not as the struct: a kernel that hands the address of its parameter
// struct to a function, a member function included, loses the compiler's knowledge that the planes are global memory, and
// its sample loads become flat loads.)
// the bin of the sample at (x, y) of plane c whose clean value is b: by the clean frame's luma (py, W samples wide), for
// chroma its averageLuma
template <int BPS>
__device__ __forceinline__ int clean_bin(int c, int b, const uint8_t *py, uint32_t sy, int x, int y, int W, int xdec, int ydec, int shift) {
  int I = b;
  if (c) {
    const int xs = x << xdec, ys = y << ydec;
    I = sample<BPS>(py, sy, xs, ys);
    if (xdec) I = (I + sample<BPS>(py, sy, min(xs + 1, W - 1), ys) + 1) >> 1;
  }
  return min(I >> shift, kBins - 1);  // (a sample above the depth's maximum: the caller's error, not a wild index)
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void km_measure(ClassParams<MeasureJob> p) {
  __shared__ int16_t s_d[kLH * kLW];
  __shared__ uint8_t s_bin[kTH * kTW];
  __shared__ unsigned long long s_acc[kWaves][kEntries];  // (two's complement: the signed sums are added as unsigned)
  const MeasureJob &job = p.jobs[blockIdx.z];
  const int c = p.plane0 + (int)blockIdx.y;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = (int)blockIdx.x / p.units_x, tx = (int)blockIdx.x - ty * p.units_x;
  const int x0 = tx * kTW, y0 = ty * kTH;
  const uint8_t *pa = job.a[c], *pb = job.b[c], *py = job.b[0];
  const uint32_t sa = job.a_stride[c], sb = job.b_stride[c], sy = job.b_stride[0];

  for (int i = tid; i < kWaves * kEntries; i += kThreads) (&s_acc[0][0])[i] = 0;
  // the tile of d with its halo, and the bins of the tile's own samples
  for (int i = tid; i < kLH * kLW; i += kThreads) {
    const int ly = i / kLW, lx = i - ly * kLW;
    const int x = x0 + lx - kHalo, y = y0 + ly - kHalo;
    const bool inside = x >= 0 && x < p.pw && y >= 0 && y < p.ph;
    const bool own = lx >= kHalo && lx < kHalo + kTW && ly >= kHalo;
    int d = 0, bin = kNoBin;
    if (inside) {
      const int b = sample<BPS>(pb, sb, x, y);
      d = sample<BPS>(pa, sa, x, y) - b;
      if (own) bin = clean_bin<BPS>(c, b, py, sy, x, y, p.W, p.xdec, p.ydec, p.shift);
    }
    s_d[i] = (int16_t)d;
    if (own) s_bin[(ly - kHalo) * kTW + (lx - kHalo)] = (uint8_t)bin;
  }
  __syncthreads();

  // the wave's rows of the tile that the plane has (uniform)
  const int row0 = wave * kRowsPerWave, rows = min(kRowsPerWave, p.ph - (y0 + row0));
  if (rows > 0) {
    int acc[kLags];
#pragma unroll
    for (int i = 0; i < kLags; ++i) acc[i] = 0;
    // the window: rows y - 3 .. y of the LDS tile, columns x - 3 .. x + 3 (LDS row ly = tile row + 3, column lx = lane + 3 + dx)
    int w[4][7];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 7; ++k) w[r + 1][k] = s_d[(row0 + r) * kLW + lane + k];
    int cur = -1, bn = 0, bs1 = 0, bs2 = 0;  // the bin the lane's column is in and its sums so far (cur < 0: none)
    unsigned long long *mine = s_acc[wave];
    // hands on the bin sums of the lanes with `go` set: a reduction and an update a distinct bin
    auto hand_on = [&](bool go) __attribute__((always_inline)) {
      unsigned long long todo = __builtin_amdgcn_ballot_w64(go);
      while (todo) {
        const int b = __builtin_amdgcn_readlane(cur, (int)__builtin_ctzll(todo));
        const bool m = go && cur == b;
        todo &= ~__builtin_amdgcn_ballot_w64(m);
        const int n = wave_sum(m ? bn : 0), s1 = wave_sum(m ? bs1 : 0);
        const long long s2 = wave_sum_wide(m ? bs2 : 0);
        if (lane == 0) {
          mine[b] += (unsigned long long)(long long)n;
          mine[kBins + b] += (unsigned long long)(long long)s1;
          mine[2 * kBins + b] += (unsigned long long)s2;
        }
        if (m) cur = -1, bn = bs1 = bs2 = 0;
      }
    };
    for (int r = 0; r < rows; ++r) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int k = 0; k < 7; ++k) w[q][k] = w[q + 1][k];
#pragma unroll
      for (int k = 0; k < 7; ++k) w[3][k] = s_d[(row0 + r + kHalo) * kLW + lane + k];
      const int d = w[3][3];
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[q * 7 + k] += __mul24(d, w[q][k]);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[21 + k] += __mul24(d, w[3][k]);
      const int dd = __mul24(d, d);
      acc[24] += dd;
      const int k = s_bin[(row0 + r) * kTW + lane];
      const bool change = cur >= 0 && k != cur;
      if (__builtin_amdgcn_ballot_w64(change)) hand_on(change);
      if (k != kNoBin) cur = k, bn += 1, bs1 += d, bs2 += dd;
    }
    hand_on(cur >= 0);
#pragma unroll
    for (int i = 0; i < kLags; ++i) {
      const long long t = wave_sum_wide(acc[i]);
      if (lane == 0) mine[3 * kBins + i] = (unsigned long long)t;
    }
  }
  __syncthreads();
  if (tid < kEntries) {
    unsigned long long t = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) t += s_acc[v][tid];
    const size_t at = (size_t)blockIdx.z * p.units_frame + p.unit_base + (size_t)blockIdx.y * p.units_plane + blockIdx.x;
    p.partials[at * kEntries + tid] = t;
  }
}

// The job's record from its workgroups' partial records: grid (plane, job).  FIELDS bin fields of 32 and 25 offsets a
// partial record and a plane of the record: km_tail<3> writes g1s_measure_record_t (n, s1, s2, r) with 4 groups of 128
// threads, km_tail<4> g1s_measure_trecord_t (n, x, u, v, c) with 2 groups of 256; a thread of a group an entry, a group
// every GROUPS-th partial record.
template <int FIELDS>
__global__ __launch_bounds__(kTailThreads) void km_tail(TailParams p) {
  constexpr int N = FIELDS * kBins + kLags, WIDTH = N <= 128 ? 128 : 256, GROUPS = kTailThreads / WIDTH;
  static_assert(N <= WIDTH, "km_tail gives an entry a thread of a group");
  __shared__ unsigned long long s_sum[GROUPS][WIDTH];
  const int c = (int)blockIdx.x, i = (int)threadIdx.x % WIDTH, g = (int)threadIdx.x / WIDTH;
  const unsigned long long *src = p.partials + ((size_t)blockIdx.y * p.units_frame + p.unit_base[c]) * N;
  unsigned long long t = 0;
  if (i < N)
    for (uint32_t k = (uint32_t)g; k < p.units[c]; k += GROUPS) t += src[(size_t)k * N + i];
  s_sum[g][i] = t;
  __syncthreads();
  if (g == 0 && i < N) {
    for (int v = 1; v < GROUPS; ++v) t += s_sum[v][i];
    // the record as 64-bit words: the bin fields [3][32] one after the other, then the offsets [3][25]
    unsigned long long *rec = p.records + (size_t)blockIdx.y * (3 * N);
    const int field = i < FIELDS * kBins ? i / kBins : FIELDS, k = i - field * kBins;
    rec[field < FIELDS ? field * 3 * kBins + c * kBins + k : 3 * FIELDS * kBins + c * kLags + k] = t;
  }
}

// ---- the temporal record (rules 7 - 11): the residual of pair t against the residual of pair t - 1 ----
//   km_measure_t<BPS>  a workgroup per (tile, plane of the class, temporal job), km_measure's tile, waves and plane classes.
//                      LDS: d_t of the tile as int16 without a halo; d_{t-1} as int16 with a halo of 2 on all four sides
//                      (zeros outside the plane: a skipped product is a product with 0); the tile's bins as bytes, from
//                      pair t's clean frame; the waves' accumulators.  A wave walks its 32 rows, a lane a column, with the
//                      5 x 5 window of d_{t-1} in registers: 5 LDS reads of d_{t-1} and 25 multiply-adds a sample.
//   km_tail<4>         km_tail for the partial records of km_measure_t.
// The 32-bit sums follow km_measure's schedule: a lane's 25 lag sums and its bin sums (n, x, u, v) take one product a row
// for the wave's 32 rows at the most (below 2^29 in size) and go on in 64 bits through wave_sum_wide, which carries the
// signed x and c as it carries km_measure's lag sums.
constexpr int kTHalo = 2, kTWin = 2 * kTHalo + 1;
constexpr int kPW = kTW + 2 * kTHalo, kPH = kTH + 2 * kTHalo;  // the LDS tile of d_{t-1}
constexpr int kTLags = kTWin * kTWin;
constexpr int kTEntries = 4 * kBins + kTLags;  // a partial temporal record: n[32], x[32], u[32], v[32], c[25]
static_assert(kRowsPerWave <= 127, "a 32-bit sum of km_measure_t holds 127 products of 12-bit residuals, one a row");
static_assert(kTLags == kLags, "g1s_measure_trecord_t has 25 offsets, as km_tail takes them");
static_assert(sizeof(g1s_measure_trecord_t) == 8 * 3 * kTEntries, "km_tail<4> writes the record as 64-bit words");

struct TemporalJob {
  MeasureJob cur, prev;  // pair t and pair t - 1 of the run
};

// The row loop of km_measure_x's pairings (km_measure_t below has it written out), over the wave's rows: a = the tile's own sample, from a plane
// stored with the halo (HALO_A, kPW wide) or without (kTW wide); b = the 5 x 5 window round it in a plane with the halo.
// Into `mine`: the bin sums n, x = sum a b, u = sum a^2, v = sum b^2 at offset (0, 0), then the 25 lag sums.
template <bool HALO_A>
__device__ __forceinline__ void lag_pass(const int16_t *s_a, const int16_t *s_b, const uint8_t *s_bin, unsigned long long *mine, int row0, int rows,
                                         int lane) {
  int acc[kTLags];
#pragma unroll
  for (int i = 0; i < kTLags; ++i) acc[i] = 0;
  // the window: rows y - 2 .. y + 2 of b, columns x - 2 .. x + 2 (LDS row ly = tile row + 2 + dy, column lx = lane + 2 + dx)
  int w[kTWin][kTWin];
#pragma unroll
  for (int q = 0; q < kTWin - 1; ++q)
#pragma unroll
    for (int k = 0; k < kTWin; ++k) w[q + 1][k] = s_b[(row0 + q) * kPW + lane + k];
  int cur = -1, bn = 0, bx = 0, bu = 0, bv = 0;  // the bin the lane's column is in and its sums so far (cur < 0: none)
  auto hand_on = [&](bool go) __attribute__((always_inline)) {
    unsigned long long todo = __builtin_amdgcn_ballot_w64(go);
    while (todo) {
      const int b = __builtin_amdgcn_readlane(cur, (int)__builtin_ctzll(todo));
      const bool m = go && cur == b;
      todo &= ~__builtin_amdgcn_ballot_w64(m);
      const int n = wave_sum(m ? bn : 0);
      const long long x = wave_sum_wide(m ? bx : 0), u = wave_sum_wide(m ? bu : 0), v = wave_sum_wide(m ? bv : 0);
      if (lane == 0) {
        mine[b] += (unsigned long long)(long long)n;
        mine[kBins + b] += (unsigned long long)x;
        mine[2 * kBins + b] += (unsigned long long)u;
        mine[3 * kBins + b] += (unsigned long long)v;
      }
      if (m) cur = -1, bn = bx = bu = bv = 0;
    }
  };
  for (int r = 0; r < rows; ++r) {
#pragma unroll
    for (int q = 0; q < kTWin - 1; ++q)
#pragma unroll
      for (int k = 0; k < kTWin; ++k) w[q][k] = w[q + 1][k];
#pragma unroll
    for (int k = 0; k < kTWin; ++k) w[kTWin - 1][k] = s_b[(row0 + r + kTWin - 1) * kPW + lane + k];
    const int d = HALO_A ? (int)s_a[(row0 + r + kTHalo) * kPW + lane + kTHalo] : (int)s_a[(row0 + r) * kTW + lane];
#pragma unroll
    for (int q = 0; q < kTWin; ++q)
#pragma unroll
      for (int k = 0; k < kTWin; ++k) acc[q * kTWin + k] += __mul24(d, w[q][k]);
    const int e = w[kTHalo][kTHalo];
    const int k = s_bin[(row0 + r) * kTW + lane];
    const bool change = cur >= 0 && k != cur;
    if (__builtin_amdgcn_ballot_w64(change)) hand_on(change);
    if (k != kNoBin) cur = k, bn += 1, bx += __mul24(d, e), bu += __mul24(d, d), bv += __mul24(e, e);
  }
  hand_on(cur >= 0);
#pragma unroll
  for (int i = 0; i < kTLags; ++i) {
    const long long t = wave_sum_wide(acc[i]);
    if (lane == 0) mine[4 * kBins + i] = (unsigned long long)t;
  }
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void km_measure_t(ClassParams<TemporalJob> p) {
  __shared__ int16_t s_d[kTH * kTW];
  __shared__ int16_t s_p[kPH * kPW];
  __shared__ uint8_t s_bin[kTH * kTW];
  __shared__ unsigned long long s_acc[kWaves][kTEntries];  // (two's complement, as km_measure's)
  const TemporalJob &job = p.jobs[blockIdx.z];
  const int c = p.plane0 + (int)blockIdx.y;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = (int)blockIdx.x / p.units_x, tx = (int)blockIdx.x - ty * p.units_x;
  const int x0 = tx * kTW, y0 = ty * kTH;
  const uint8_t *pa = job.cur.a[c], *pb = job.cur.b[c], *py = job.cur.b[0], *qa = job.prev.a[c], *qb = job.prev.b[c];
  const uint32_t sa = job.cur.a_stride[c], sb = job.cur.b_stride[c], sy = job.cur.b_stride[0];
  const uint32_t ta = job.prev.a_stride[c], tb = job.prev.b_stride[c];

  for (int i = tid; i < kWaves * kTEntries; i += kThreads) (&s_acc[0][0])[i] = 0;
  // d_{t-1} of the tile with its halo; for the tile's own samples d_t and the bin beside it
  for (int i = tid; i < kPH * kPW; i += kThreads) {
    const int ly = i / kPW, lx = i - ly * kPW;
    const int x = x0 + lx - kTHalo, y = y0 + ly - kTHalo;
    const bool inside = x >= 0 && x < p.pw && y >= 0 && y < p.ph;
    const bool own = lx >= kTHalo && lx < kTHalo + kTW && ly >= kTHalo && ly < kTHalo + kTH;
    int d = 0, e = 0, bin = kNoBin;
    if (inside) {
      e = sample<BPS>(qa, ta, x, y) - sample<BPS>(qb, tb, x, y);
      if (own) {
        const int b = sample<BPS>(pb, sb, x, y);
        d = sample<BPS>(pa, sa, x, y) - b;
        bin = clean_bin<BPS>(c, b, py, sy, x, y, p.W, p.xdec, p.ydec, p.shift);  // (pair t's clean frame)
      }
    }
    s_p[i] = (int16_t)e;
    if (own) {
      const int at = (ly - kTHalo) * kTW + (lx - kTHalo);
      s_d[at] = (int16_t)d;
      s_bin[at] = (uint8_t)bin;
    }
  }
  __syncthreads();

  const int row0 = wave * kRowsPerWave, rows = min(kRowsPerWave, p.ph - (y0 + row0));
  if (rows > 0) {
    int acc[kTLags];
#pragma unroll
    for (int i = 0; i < kTLags; ++i) acc[i] = 0;
    // the window: rows y - 2 .. y + 2 of d_{t-1}, columns x - 2 .. x + 2 (LDS row ly = tile row + 2 + dy, column lx = lane + 2 + dx)
    int w[kTWin][kTWin];
#pragma unroll
    for (int q = 0; q < kTWin - 1; ++q)
#pragma unroll
      for (int k = 0; k < kTWin; ++k) w[q + 1][k] = s_p[(row0 + q) * kPW + lane + k];
    int cur = -1, bn = 0, bx = 0, bu = 0, bv = 0;  // the bin the lane's column is in and its sums so far (cur < 0: none)
    unsigned long long *mine = s_acc[wave];
    auto hand_on = [&](bool go) __attribute__((always_inline)) {
      unsigned long long todo = __builtin_amdgcn_ballot_w64(go);
      while (todo) {
        const int b = __builtin_amdgcn_readlane(cur, (int)__builtin_ctzll(todo));
        const bool m = go && cur == b;
        todo &= ~__builtin_amdgcn_ballot_w64(m);
        const int n = wave_sum(m ? bn : 0);
        const long long x = wave_sum_wide(m ? bx : 0), u = wave_sum_wide(m ? bu : 0), v = wave_sum_wide(m ? bv : 0);
        if (lane == 0) {
          mine[b] += (unsigned long long)(long long)n;
          mine[kBins + b] += (unsigned long long)x;
          mine[2 * kBins + b] += (unsigned long long)u;
          mine[3 * kBins + b] += (unsigned long long)v;
        }
        if (m) cur = -1, bn = bx = bu = bv = 0;
      }
    };
    for (int r = 0; r < rows; ++r) {
#pragma unroll
      for (int q = 0; q < kTWin - 1; ++q)
#pragma unroll
        for (int k = 0; k < kTWin; ++k) w[q][k] = w[q + 1][k];
#pragma unroll
      for (int k = 0; k < kTWin; ++k) w[kTWin - 1][k] = s_p[(row0 + r + kTWin - 1) * kPW + lane + k];
      const int d = s_d[(row0 + r) * kTW + lane];
#pragma unroll
      for (int q = 0; q < kTWin; ++q)
#pragma unroll
        for (int k = 0; k < kTWin; ++k) acc[q * kTWin + k] += __mul24(d, w[q][k]);
      const int e = w[kTHalo][kTHalo];
      const int k = s_bin[(row0 + r) * kTW + lane];
      const bool change = cur >= 0 && k != cur;
      if (__builtin_amdgcn_ballot_w64(change)) hand_on(change);
      if (k != kNoBin) cur = k, bn += 1, bx += __mul24(d, e), bu += __mul24(d, d), bv += __mul24(e, e);
    }
    hand_on(cur >= 0);
#pragma unroll
    for (int i = 0; i < kTLags; ++i) {
      const long long t = wave_sum_wide(acc[i]);
      if (lane == 0) mine[4 * kBins + i] = (unsigned long long)t;
    }
  }
  __syncthreads();
  if (tid < kTEntries) {
    unsigned long long t = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) t += s_acc[v][tid];
    const size_t at = (size_t)blockIdx.z * p.units_frame + p.unit_base + (size_t)blockIdx.y * p.units_plane + blockIdx.x;
    p.partials[at * kTEntries + tid] = t;
  }
}

// ---- the cross record (rules 12 - 17): the chroma residuals against the luma residual under them, and against each other ----
//   km_measure_x<BPS>  a workgroup per (chroma tile, pair), km_measure_t's tile and waves with other operands.  LDS: d_Cb of
//                      the tile as int16 without a halo; d_Cr and L (rule 12: the rounded mean of the luma residual under a
//                      chroma sample, formed here from the (1 + xdec)(1 + ydec) luma samples of both frames) as int16 with a
//                      halo of 2 on all four sides, zeros outside the chroma plane; the tile's bins as bytes; ONE set of the
//                      waves' accumulators.  Everything is loaded once a tile; the three pairings (d_Cb, L), (d_Cr, L),
//                      (d_Cb, d_Cr) then walk the tile one after another through one set of 25 lag accumulators and one set
//                      of running bin sums (lag_pass), and the workgroup's partial record of a pairing goes out with
//                      plain stores before the next one starts.
//   km_tail<4>         sums the partials unchanged: they lie as [pair][pairing][tile][kTEntries], so that a "plane" is a
//                      pairing and all three tile counts are the chroma plane's.
// The 32-bit sums are km_measure_t's: |L| <= 2^B - 1 (a rounded mean of residuals), so every product stays below 2^24.
constexpr int kXLdsBytes = 2 * kTH * kTW + 2 * 2 * kPH * kPW + kTH * kTW + 8 * kWaves * kTEntries;
static_assert(kRowsPerWave <= 127, "a 32-bit sum of km_measure_x holds 127 products of 12-bit residuals, one a row");
static_assert(sizeof(g1s_measure_xrecord_t) == 8 * 3 * kTEntries, "km_tail<4> writes the cross record as 64-bit words");
static_assert(kXLdsBytes == 65376 && kXLdsBytes <= 65536, "km_measure_x: 160 bytes under 64 KiB, two workgroups a CU");

struct CrossParams {
  const MeasureJob *jobs;
  unsigned long long *partials;  // [pair][pairing][tiles][kTEntries]
  int cw, ch, tiles_x;           // the chroma plane
  int W, H, xdec, ydec, shift;   // the luma plane, chroma decimation, B - 5
  uint32_t tiles;                // of the chroma plane
};

template <int BPS>
__global__ __launch_bounds__(kThreads) void km_measure_x(CrossParams p) {
  __shared__ int16_t s_d[kTH * kTW];
  __shared__ int16_t s_r[kPH * kPW];
  __shared__ int16_t s_l[kPH * kPW];
  __shared__ uint8_t s_bin[kTH * kTW];
  __shared__ unsigned long long s_acc[kWaves][kTEntries];  // (two's complement, as km_measure's)
  static_assert(sizeof(s_d) + sizeof(s_r) + sizeof(s_l) + sizeof(s_bin) + sizeof(s_acc) == kXLdsBytes, "the LDS budget above");
  const MeasureJob &job = p.jobs[blockIdx.z];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
  const int x0 = tx * kTW, y0 = ty * kTH;
  const uint8_t *ya = job.a[0], *yb = job.b[0];
  const uint32_t sya = job.a_stride[0], syb = job.b_stride[0];

  for (int i = tid; i < kWaves * kTEntries; i += kThreads) (&s_acc[0][0])[i] = 0;
  // d_Cr and L of the tile with their halo; for the tile's own samples d_Cb and the bin beside them
  const int round = (1 << (p.xdec + p.ydec)) >> 1;
  for (int i = tid; i < kPH * kPW; i += kThreads) {
    const int ly = i / kPW, lx = i - ly * kPW;
    const int x = x0 + lx - kTHalo, y = y0 + ly - kTHalo;
    const bool inside = x >= 0 && x < p.cw && y >= 0 && y < p.ch;
    const bool own = lx >= kTHalo && lx < kTHalo + kTW && ly >= kTHalo && ly < kTHalo + kTH;
    int d = 0, e = 0, L = 0, bin = kNoBin;
    if (inside) {
      e = sample<BPS>(job.a[2], job.a_stride[2], x, y) - sample<BPS>(job.b[2], job.b_stride[2], x, y);
      // rule 12: the box of the luma residual under the sample, clamped at the luma plane's edges, rounded towards minus infinity
      const int xs = x << p.xdec, ys = y << p.ydec;
      const int xs1 = min(xs + p.xdec, p.W - 1), ys1 = min(ys + p.ydec, p.H - 1);
      const int b00 = sample<BPS>(yb, syb, xs, ys);
      int S = sample<BPS>(ya, sya, xs, ys) - b00, b01 = b00;
      if (p.xdec) {
        b01 = sample<BPS>(yb, syb, xs1, ys);
        S += sample<BPS>(ya, sya, xs1, ys) - b01;
        if (p.ydec) S += sample<BPS>(ya, sya, xs, ys1) - sample<BPS>(yb, syb, xs, ys1) + sample<BPS>(ya, sya, xs1, ys1) - sample<BPS>(yb, syb, xs1, ys1);
      }
      L = (S + round) >> (p.xdec + p.ydec);
      if (own) {
        d = sample<BPS>(job.a[1], job.a_stride[1], x, y) - sample<BPS>(job.b[1], job.b_stride[1], x, y);
        const int I = p.xdec ? (b00 + b01 + 1) >> 1 : b00;  // averageLuma of the clean frame
        bin = min(I >> p.shift, kBins - 1);
      }
    }
    s_r[i] = (int16_t)e;
    s_l[i] = (int16_t)L;
    if (own) {
      const int at = (ly - kTHalo) * kTW + (lx - kTHalo);
      s_d[at] = (int16_t)d;
      s_bin[at] = (uint8_t)bin;
    }
  }
  __syncthreads();

  const int row0 = wave * kRowsPerWave, rows = min(kRowsPerWave, p.ch - (y0 + row0));
  // the pairing's partial record out, the accumulators zero again (an entry is read and cleared by one thread)
  auto hand_over = [&](int j) __attribute__((always_inline)) {
    __syncthreads();
    if (tid < kTEntries) {
      unsigned long long t = 0;
#pragma unroll
      for (int v = 0; v < kWaves; ++v) t += s_acc[v][tid], s_acc[v][tid] = 0;
      const size_t at = ((size_t)blockIdx.z * 3 + (size_t)j) * p.tiles + blockIdx.x;
      p.partials[at * kTEntries + tid] = t;
    }
    __syncthreads();
  };
  // the pairings (d_Cb, L), (d_Cr, L), (d_Cb, d_Cr): the second's own sample comes from the plane with the halo
  if (rows > 0) lag_pass<false>(s_d, s_l, s_bin, s_acc[wave], row0, rows, lane);
  hand_over(0);
  if (rows > 0) lag_pass<true>(s_r, s_l, s_bin, s_acc[wave], row0, rows, lane);
  hand_over(1);
  if (rows > 0) lag_pass<false>(s_d, s_r, s_bin, s_acc[wave], row0, rows, lane);
  hand_over(2);
}

// ---- the scale record (rules 18 - 23): the residual summed over aligned 2^k x 2^k boxes, k = 1 .. 5, binned by the box ----
//   km_measure_s<BPS>  a workgroup per (strip of kSTiles tiles of km_measure side by side: 512 x 128 samples, plane of the class,
//                      pair).  Boxes are aligned at the origin and 32 divides the tile's sides: no box crosses a tile, there is
//                      no halo, and no sample goes through LDS.  A wave takes a band of 32 rows of the strip and walks it tile
//                      by tile, 64 x 8 samples a step: a lane (lx = lane & 7, ly = lane >> 3) loads the 8 consecutive samples
//                      x = 8 lx .. 8 lx + 7 of row ly of a and of b -- one 16-byte (8-byte at 8 bits) load where the address
//                      allows it, sample by sample where it does not or where the plane ends inside -- and for chroma the
//                      clean luma it is binned by.  It forms d and I and their sums of widths 2, 4 and 8 itself.  Rows are
//                      combined between lanes: ly ^ 1 by DPP row_ror:8, ly ^ 2 by a swizzle of the 32-lane halves, ly ^ 4 by a
//                      permute; that gives the boxes of k = 1, 2, 3 of the step in every lane that took part.  k = 4 adds two
//                      steps in a register and lx ^ 1 by DPP, k = 5 four steps and lx ^ 2.  Every sample comes from HBM once.
//   km_tail_s          a workgroup per (plane, pair) sums the strips' partial records into the pair's record.
// Bin sums: a box's (scale, bin) is its key; the lanes that own a box hand it on together, as hand_on does in km_measure: for
// every distinct key among them one masked DPP reduction and one LDS update by lane 0 (the count is the mask's population).
// A step has three such rounds: two for k = 1 (its 128 boxes spread over all 64 lanes: even rows take the left two boxes of
// their lane's four, odd rows the right two) and one for k = 2 .. 5 together, whose owners are distinct lanes (k = 2:
// ly & 3 < 2, k = 3: ly = 2, k = 4: ly = 3 and even lx, k = 5: ly = 6 and lx & 3 = 0; every lane of a group holds the group's
// sums after the exchanges).  A tile has N / 3 boxes in all; a flat tile costs 2 + 2 .. 4 hand-ons a step.
// Exactness: |d| <= 4095, I <= 4095.  A lane's sums over 8 samples are below 2^15; every box sum B and C is below 4^5 2^12 =
// 2^22 and lives in 32 bits; s1 across a wave is below 2^28 (wave_sum); B^2 < 2^44 is formed in 64 bits and summed across
// the wave as two 16-bit pieces and the rest (wave_sum_u64, lane values below 2^57); the LDS and the partial sums are 64-bit.
// The partial records: 480 words a strip and plane.  A strip is 8 tiles wide, so a 4K 4:2:0 pair has 136 + 2 x 36 = 208 of them,
// 0.8 MB, where km_measure's tile would make 6 MB.
constexpr int kScales = 5;
constexpr int kSEntries = kScales * 3 * kBins;  // a partial scale record: [k - 1][n, s1, s2][bin]
constexpr int kSTiles = 8, kSW = kTW * kSTiles;  // the strip of a workgroup
static_assert(kRowsPerWave == 32 && kTW == 64, "a wave's band holds whole 32 x 32 boxes, a step is 8 lanes of 8 samples wide");
static_assert(kSEntries <= kTailThreads, "km_tail_s gives an entry a thread");
static_assert(sizeof(g1s_measure_srecord_t) == 8 * 3 * kSEntries, "km_tail_s writes the scale record as 64-bit words");

// ClassParams for km_measure_s, which also needs the luma height (its own struct: the field stands beside the width)
struct ScaleParams {
  const MeasureJob *jobs;
  unsigned long long *partials;  // [pair][units_frame][kSEntries]
  int pw, ph, units_x;           // the class's plane size, the strips across it
  int plane0;
  int W, H, xdec, ydec, shift;  // luma size, chroma decimation, B - 5
  uint32_t units_frame, unit_base, units_plane;
};

// the value of lane ^ M, every lane taking part
template <int M>
__device__ __forceinline__ int lane_xor(int v, int lane) {
  if (M == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
  if (M == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
  if (M == 8) return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);  // row_ror:8
  if (M == 16) return __builtin_amdgcn_ds_swizzle(v, 0x401F);                    // bit mode: and 0x1f, or 0, xor 0x10
  return __builtin_amdgcn_ds_bpermute((lane ^ M) << 2, v);
}

// samples x .. x + 7 of row y of a pw x ph plane; zeros outside it
template <int BPS>
__device__ __forceinline__ void load8(const uint8_t *plane, uint32_t stride, int x, int y, int pw, int ph, int v[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0;
  if (x >= pw || y >= ph) return;
  const uint8_t *at = plane + (size_t)y * stride + (size_t)x * BPS;
  if (x + 8 <= pw && ((uintptr_t)at & (8 * BPS - 1)) == 0) {
    if (BPS == 2) {
      const uint4 q = *reinterpret_cast<const uint4 *>(at);
      v[0] = (int)(q.x & 0xffffu), v[1] = (int)(q.x >> 16), v[2] = (int)(q.y & 0xffffu), v[3] = (int)(q.y >> 16);
      v[4] = (int)(q.z & 0xffffu), v[5] = (int)(q.z >> 16), v[6] = (int)(q.w & 0xffffu), v[7] = (int)(q.w >> 16);
    } else {
      const uint2 q = *reinterpret_cast<const uint2 *>(at);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (int)((q.x >> (8 * j)) & 0xffu), v[4 + j] = (int)((q.y >> (8 * j)) & 0xffu);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (x + j < pw) v[j] = BPS == 2 ? (int)reinterpret_cast<const uint16_t *>(at)[j] : (int)at[j];
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void km_measure_s(ScaleParams p) {
  __shared__ unsigned long long s_acc[kWaves][kSEntries];  // (two's complement, as km_measure's)
  const MeasureJob &job = p.jobs[blockIdx.z];
  const int c = p.plane0 + (int)blockIdx.y;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = (int)blockIdx.x / p.units_x, tx = (int)blockIdx.x - ty * p.units_x;
  const int x0 = tx * kSW, yw = ty * kTH + wave * kRowsPerWave;  // the wave's band of the strip
  const uint8_t *pa = job.a[c], *pb = job.b[c], *py = job.b[0];
  const uint32_t sa = job.a_stride[c], sb = job.b_stride[c], sy = job.b_stride[0];
  const int lx = lane & 7, ly = lane >> 3;
  unsigned long long *mine = s_acc[wave];

  for (int i = tid; i < kWaves * kSEntries; i += kThreads) (&s_acc[0][0])[i] = 0;
  __syncthreads();

  // hands on the boxes of the lanes with `go` set: key = (k - 1) 32 + K, a reduction and an update a distinct key
  auto hand_on = [&](bool go, int key, int B) __attribute__((always_inline)) {
    unsigned long long todo = __builtin_amdgcn_ballot_w64(go);
    while (todo) {
      const int k = __builtin_amdgcn_readlane(key, (int)__builtin_ctzll(todo));
      const bool m = go && key == k;
      const unsigned long long who = __builtin_amdgcn_ballot_w64(m);
      todo &= ~who;
      const int s1 = wave_sum(m ? B : 0);
      const unsigned long long s2 = wave_sum_u64(m ? (unsigned long long)((long long)B * (long long)B) : 0ull);
      if (lane == 0) {
        unsigned long long *at = mine + (k >> 5) * 3 * kBins + (k & (kBins - 1));
        at[0] += (unsigned long long)__builtin_popcountll(who);
        at[kBins] += (unsigned long long)(long long)s1;
        at[2 * kBins] += s2;
      }
    }
  };
  // the key of a box of scale k with intensity sum C
  auto key_of = [&](int k, int C) { return (k - 1) * kBins + min(C >> (2 * k + p.shift), kBins - 1); };

  if (yw < p.ph) {  // (uniform in the wave)
    for (int sub = 0; sub < kSTiles; ++sub) {
      const int xt = x0 + sub * kTW;
      if (xt >= p.pw) break;  // (uniform)
      const int x = xt + 8 * lx;
      int b4 = 0, c4 = 0, b5 = 0, c5 = 0;  // the sums of k = 4 over two steps and of k = 5 over four
      for (int step = 0; step < 4; ++step) {
        const int y = yw + 8 * step + ly;
        int d[8], I[8];
        load8<BPS>(pa, sa, x, y, p.pw, p.ph, d);
        load8<BPS>(pb, sb, x, y, p.pw, p.ph, I);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] -= I[j];
        if (c) {  // averageLuma of the clean frame, sample by sample (rule 2)
          const int ys = y << p.ydec;
          if (y >= p.ph) {
#pragma unroll
            for (int j = 0; j < 8; ++j) I[j] = 0;
          } else if (!p.xdec) {
            load8<BPS>(py, sy, x, ys, p.W, p.H, I);
          } else {
            int l[16];
            load8<BPS>(py, sy, 2 * x, ys, p.W, p.H, l);
            load8<BPS>(py, sy, 2 * x + 8, ys, p.W, p.H, l + 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) I[j] = (l[2 * j] + (2 * (x + j) + 1 < p.W ? l[2 * j + 1] : l[2 * j]) + 1) >> 1;
          }
        }
        // the lane's own sums of widths 2, 4 and 8
        int B1[4], C1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) B1[j] = d[2 * j] + d[2 * j + 1], C1[j] = I[2 * j] + I[2 * j + 1];
        // k = 1: rows ly and ly ^ 1
#pragma unroll
        for (int j = 0; j < 4; ++j) B1[j] += lane_xor<8>(B1[j], lane), C1[j] += lane_xor<8>(C1[j], lane);
        // k = 2: four columns, rows ly & ~3 .. + 3
        int B2[2], C2[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          B2[j] = B1[2 * j] + B1[2 * j + 1], C2[j] = C1[2 * j] + C1[2 * j + 1];
          B2[j] += lane_xor<16>(B2[j], lane), C2[j] += lane_xor<16>(C2[j], lane);
        }
        // k = 3: the lane's eight columns, the step's eight rows
        int B3 = B2[0] + B2[1], C3 = C2[0] + C2[1];
        B3 += lane_xor<32>(B3, lane), C3 += lane_xor<32>(C3, lane);
        b4 += B3, c4 += C3;
        // (a choice between two registers by a mask: written as a choice between two elements it becomes an indexed array)
        auto pick = [](int mask, int a, int b) { return a ^ ((a ^ b) & mask); };
        const int y2 = y & ~1, odd = ly & 1;
        // a whole box: its last column and its last row lie inside the plane
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int xb = x + 4 * odd + 2 * q;
          hand_on(xb + 2 <= p.pw && y2 + 2 <= p.ph, key_of(1, pick(-odd, C1[q], C1[2 + q])), pick(-odd, B1[q], B1[2 + q]));
        }
        // k = 2 .. 5 in one round: distinct owners
        bool go = false;
        int key = 0, B = 0;
        const int y4 = y & ~3, y8 = y & ~7;
        if ((ly & 3) < 2) {
          go = x + 4 * (ly & 3) + 4 <= p.pw && y4 + 4 <= p.ph;
          key = key_of(2, pick(-(ly & 1), C2[0], C2[1])), B = pick(-(ly & 1), B2[0], B2[1]);
        } else if (ly == 2) {
          go = x + 8 <= p.pw && y8 + 8 <= p.ph, key = key_of(3, C3), B = B3;
        }
        if (step & 1) {  // (uniform)
          const int B4 = b4 + lane_xor<1>(b4, lane), C4 = c4 + lane_xor<1>(c4, lane);
          b4 = c4 = 0;
          b5 += B4, c5 += C4;
          if (ly == 3 && !(lx & 1)) go = x + 16 <= p.pw && (y8 & ~15) + 16 <= p.ph, key = key_of(4, C4), B = B4;
          if (step == 3) {
            // (b5 holds the 16 columns of lx and lx ^ 1 over the band's 32 rows)
            const int B5 = b5 + lane_xor<2>(b5, lane), C5 = c5 + lane_xor<2>(c5, lane);
            if (ly == 6 && !(lx & 3)) go = x + 32 <= p.pw && yw + 32 <= p.ph, key = key_of(5, C5), B = B5;
          }
        }
        hand_on(go, key, B);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kSEntries; i += kThreads) {
    unsigned long long t = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) t += s_acc[v][i];
    const size_t at = (size_t)blockIdx.z * p.units_frame + p.unit_base + (size_t)blockIdx.y * p.units_plane + blockIdx.x;
    p.partials[at * kSEntries + i] = t;
  }
}

// the pair's scale record from its workgroups' partial records: grid (plane, pair).  (Not an instance of km_tail: an entry
// is (scale, field, bin) here and goes to [field][plane][scale][bin], a strip count needs no groups; one body for both would
// branch on the record it writes.)
__global__ __launch_bounds__(kTailThreads) void km_tail_s(TailParams p) {
  const int c = (int)blockIdx.x, i = (int)threadIdx.x;
  if (i >= kSEntries) return;
  const unsigned long long *src = p.partials + ((size_t)blockIdx.y * p.units_frame + p.unit_base[c]) * kSEntries;
  unsigned long long t = 0;
  for (uint32_t k = 0; k < p.units[c]; ++k) t += src[(size_t)k * kSEntries + i];
  // g1s_measure_srecord_t as 64-bit words: n[3][5][32], s1[3][5][32], s2[3][5][32]; entry i = (scale, field, bin)
  const int scale = i / (3 * kBins), field = (i / kBins) % 3, bin = i % kBins;
  unsigned long long *rec = p.records + (size_t)blockIdx.y * (sizeof(g1s_measure_srecord_t) / 8);
  rec[(field * 3 + c) * kScales * kBins + scale * kBins + bin] = t;
}

}  // namespace

// =============================================================== host engine =====
using namespace g1s_op;

// A RecordLane (meter_op.h) a record kind: plain, temporal, cross, scales.
struct g1s_measure : BatchedOp {
  JobQueue<MeasureJob> pairs;  // the batch being filled: every kind but the temporal one reads it, uploaded once
  // how a frame's planes are cut into the units workgroups take: km_measure's tiles, km_measure_s's strips; pairings:
  // km_measure_x's partial records as km_tail<4> reads them, a pairing where a plane is, the chroma plane's tiles each
  Units tiles, strips, pairings;
  RecordLane<g1s_measure_record_t> plain;      // always on
  RecordLane<g1s_measure_trecord_t> temporal;  // rules 7 - 11: a record a temporal job
  RecordLane<g1s_measure_xrecord_t> cross;     // rules 12 - 17: a record a pair, from the batch's own jobs
  RecordLane<g1s_measure_srecord_t> scales;    // rules 18 - 23: likewise
  // a temporal meter: the run's last pair as the kernels read it (side 0 noisy, side 1 clean; the ring moves on with every
  // pair; the caller's device planes are kept over a hand-over) and the batch's temporal jobs
  MeasureJob prev{};
  FrameBefore<2> before;
  JobQueue<TemporalJob> tpairs;
  // the chroma launches alone, for tools/bench_measure.py --cross (recorded only while timing is on)
  Event ev_c[2], ev_tc[2];
  double ms_chroma = 0, ms_tchroma = 0;

  int set_geometry(const g1s_frame_t &f);
  template <class Params, class Job>
  Params class_params(const Job *d_jobs, unsigned long long *partials, int plane0, int unit_w, const Units &u) const;
  template <class Params, class Job>
  int launch_classes(void (*kernel)(Params), const Job *d_jobs, uint32_t n, unsigned long long *partials, int unit_w, const Units &u, Event *chroma_ev);
  int flush();
  int settle();
};

int g1s_measure::set_geometry(const g1s_frame_t &f) {
  set_frame_geometry(f);
  tiles.cut(geom, kTW, kTH), strips.cut(geom, kSW, kTH);
  for (int j = 0; j < 3; ++j) pairings.n[j] = tiles.n[1];
  pairings.lay();
  G1S_OP_TRY(plain.size_partials((size_t)tiles.frame * kEntries * batch));
  G1S_OP_TRY(temporal.size_partials((size_t)tiles.frame * kTEntries * batch));
  G1S_OP_TRY(cross.size_partials(geom.nplanes == 3 ? (size_t)pairings.frame * kTEntries * batch : 0));
  G1S_OP_TRY(scales.size_partials((size_t)strips.frame * kSEntries * batch));
  before.reset(), before.next_slot = 0;  // (a new geometry ends the run; the rings are made again)
  return G1S_OK;
}

// the parameters (ClassParams<Job>, or ScaleParams) of the launch over the plane class that begins at plane0, in units
// unit_w samples wide
template <class Params, class Job>
Params g1s_measure::class_params(const Job *d_jobs, unsigned long long *partials, int plane0, int unit_w, const Units &u) const {
  Params cp{};
  cp.jobs = d_jobs, cp.partials = partials;
  cp.pw = (int)geom.pw(plane0), cp.ph = (int)geom.ph(plane0), cp.units_x = (cp.pw + unit_w - 1) / unit_w, cp.plane0 = plane0;
  cp.W = geom.W, cp.xdec = geom.subx, cp.ydec = geom.suby, cp.shift = (int)bit_depth - 5;
  if constexpr (std::is_same<Params, ScaleParams>::value) cp.H = geom.H;
  cp.units_frame = u.frame, cp.unit_base = u.base[plane0], cp.units_plane = u.n[plane0];
  return cp;
}

// a kernel over n jobs, a launch a plane class: luma, then both chroma planes.  chroma_ev: the events round the chroma
// launch while timing, or null
template <class Params, class Job>
int g1s_measure::launch_classes(void (*kernel)(Params), const Job *d_jobs, uint32_t n, unsigned long long *partials, int unit_w, const Units &u,
                                Event *chroma_ev) {
  for (int plane0 = 0; plane0 < geom.nplanes; plane0 += plane0 ? 2 : 1) {
    const bool mark = timing && plane0 && chroma_ev;
    if (mark) G1S_OP_TRY(hipEventRecord(chroma_ev[0], stream));
    hipLaunchKernelGGL(kernel, dim3(u.n[plane0], plane0 ? 2u : 1u, n), dim3(kThreads), 0, stream, class_params<Params>(d_jobs, partials, plane0, unit_w, u));
    G1S_OP_TRY(hipGetLastError());
    if (mark) G1S_OP_TRY(hipEventRecord(chroma_ev[1], stream));
  }
  return G1S_OK;
}

// the queued pairs as one batch, kind after kind on the meter's stream: a launch per plane class, the summing launch, the
// records back; then all waited for
int g1s_measure::flush() {
  const uint32_t B = (uint32_t)pairs.jobs.size(), T = (uint32_t)tpairs.jobs.size();
  if (!B) return G1S_OK;
  int set, rc = next_set(&set);
  if (rc) return rc;
  const bool wide = bps == 2;
  const unsigned planes = (unsigned)geom.nplanes;
  G1S_OP_TRY(pairs.upload(set, stream));
  const MeasureJob *d_jobs = pairs.sets.d[set];
  G1S_OP_TRY(plain.begin(B, timing, stream));
  if ((rc = launch_classes(wide ? km_measure<2> : km_measure<1>, d_jobs, B, plain.d_partials, kTW, tiles, ev_c)) != 0) return rc;
  G1S_OP_TRY(plain.sum(km_tail<3>, planes, B, kTailThreads, tiles, stream));
  G1S_OP_TRY(plain.end(B, timing, stream));
  // the batch's temporal jobs behind it: the same launches with km_measure_t and km_tail<4>
  if (T) {
    G1S_OP_TRY(tpairs.upload(set, stream));
    G1S_OP_TRY(temporal.begin(T, timing, stream));
    if ((rc = launch_classes(wide ? km_measure_t<2> : km_measure_t<1>, tpairs.sets.d[set].p, T, temporal.d_partials, kTW, tiles, ev_tc)) != 0) return rc;
    G1S_OP_TRY(temporal.sum(km_tail<4>, planes, T, kTailThreads, tiles, stream));
    G1S_OP_TRY(temporal.end(T, timing, stream));
  }
  // a cross meter: the batch's own jobs once more, one km_measure_x launch and km_tail<4> over its partials, where a pairing
  // stands for a plane (a pair with one plane keeps the zeros of the memset)
  if (cross.on) {
    G1S_OP_TRY(cross.begin(B, timing, stream));
    if (geom.nplanes == 3) {
      CrossParams xp{};
      xp.jobs = d_jobs, xp.partials = cross.d_partials;
      xp.cw = (int)geom.pw(1), xp.ch = (int)geom.ph(1), xp.tiles_x = (xp.cw + kTW - 1) / kTW;
      xp.W = geom.W, xp.H = (int)geom.ph(0), xp.xdec = geom.subx, xp.ydec = geom.suby, xp.shift = (int)bit_depth - 5;
      xp.tiles = tiles.n[1];
      void (*const kernel)(CrossParams) = wide ? km_measure_x<2> : km_measure_x<1>;
      hipLaunchKernelGGL(kernel, dim3(tiles.n[1], 1u, B), dim3(kThreads), 0, stream, xp);
      G1S_OP_TRY(hipGetLastError());
      G1S_OP_TRY(cross.sum(km_tail<4>, 3u, B, kTailThreads, pairings, stream));
    }
    G1S_OP_TRY(cross.end(B, timing, stream));
  }
  // a scales meter: the batch's own jobs once more, a km_measure_s launch a plane class and km_tail_s over the strips' partials
  if (scales.on) {
    G1S_OP_TRY(scales.begin(B, timing, stream));
    if ((rc = launch_classes(wide ? km_measure_s<2> : km_measure_s<1>, d_jobs, B, scales.d_partials, kSW, strips, nullptr)) != 0) return rc;
    G1S_OP_TRY(scales.sum(km_tail_s, planes, B, kTailThreads, strips, stream));
    G1S_OP_TRY(scales.end(B, timing, stream));
  }
  if ((rc = set_done(set)) != 0 || (rc = wait()) != 0) return rc;
  if (timing) {  // (every time is read before a record is appended: a failure here leaves the records as they were)
    G1S_OP_TRY(plain.clock(B));
    if (T) G1S_OP_TRY(temporal.clock(T));
    if (cross.on) G1S_OP_TRY(cross.clock(B));
    if (scales.on) G1S_OP_TRY(scales.clock(B));
    if (geom.nplanes == 3) {
      float ms = 0;
      G1S_OP_TRY(hipEventElapsedTime(&ms, ev_c[0], ev_c[1]));
      ms_chroma += ms;
      if (T) {
        G1S_OP_TRY(hipEventElapsedTime(&ms, ev_tc[0], ev_tc[1]));
        ms_tchroma += ms;
      }
    }
  }
  plain.collect(B);
  if (T) temporal.collect(T);
  if (cross.on) cross.collect(B);
  if (scales.on) scales.collect(B);
  pairs.jobs.clear();
  tpairs.jobs.clear();
  return G1S_OK;
}

// A hand-over: what is queued goes out, and the run's last pair survives it -- the planes of it that are the caller's are
// copied into frames of the meter's own and read from there by the next pair's temporal job.  (After flush(): nothing is in
// flight.)
int g1s_measure::settle() {
  int rc = flush();
  if (rc || !before.have) return rc;
  if (before.room(0, stage) != hipSuccess || before.room(1, stage) != hipSuccess) return fail(G1S_ERR_HIP, "hipMalloc of the kept frame failed");
  G1S_OP_TRY(before.keep(0, geom, stage, prev.a, prev.a_stride, stream));
  G1S_OP_TRY(before.keep(1, geom, stage, prev.b, prev.b_stride, stream));
  return wait();
}

namespace {

// what a meter without the kind says to the kind's calls
const char kNotTemporal[] = "the meter was not made by g1s_measure_new_temporal",
           kNotCross[] = "the meter was not made by g1s_measure_new_modes with G1S_MEASURE_CROSS",
           kNotScales[] = "the meter was not made by g1s_measure_new_scales";

// the four *_timing calls: the time in a kind's launches in the timed batches, the records those made
template <class Rec>
int kind_timing(g1s_measure_t *m, RecordLane<Rec> g1s_measure::*lane, double *ms, uint64_t *n) {
  if (!m) return G1S_ERR_INVALID;
  if (ms) *ms = (m->*lane).ms[0];
  if (n) *n = (m->*lane).timed;
  return G1S_OK;
}

// g1s_measure_new, g1s_measure_new_temporal, g1s_measure_new_modes and g1s_measure_new_scales: the same refusals, the same
// meter but for the lanes that are on
g1s_measure_t *measure_new(uint32_t bit_depth, const g1s_measure_opts_t *opts, uint32_t modes, bool scales = false) {
  if (modes & ~(uint32_t)(G1S_MEASURE_TEMPORAL | G1S_MEASURE_CROSS))
    return refuse_new("unknown mode bits: g1s_measure_new_modes takes G1S_MEASURE_TEMPORAL and G1S_MEASURE_CROSS");
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return refuse_new("measure is defined for bit depths 8, 10 and 12");
  return new_op<g1s_measure>("measure", opts, "g1s_measure_opts_t", bit_depth, [&](g1s_measure &m, std::string &) {
    m.plain.on = true, m.temporal.on = (modes & G1S_MEASURE_TEMPORAL) != 0, m.cross.on = (modes & G1S_MEASURE_CROSS) != 0, m.scales.on = scales;
    const uint32_t B = m.batch;
    bool ok = true;
    for (Event &e : m.ev_c) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    ok = ok && m.pairs.alloc(B) && m.plain.alloc(B) && m.temporal.alloc(B) && m.cross.alloc(B) && m.scales.alloc(B);
    if (m.temporal.on) {
      for (Event &e : m.ev_tc) ok = ok && hipEventCreate(&e.p) == hipSuccess;
      ok = ok && m.tpairs.alloc(B);
    }
    return ok;
  });
}

}  // namespace

extern "C" {

g1s_measure_t *g1s_measure_new(uint32_t bit_depth, const g1s_measure_opts_t *opts) { return measure_new(bit_depth, opts, 0); }

g1s_measure_t *g1s_measure_new_temporal(uint32_t bit_depth, const g1s_measure_opts_t *opts) { return measure_new(bit_depth, opts, G1S_MEASURE_TEMPORAL); }

g1s_measure_t *g1s_measure_new_modes(uint32_t bit_depth, const g1s_measure_opts_t *opts, uint32_t modes) { return measure_new(bit_depth, opts, modes); }

g1s_measure_t *g1s_measure_new_scales(uint32_t bit_depth, const g1s_measure_opts_t *opts, uint32_t modes) { return measure_new(bit_depth, opts, modes, true); }

int g1s_measure_frame(g1s_measure_t *m, const g1s_frame_t *noisy, const g1s_frame_t *clean) {
  if (!m || !noisy || !clean) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  (void)hipSetDevice(m->device);
  const Refusal no = check_frame_pair(*noisy, *clean, m->bps, 65536u, "g1s_measure_new",
                                      "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)", "noisy and clean");
  if (no.code) return m->fail(no.code, no.text);
  if (m->scales.on && !scales_size_ok(m->bit_depth, noisy->width, noisy->height)) return m->fail(G1S_ERR_INVALID, scales_refusal_text());
  int rc = take_shape(*m, *noisy);
  if (rc) return rc;
  MeasureJob job{};
  // a plain meter: the batch's slots; a temporal meter: rings of batch + 1 slots, so that the pair before the batch's first
  // pair is still there
  const bool temporal = m->temporal.on;
  const uint32_t slots = temporal ? m->before.slots(m->batch) : m->batch, slot = temporal ? m->before.next_slot : (uint32_t)m->pairs.jobs.size();
  if ((rc = m->stage_in(*noisy, slot, slots, job.a, job.a_stride, 0)) != 0) return rc;
  if ((rc = m->stage_in(*clean, slot, slots, job.b, job.b_stride, 1)) != 0) return rc;
  if ((rc = m->wait_host_input(noisy->on_device == 0 ? *noisy : *clean)) != 0) return rc;
  m->pairs.jobs.push_back(job);
  if (temporal) {
    if (m->before.have) m->tpairs.jobs.push_back(TemporalJob{job, m->prev});
    m->prev = job, m->before.have = true, m->before.advance(m->batch);
    m->before.callers[0] = noisy->on_device == 1, m->before.callers[1] = clean->on_device == 1;
  }
  return m->pairs.jobs.size() >= m->batch ? m->flush() : G1S_OK;
}

int g1s_measure_cut(g1s_measure_t *m) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  if (!m->temporal.on) return not_made(m, kNotTemporal);
  (void)hipSetDevice(m->device);
  m->before.have = false;
  return m->flush();
}

int g1s_measure_finish(g1s_measure_t *m, g1s_measure_record_t *per_frame, size_t cap, size_t *n_out) {
  return finish_kind(m, &g1s_measure::plain, kAlwaysMade, per_frame, cap, n_out);
}

int g1s_measure_finish_temporal(g1s_measure_t *m, g1s_measure_trecord_t *per_pair, size_t cap, size_t *n_out) {
  return finish_kind(m, &g1s_measure::temporal, kNotTemporal, per_pair, cap, n_out);
}

int g1s_measure_finish_cross(g1s_measure_t *m, g1s_measure_xrecord_t *per_pair, size_t cap, size_t *n_out) {
  return finish_kind(m, &g1s_measure::cross, kNotCross, per_pair, cap, n_out);
}

int g1s_measure_finish_scales(g1s_measure_t *m, g1s_measure_srecord_t *per_pair, size_t cap, size_t *n_out) {
  return finish_kind(m, &g1s_measure::scales, kNotScales, per_pair, cap, n_out);
}

int g1s_measure_set_timing(g1s_measure_t *m, int enable, double *ms_kernel, uint64_t *frames) {
  if (m) m->timing = enable != 0;
  return kind_timing(m, &g1s_measure::plain, ms_kernel, frames);
}

int g1s_measure_temporal_timing(g1s_measure_t *m, double *ms_kernel, uint64_t *pairs) { return kind_timing(m, &g1s_measure::temporal, ms_kernel, pairs); }

int g1s_measure_cross_timing(g1s_measure_t *m, double *ms_kernel, uint64_t *pairs) { return kind_timing(m, &g1s_measure::cross, ms_kernel, pairs); }

int g1s_measure_scales_timing(g1s_measure_t *m, double *ms_kernel, uint64_t *pairs) { return kind_timing(m, &g1s_measure::scales, ms_kernel, pairs); }

int g1s_measure_chroma_timing(g1s_measure_t *m, double *ms_chroma, double *ms_temporal_chroma) {
  if (!m) return G1S_ERR_INVALID;
  if (ms_chroma) *ms_chroma = m->ms_chroma;
  if (ms_temporal_chroma) *ms_temporal_chroma = m->ms_tchroma;
  return G1S_OK;
}

const char *g1s_measure_last_error(const g1s_measure_t *m) { return m ? m->err.c_str() : ""; }

void g1s_measure_free(g1s_measure_t *m) { free_op(m); }

// (measure_file.cpp) the device the file commands put their own buffers and the synthesizer on
int32_t g1s_measure_device_(const g1s_measure_t *m) { return m->device; }

}  // extern "C"
