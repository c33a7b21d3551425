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
// A temporal meter (rules 7 - 11) runs km_measure_t and km_tail_t behind them: they stand below km_tail with their own notes.
// A cross meter (rules 12 - 17) runs km_measure_x and km_tail_t behind those: below km_tail_t.
// A scales meter (rules 18 - 23) runs km_measure_s and km_tail_s behind those: below km_measure_x, with their own notes.
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
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "fold.h"
#include "frame_op.h"
#include "wave_sum.hip.h"

namespace {

constexpr int kTW = 64, kTH = 128, kHalo = 3;
constexpr int kLW = kTW + 2 * kHalo, kLH = kTH + kHalo;  // the LDS tile: halo left, right and above
constexpr int kWaves = 4, kThreads = 64 * kWaves, kRowsPerWave = kTH / kWaves;
constexpr int kBins = 32, kLags = 25;
constexpr int kEntries = 3 * kBins + kLags;  // a partial record: n[32], s1[32], s2[32], r[25]
constexpr int kNoBin = 0xff;
constexpr int kTailGroups = 4;
static_assert(kRowsPerWave <= 127, "a 32-bit lag sum holds 127 products of 12-bit residuals");

struct MeasureJob {
  const uint8_t *a[3], *b[3];
  uint32_t a_stride[3], b_stride[3];  // bytes
};

struct MeasureParams {
  const MeasureJob *jobs;
  unsigned long long *partials;  // [pair][tiles_frame][kEntries]
  int pw, ph, tiles_x;           // the class's plane size
  int plane0;                    // first plane of the class: 0 luma, 1 chroma
  int W, xdec, ydec, shift;      // luma width, chroma decimation, B - 5
  uint32_t tiles_frame, tile_base, tiles_plane;
};

struct TailParams {
  const unsigned long long *partials;
  unsigned long long *records;  // [pair] g1s_measure_record_t
  uint32_t tiles_frame, tiles[3], tile_base[3];
};

template <int BPS>
__device__ __forceinline__ int sample(const uint8_t *plane, uint32_t stride, int x, int y) {
  const uint8_t *row = plane + (size_t)y * stride;
  return BPS == 2 ? (int)reinterpret_cast<const uint16_t *>(row)[x] : (int)row[x];
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void km_measure(MeasureParams p) {
  __shared__ int16_t s_d[kLH * kLW];
  __shared__ uint8_t s_bin[kTH * kTW];
  __shared__ unsigned long long s_acc[kWaves][kEntries];  // (two's complement: the signed sums are added as unsigned)
  const MeasureJob &job = p.jobs[blockIdx.z];
  const int c = p.plane0 + (int)blockIdx.y;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
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
      if (own) {
        int I = b;
        if (c) {  // averageLuma of the clean frame
          const int xs = x << p.xdec, ys = y << p.ydec;
          I = sample<BPS>(py, sy, xs, ys);
          if (p.xdec) I = (I + sample<BPS>(py, sy, min(xs + 1, p.W - 1), ys) + 1) >> 1;
        }
        bin = min(I >> p.shift, kBins - 1);  // (a sample above the depth's maximum: the caller's error, not a wild index)
      }
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
    const size_t at = (size_t)blockIdx.z * p.tiles_frame + p.tile_base + (size_t)blockIdx.y * p.tiles_plane + blockIdx.x;
    p.partials[at * kEntries + tid] = t;
  }
}

// the pair's record from its workgroups' partial records: grid (plane, pair)
__global__ __launch_bounds__(128 * kTailGroups) void km_tail(TailParams p) {
  __shared__ unsigned long long s_sum[kTailGroups][128];
  const int c = (int)blockIdx.x, i = (int)threadIdx.x & 127, g = (int)threadIdx.x >> 7;
  const unsigned long long *src = p.partials + ((size_t)blockIdx.y * p.tiles_frame + p.tile_base[c]) * kEntries;
  unsigned long long t = 0;
  if (i < kEntries)
    for (uint32_t k = (uint32_t)g; k < p.tiles[c]; k += kTailGroups) t += src[(size_t)k * kEntries + i];
  s_sum[g][i] = t;
  __syncthreads();
  if (g == 0 && i < kEntries) {
    for (int v = 1; v < kTailGroups; ++v) t += s_sum[v][i];
    // g1s_measure_record_t as 64-bit words: n[3][32], s1[3][32], s2[3][32], r[3][25]
    unsigned long long *rec = p.records + (size_t)blockIdx.y * (sizeof(g1s_measure_record_t) / 8);
    const int field = i < 3 * kBins ? i / kBins : 3, k = i - field * kBins;
    rec[field < 3 ? field * 3 * kBins + c * kBins + k : 9 * kBins + c * kLags + k] = t;
  }
}

// ---- the temporal record (rules 7 - 11): the residual of pair t against the residual of pair t - 1 ----
//   km_measure_t<BPS>  a workgroup per (tile, plane of the class, temporal job), km_measure's tile, waves and plane classes.
//                      LDS: d_t of the tile as int16 without a halo; d_{t-1} as int16 with a halo of 2 on all four sides
//                      (zeros outside the plane: a skipped product is a product with 0); the tile's bins as bytes, from
//                      pair t's clean frame; the waves' accumulators.  A wave walks its 32 rows, a lane a column, with the
//                      5 x 5 window of d_{t-1} in registers: 5 LDS reads of d_{t-1} and 25 multiply-adds a sample.
//   km_tail_t          km_tail for the partial records of km_measure_t.
// The 32-bit sums follow km_measure's schedule: a lane's 25 lag sums and its bin sums (n, x, u, v) take one product a row
// for the wave's 32 rows at the most (below 2^29 in size) and go on in 64 bits through wave_sum_wide, which carries the
// signed x and c as it carries km_measure's lag sums.
constexpr int kTHalo = 2, kTWin = 2 * kTHalo + 1;
constexpr int kPW = kTW + 2 * kTHalo, kPH = kTH + 2 * kTHalo;  // the LDS tile of d_{t-1}
constexpr int kTLags = kTWin * kTWin;
constexpr int kTEntries = 4 * kBins + kTLags;  // a partial temporal record: n[32], x[32], u[32], v[32], c[25]
constexpr int kTTailWidth = 256, kTTailGroups = 2;
static_assert(kRowsPerWave <= 127, "a 32-bit sum of km_measure_t holds 127 products of 12-bit residuals, one a row");
static_assert(kTLags == 25 && kTEntries <= kTTailWidth, "g1s_measure_trecord_t has 25 offsets; km_tail_t gives an entry a thread");
static_assert(sizeof(g1s_measure_trecord_t) == 8 * 3 * kTEntries, "km_tail_t writes the record as 64-bit words");

struct TemporalJob {
  MeasureJob cur, prev;  // pair t and pair t - 1 of the run
};

struct TemporalParams {
  const TemporalJob *jobs;
  unsigned long long *partials;  // [job][tiles_frame][kTEntries]
  int pw, ph, tiles_x;
  int plane0;
  int W, xdec, ydec, shift;
  uint32_t tiles_frame, tile_base, tiles_plane;
};

template <int BPS>
__global__ __launch_bounds__(kThreads) void km_measure_t(TemporalParams p) {
  __shared__ int16_t s_d[kTH * kTW];
  __shared__ int16_t s_p[kPH * kPW];
  __shared__ uint8_t s_bin[kTH * kTW];
  __shared__ unsigned long long s_acc[kWaves][kTEntries];  // (two's complement, as km_measure's)
  const TemporalJob &job = p.jobs[blockIdx.z];
  const int c = p.plane0 + (int)blockIdx.y;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
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
        int I = b;
        if (c) {  // averageLuma of pair t's clean frame
          const int xs = x << p.xdec, ys = y << p.ydec;
          I = sample<BPS>(py, sy, xs, ys);
          if (p.xdec) I = (I + sample<BPS>(py, sy, min(xs + 1, p.W - 1), ys) + 1) >> 1;
        }
        bin = min(I >> p.shift, kBins - 1);
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
    const size_t at = (size_t)blockIdx.z * p.tiles_frame + p.tile_base + (size_t)blockIdx.y * p.tiles_plane + blockIdx.x;
    p.partials[at * kTEntries + tid] = t;
  }
}

// the job's temporal record from its workgroups' partial records: grid (plane, job)
__global__ __launch_bounds__(kTTailWidth * kTTailGroups) void km_tail_t(TailParams p) {
  __shared__ unsigned long long s_sum[kTTailGroups][kTTailWidth];
  const int c = (int)blockIdx.x, i = (int)threadIdx.x % kTTailWidth, g = (int)threadIdx.x / kTTailWidth;
  const unsigned long long *src = p.partials + ((size_t)blockIdx.y * p.tiles_frame + p.tile_base[c]) * kTEntries;
  unsigned long long t = 0;
  if (i < kTEntries)
    for (uint32_t k = (uint32_t)g; k < p.tiles[c]; k += kTTailGroups) t += src[(size_t)k * kTEntries + i];
  s_sum[g][i] = t;
  __syncthreads();
  if (g == 0 && i < kTEntries) {
    for (int v = 1; v < kTTailGroups; ++v) t += s_sum[v][i];
    // g1s_measure_trecord_t as 64-bit words: n[3][32], x[3][32], u[3][32], v[3][32], c[3][25]
    unsigned long long *rec = p.records + (size_t)blockIdx.y * (sizeof(g1s_measure_trecord_t) / 8);
    const int field = i < 4 * kBins ? i / kBins : 4, k = i - field * kBins;
    rec[field < 4 ? field * 3 * kBins + c * kBins + k : 12 * kBins + c * kTLags + k] = t;
  }
}

// ---- the cross record (rules 12 - 17): the chroma residuals against the luma residual under them, and against each other ----
//   km_measure_x<BPS>  a workgroup per (chroma tile, pair), km_measure_t's tile and waves with other operands.  LDS: d_Cb of
//                      the tile as int16 without a halo; d_Cr and L (rule 12: the rounded mean of the luma residual under a
//                      chroma sample, formed here from the (1 + xdec)(1 + ydec) luma samples of both frames) as int16 with a
//                      halo of 2 on all four sides, zeros outside the chroma plane; the tile's bins as bytes; ONE set of the
//                      waves' accumulators.  Everything is loaded once a tile; the three pairings (d_Cb, L), (d_Cr, L),
//                      (d_Cb, d_Cr) then walk the tile one after another through one set of 25 lag accumulators and one set
//                      of running bin sums (cross_pass<J>), and the workgroup's partial record of a pairing goes out with
//                      plain stores before the next one starts.
//   km_tail_t          sums the partials unchanged: they lie as [pair][pairing][tile][kTEntries], so that a "plane" is a
//                      pairing and all three tile counts are the chroma plane's.
// The 32-bit sums are km_measure_t's: |L| <= 2^B - 1 (a rounded mean of residuals), so every product stays below 2^24.
constexpr int kXLdsBytes = 2 * kTH * kTW + 2 * 2 * kPH * kPW + kTH * kTW + 8 * kWaves * kTEntries;
static_assert(kRowsPerWave <= 127, "a 32-bit sum of km_measure_x holds 127 products of 12-bit residuals, one a row");
static_assert(sizeof(g1s_measure_xrecord_t) == 8 * 3 * kTEntries, "km_tail_t writes the cross record as 64-bit words");
static_assert(kXLdsBytes == 65376 && kXLdsBytes <= 65536, "km_measure_x: 160 bytes under 64 KiB, two workgroups a CU");

struct CrossParams {
  const MeasureJob *jobs;
  unsigned long long *partials;  // [pair][pairing][tiles][kTEntries]
  int cw, ch, tiles_x;           // the chroma plane
  int W, H, xdec, ydec, shift;   // the luma plane, chroma decimation, B - 5
  uint32_t tiles;                // of the chroma plane
};

// one pairing over the wave's rows: J = 0 (d_Cb, L), 1 (d_Cr, L), 2 (d_Cb, d_Cr).  km_measure_t's row loop: a = the tile's
// own sample, b = the 5 x 5 window round it in a plane with a halo.
template <int J>
__device__ __forceinline__ void cross_pass(const int16_t *s_d, const int16_t *s_r, const int16_t *s_l, const uint8_t *s_bin,
                                           unsigned long long *mine, int row0, int rows, int lane) {
  const int16_t *s_b = J == 2 ? s_r : s_l;
  int acc[kTLags];
#pragma unroll
  for (int i = 0; i < kTLags; ++i) acc[i] = 0;
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
    const int d = J == 1 ? (int)s_r[(row0 + r + kTHalo) * kPW + lane + kTHalo] : (int)s_d[(row0 + r) * kTW + lane];
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
  if (rows > 0) cross_pass<0>(s_d, s_r, s_l, s_bin, s_acc[wave], row0, rows, lane);
  hand_over(0);
  if (rows > 0) cross_pass<1>(s_d, s_r, s_l, s_bin, s_acc[wave], row0, rows, lane);
  hand_over(1);
  if (rows > 0) cross_pass<2>(s_d, s_r, s_l, s_bin, s_acc[wave], row0, rows, lane);
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
constexpr int kSTailThreads = 512;
static_assert(kRowsPerWave == 32 && kTW == 64, "a wave's band holds whole 32 x 32 boxes, a step is 8 lanes of 8 samples wide");
static_assert(kSEntries <= kSTailThreads, "km_tail_s gives an entry a thread");
static_assert(sizeof(g1s_measure_srecord_t) == 8 * 3 * kSEntries, "km_tail_s writes the scale record as 64-bit words");

struct ScaleParams {
  const MeasureJob *jobs;
  unsigned long long *partials;  // [pair][strips_frame][kSEntries]
  int pw, ph, strips_x;          // the class's plane size
  int plane0;
  int W, H, xdec, ydec, shift;  // luma size, chroma decimation, B - 5
  uint32_t strips_frame, strip_base, strips_plane;
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
  const int ty = (int)blockIdx.x / p.strips_x, tx = (int)blockIdx.x - ty * p.strips_x;
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
    const size_t at = (size_t)blockIdx.z * p.strips_frame + p.strip_base + (size_t)blockIdx.y * p.strips_plane + blockIdx.x;
    p.partials[at * kSEntries + i] = t;
  }
}

// the pair's scale record from its workgroups' partial records: grid (plane, pair)
__global__ __launch_bounds__(kSTailThreads) void km_tail_s(TailParams p) {
  const int c = (int)blockIdx.x, i = (int)threadIdx.x;
  if (i >= kSEntries) return;
  const unsigned long long *src = p.partials + ((size_t)blockIdx.y * p.tiles_frame + p.tile_base[c]) * kSEntries;
  unsigned long long t = 0;
  for (uint32_t k = 0; k < p.tiles[c]; ++k) t += src[(size_t)k * kSEntries + i];
  // g1s_measure_srecord_t as 64-bit words: n[3][5][32], s1[3][5][32], s2[3][5][32]; entry i = (scale, field, bin)
  const int scale = i / (3 * kBins), field = (i / kBins) % 3, bin = i % kBins;
  unsigned long long *rec = p.records + (size_t)blockIdx.y * (sizeof(g1s_measure_srecord_t) / 8);
  rec[(field * 3 + c) * kScales * kBins + scale * kBins + bin] = t;
}

// rule 8's offsets: raster order, (0, 0) is index 12
void temporal_offset(int i, int *dx, int *dy) { *dy = i / kTWin - kTHalo, *dx = i % kTWin - kTHalo; }

// rule 4's offsets in the table's coefficient order, (0, 0) last
void lag_offset(int i, int *dx, int *dy) {
  if (i == 24) *dx = 0, *dy = 0;
  else *dy = i / 7 - 3, *dx = i % 7 - 3;
}

}  // namespace

// =============================================================== host engine =====
using namespace g1s_op;

struct g1s_measure : BatchedOp {
  Event ev[2];
  std::vector<MeasureJob> jobs;  // the batch being filled
  ParamSets<MeasureJob> p_jobs;
  DevBuf<unsigned long long> d_partials;
  size_t partials_cap = 0;
  uint32_t tiles[3] = {0, 0, 0}, tile_base[3] = {0, 0, 0}, tiles_frame = 0;
  DevBuf<g1s_measure_record_t> d_recs;
  PinnedBuf<g1s_measure_record_t> h_recs;
  std::vector<g1s_measure_record_t> records;  // since the last hand-over
  double ms_kernel = 0;
  uint64_t frames_timed = 0;
  // a temporal meter: the run's last pair as the kernels read it (its planes: the caller's, or a slot of the input rings,
  // which then have batch + 1 slots filled round-robin), the batch's temporal jobs, the temporal records
  bool temporal = false, have_prev = false;
  MeasureJob prev{};
  bool prev_staged[2] = {false, false};  // (are the planes of prev.a / prev.b the meter's own: a ring's or d_keep's?)
  uint32_t ring_at = 0;
  DevBuf<uint8_t> d_keep[2];  // a frame each: the caller's device planes of the run's last pair, kept over a hand-over
  Event ev_t[2];
  std::vector<TemporalJob> tjobs;
  ParamSets<TemporalJob> p_tjobs;
  DevBuf<unsigned long long> d_tpartials;
  size_t tpartials_cap = 0;
  DevBuf<g1s_measure_trecord_t> d_trecs;
  PinnedBuf<g1s_measure_trecord_t> h_trecs;
  std::vector<g1s_measure_trecord_t> trecords;  // since the last hand-over
  double ms_tkernel = 0;
  uint64_t pairs_timed = 0;
  // a cross meter (rules 12 - 17): a cross record a pair, from the batch's own jobs
  bool cross = false;
  Event ev_x[2];
  DevBuf<unsigned long long> d_xpartials;
  size_t xpartials_cap = 0;
  DevBuf<g1s_measure_xrecord_t> d_xrecs;
  PinnedBuf<g1s_measure_xrecord_t> h_xrecs;
  std::vector<g1s_measure_xrecord_t> xrecords;  // since the last hand-over
  double ms_xkernel = 0;
  uint64_t xpairs_timed = 0;
  // a scales meter (rules 18 - 23): a scale record a pair, from the batch's own jobs
  bool scales = false;
  Event ev_s[2];
  DevBuf<unsigned long long> d_spartials;
  size_t spartials_cap = 0;
  uint32_t strips[3] = {0, 0, 0}, strip_base[3] = {0, 0, 0}, strips_frame = 0;
  DevBuf<g1s_measure_srecord_t> d_srecs;
  PinnedBuf<g1s_measure_srecord_t> h_srecs;
  std::vector<g1s_measure_srecord_t> srecords;  // since the last hand-over
  double ms_skernel = 0;
  uint64_t spairs_timed = 0;
  // the chroma launches alone, for tools/bench_measure.py --cross (recorded only while timing is on)
  Event ev_c[2], ev_tc[2];
  double ms_chroma = 0, ms_tchroma = 0;

  int set_geometry(const g1s_frame_t &f);
  int flush();
  int keep_prev();
};

int g1s_measure::set_geometry(const g1s_frame_t &f) {
  set_frame_geometry(f);
  tiles_frame = 0;
  for (int c = 0; c < 3; ++c) {
    tiles[c] = c < geom.nplanes ? (uint32_t)(((geom.pw(c) + kTW - 1) / kTW) * ((geom.ph(c) + kTH - 1) / kTH)) : 0u;
    tile_base[c] = tiles_frame;
    tiles_frame += tiles[c];
  }
  const size_t need = (size_t)tiles_frame * kEntries * batch;
  if (need > partials_cap) {
    d_partials = DevBuf<unsigned long long>();
    G1S_OP_TRY(hipMalloc((void **)&d_partials.p, need * sizeof(unsigned long long)));
    partials_cap = need;
  }
  const size_t tneed = temporal ? (size_t)tiles_frame * kTEntries * batch : 0;
  if (tneed > tpartials_cap) {
    d_tpartials = DevBuf<unsigned long long>();
    G1S_OP_TRY(hipMalloc((void **)&d_tpartials.p, tneed * sizeof(unsigned long long)));
    tpartials_cap = tneed;
  }
  const size_t xneed = cross && geom.nplanes == 3 ? (size_t)tiles[1] * 3 * kTEntries * batch : 0;
  if (xneed > xpartials_cap) {
    d_xpartials = DevBuf<unsigned long long>();
    G1S_OP_TRY(hipMalloc((void **)&d_xpartials.p, xneed * sizeof(unsigned long long)));
    xpartials_cap = xneed;
  }
  strips_frame = 0;
  for (int c = 0; c < 3; ++c) {
    strips[c] = scales && c < geom.nplanes ? (uint32_t)(((geom.pw(c) + kSW - 1) / kSW) * ((geom.ph(c) + kTH - 1) / kTH)) : 0u;
    strip_base[c] = strips_frame;
    strips_frame += strips[c];
  }
  const size_t sneed = (size_t)strips_frame * kSEntries * batch;
  if (sneed > spartials_cap) {
    d_spartials = DevBuf<unsigned long long>();
    G1S_OP_TRY(hipMalloc((void **)&d_spartials.p, sneed * sizeof(unsigned long long)));
    spartials_cap = sneed;
  }
  have_prev = false, ring_at = 0;  // (a new geometry ends the run; the rings are made again)
  d_keep[0] = DevBuf<uint8_t>(), d_keep[1] = DevBuf<uint8_t>();
  return G1S_OK;
}

// the queued pairs as one batch: a launch per plane class, the summing launch, the records back, all waited for
int g1s_measure::flush() {
  const uint32_t B = (uint32_t)jobs.size();
  if (!B) return G1S_OK;
  int set, rc = next_set(&set);
  if (rc) return rc;
  std::memcpy(p_jobs.h[set], jobs.data(), sizeof(MeasureJob) * B);
  G1S_OP_TRY(p_jobs.upload(set, B, stream));
  G1S_OP_TRY(hipMemsetAsync(d_recs, 0, sizeof(g1s_measure_record_t) * B, stream));  // (the planes a frame does not have)
  if (timing) G1S_OP_TRY(hipEventRecord(ev[0], stream));
  for (int plane0 = 0; plane0 < geom.nplanes; plane0 += plane0 ? 2 : 1) {
    MeasureParams mp{};
    mp.jobs = p_jobs.d[set], mp.partials = d_partials;
    mp.pw = (int)geom.pw(plane0), mp.ph = (int)geom.ph(plane0), mp.tiles_x = (mp.pw + kTW - 1) / kTW, mp.plane0 = plane0;
    mp.W = geom.W, mp.xdec = geom.subx, mp.ydec = geom.suby, mp.shift = (int)bit_depth - 5;
    mp.tiles_frame = tiles_frame, mp.tile_base = tile_base[plane0], mp.tiles_plane = tiles[plane0];
    const dim3 grid(tiles[plane0], plane0 ? 2u : 1u, B);
    if (timing && plane0) G1S_OP_TRY(hipEventRecord(ev_c[0], stream));
    if (bps == 2) hipLaunchKernelGGL(km_measure<2>, grid, dim3(kThreads), 0, stream, mp);
    else hipLaunchKernelGGL(km_measure<1>, grid, dim3(kThreads), 0, stream, mp);
    G1S_OP_TRY(hipGetLastError());
    if (timing && plane0) G1S_OP_TRY(hipEventRecord(ev_c[1], stream));
  }
  TailParams tp{};
  tp.partials = d_partials, tp.records = reinterpret_cast<unsigned long long *>(d_recs.p), tp.tiles_frame = tiles_frame;
  for (int c = 0; c < 3; ++c) tp.tiles[c] = tiles[c], tp.tile_base[c] = tile_base[c];
  hipLaunchKernelGGL(km_tail, dim3((unsigned)geom.nplanes, B), dim3(128 * kTailGroups), 0, stream, tp);
  G1S_OP_TRY(hipGetLastError());
  if (timing) G1S_OP_TRY(hipEventRecord(ev[1], stream));
  G1S_OP_TRY(hipMemcpyAsync(h_recs, d_recs, sizeof(g1s_measure_record_t) * B, hipMemcpyDeviceToHost, stream));
  // the batch's temporal jobs behind it on the same stream: the same launches with km_measure_t and km_tail_t
  const uint32_t T = (uint32_t)tjobs.size();
  if (T) {
    std::memcpy(p_tjobs.h[set], tjobs.data(), sizeof(TemporalJob) * T);
    G1S_OP_TRY(p_tjobs.upload(set, T, stream));
    G1S_OP_TRY(hipMemsetAsync(d_trecs, 0, sizeof(g1s_measure_trecord_t) * T, stream));
    if (timing) G1S_OP_TRY(hipEventRecord(ev_t[0], stream));
    for (int plane0 = 0; plane0 < geom.nplanes; plane0 += plane0 ? 2 : 1) {
      TemporalParams mp{};
      mp.jobs = p_tjobs.d[set], mp.partials = d_tpartials;
      mp.pw = (int)geom.pw(plane0), mp.ph = (int)geom.ph(plane0), mp.tiles_x = (mp.pw + kTW - 1) / kTW, mp.plane0 = plane0;
      mp.W = geom.W, mp.xdec = geom.subx, mp.ydec = geom.suby, mp.shift = (int)bit_depth - 5;
      mp.tiles_frame = tiles_frame, mp.tile_base = tile_base[plane0], mp.tiles_plane = tiles[plane0];
      const dim3 grid(tiles[plane0], plane0 ? 2u : 1u, T);
      if (timing && plane0) G1S_OP_TRY(hipEventRecord(ev_tc[0], stream));
      if (bps == 2) hipLaunchKernelGGL(km_measure_t<2>, grid, dim3(kThreads), 0, stream, mp);
      else hipLaunchKernelGGL(km_measure_t<1>, grid, dim3(kThreads), 0, stream, mp);
      G1S_OP_TRY(hipGetLastError());
      if (timing && plane0) G1S_OP_TRY(hipEventRecord(ev_tc[1], stream));
    }
    TailParams ttp = tp;
    ttp.partials = d_tpartials, ttp.records = reinterpret_cast<unsigned long long *>(d_trecs.p);
    hipLaunchKernelGGL(km_tail_t, dim3((unsigned)geom.nplanes, T), dim3(kTTailWidth * kTTailGroups), 0, stream, ttp);
    G1S_OP_TRY(hipGetLastError());
    if (timing) G1S_OP_TRY(hipEventRecord(ev_t[1], stream));
    G1S_OP_TRY(hipMemcpyAsync(h_trecs, d_trecs, sizeof(g1s_measure_trecord_t) * T, hipMemcpyDeviceToHost, stream));
  }
  // a cross meter: the batch's own jobs once more, one km_measure_x launch and km_tail_t over its partials, where a pairing
  // stands for a plane (a pair with one plane keeps the zeros of the memset)
  if (cross) {
    G1S_OP_TRY(hipMemsetAsync(d_xrecs, 0, sizeof(g1s_measure_xrecord_t) * B, stream));
    if (timing) G1S_OP_TRY(hipEventRecord(ev_x[0], stream));
    if (geom.nplanes == 3) {
      CrossParams xp{};
      xp.jobs = p_jobs.d[set], xp.partials = d_xpartials;
      xp.cw = (int)geom.pw(1), xp.ch = (int)geom.ph(1), xp.tiles_x = (xp.cw + kTW - 1) / kTW;
      xp.W = geom.W, xp.H = (int)geom.ph(0), xp.xdec = geom.subx, xp.ydec = geom.suby, xp.shift = (int)bit_depth - 5;
      xp.tiles = tiles[1];
      if (bps == 2) hipLaunchKernelGGL(km_measure_x<2>, dim3(tiles[1], 1u, B), dim3(kThreads), 0, stream, xp);
      else hipLaunchKernelGGL(km_measure_x<1>, dim3(tiles[1], 1u, B), dim3(kThreads), 0, stream, xp);
      G1S_OP_TRY(hipGetLastError());
      TailParams xtp{};
      xtp.partials = d_xpartials, xtp.records = reinterpret_cast<unsigned long long *>(d_xrecs.p), xtp.tiles_frame = 3 * tiles[1];
      for (int j = 0; j < 3; ++j) xtp.tiles[j] = tiles[1], xtp.tile_base[j] = (uint32_t)j * tiles[1];
      hipLaunchKernelGGL(km_tail_t, dim3(3u, B), dim3(kTTailWidth * kTTailGroups), 0, stream, xtp);
      G1S_OP_TRY(hipGetLastError());
    }
    if (timing) G1S_OP_TRY(hipEventRecord(ev_x[1], stream));
    G1S_OP_TRY(hipMemcpyAsync(h_xrecs, d_xrecs, sizeof(g1s_measure_xrecord_t) * B, hipMemcpyDeviceToHost, stream));
  }
  // a scales meter: the batch's own jobs once more, a km_measure_s launch a plane class and km_tail_s over the strips' partials
  if (scales) {
    G1S_OP_TRY(hipMemsetAsync(d_srecs, 0, sizeof(g1s_measure_srecord_t) * B, stream));  // (the planes a frame does not have)
    if (timing) G1S_OP_TRY(hipEventRecord(ev_s[0], stream));
    for (int plane0 = 0; plane0 < geom.nplanes; plane0 += plane0 ? 2 : 1) {
      ScaleParams sp{};
      sp.jobs = p_jobs.d[set], sp.partials = d_spartials;
      sp.pw = (int)geom.pw(plane0), sp.ph = (int)geom.ph(plane0), sp.strips_x = (sp.pw + kSW - 1) / kSW, sp.plane0 = plane0;
      sp.W = geom.W, sp.H = geom.H, sp.xdec = geom.subx, sp.ydec = geom.suby, sp.shift = (int)bit_depth - 5;
      sp.strips_frame = strips_frame, sp.strip_base = strip_base[plane0], sp.strips_plane = strips[plane0];
      const dim3 grid(strips[plane0], plane0 ? 2u : 1u, B);
      if (bps == 2) hipLaunchKernelGGL(km_measure_s<2>, grid, dim3(kThreads), 0, stream, sp);
      else hipLaunchKernelGGL(km_measure_s<1>, grid, dim3(kThreads), 0, stream, sp);
      G1S_OP_TRY(hipGetLastError());
    }
    TailParams stp{};
    stp.partials = d_spartials, stp.records = reinterpret_cast<unsigned long long *>(d_srecs.p), stp.tiles_frame = strips_frame;
    for (int c = 0; c < 3; ++c) stp.tiles[c] = strips[c], stp.tile_base[c] = strip_base[c];
    hipLaunchKernelGGL(km_tail_s, dim3((unsigned)geom.nplanes, B), dim3(kSTailThreads), 0, stream, stp);
    G1S_OP_TRY(hipGetLastError());
    if (timing) G1S_OP_TRY(hipEventRecord(ev_s[1], stream));
    G1S_OP_TRY(hipMemcpyAsync(h_srecs, d_srecs, sizeof(g1s_measure_srecord_t) * B, hipMemcpyDeviceToHost, stream));
  }
  if ((rc = set_done(set)) != 0 || (rc = wait()) != 0) return rc;
  if (timing) {
    float ms = 0;
    G1S_OP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    ms_kernel += ms, frames_timed += B;
    if (T) {
      G1S_OP_TRY(hipEventElapsedTime(&ms, ev_t[0], ev_t[1]));
      ms_tkernel += ms, pairs_timed += T;
      if (geom.nplanes == 3) {
        G1S_OP_TRY(hipEventElapsedTime(&ms, ev_tc[0], ev_tc[1]));
        ms_tchroma += ms;
      }
    }
    if (geom.nplanes == 3) {
      G1S_OP_TRY(hipEventElapsedTime(&ms, ev_c[0], ev_c[1]));
      ms_chroma += ms;
    }
    if (cross) {
      G1S_OP_TRY(hipEventElapsedTime(&ms, ev_x[0], ev_x[1]));
      ms_xkernel += ms, xpairs_timed += B;
    }
    if (scales) {
      G1S_OP_TRY(hipEventElapsedTime(&ms, ev_s[0], ev_s[1]));
      ms_skernel += ms, spairs_timed += B;
    }
  }
  records.insert(records.end(), h_recs.p, h_recs.p + B);
  trecords.insert(trecords.end(), h_trecs.p, h_trecs.p + T);
  if (cross) xrecords.insert(xrecords.end(), h_xrecs.p, h_xrecs.p + B);
  if (scales) srecords.insert(srecords.end(), h_srecs.p, h_srecs.p + B);
  jobs.clear();
  tjobs.clear();
  return G1S_OK;
}

// The run's last pair survives a hand-over: the planes of it that are the caller's are copied into a frame of the meter's
// own, device to device, and read from there by the next pair's temporal job.  (After flush(): nothing is in flight.)
int g1s_measure::keep_prev() {
  if (!have_prev) return G1S_OK;
  for (int side = 0; side < 2; ++side) {
    if (prev_staged[side]) continue;
    const uint8_t **plane = side ? prev.b : prev.a;
    uint32_t *stride = side ? prev.b_stride : prev.a_stride;
    if (!d_keep[side] && hipMalloc((void **)&d_keep[side].p, stage.frame) != hipSuccess)
      return fail(G1S_ERR_HIP, "hipMalloc of the kept frame failed");
    for (int c = 0; c < geom.nplanes; ++c) {
      uint8_t *dst = d_keep[side] + stage.off[c];
      G1S_OP_TRY(hipMemcpy2DAsync(dst, stage.row[c], plane[c], stride[c], geom.row_bytes(c), geom.ph(c), hipMemcpyDeviceToDevice, stream));
      plane[c] = dst, stride[c] = (uint32_t)stage.row[c];
    }
    prev_staged[side] = true;
  }
  return wait();
}

namespace {

bool checked_add(uint64_t &t, uint64_t v) { return !__builtin_add_overflow(t, v, &t); }
bool checked_add(int64_t &t, int64_t v) { return !__builtin_add_overflow(t, v, &t); }

// "%.4f" of v, or "-"
std::string value(bool defined, double v) {
  if (!defined) return "-";
  char s[64];
  snprintf(s, sizeof s, "%.4f", v);
  return s;
}

struct Profile {
  bool has[kBins];
  double mean[kBins], sigma[kBins];
  bool has_rho[24];
  double rho[24];
};

// the printed values of plane c of a clip's record (one division or one square root a step, in this order)
Profile profile_of(const g1s_measure_record_t &t, int c, const double terms[kLags]) {
  Profile p{};
  for (int k = 0; k < kBins; ++k) {
    p.has[k] = t.n[c][k] > 0;
    if (!p.has[k]) continue;
    const double n = (double)t.n[c][k];
    p.mean[k] = (double)t.s1[c][k] / n;
    const double var = (double)t.s2[c][k] / n - p.mean[k] * p.mean[k];
    p.sigma[k] = std::sqrt(var > 0.0 ? var : 0.0);
  }
  for (int i = 0; i < 24; ++i) {
    p.has_rho[i] = t.r[c][24] != 0 && terms[i] > 0.0;
    if (p.has_rho[i]) p.rho[i] = ((double)t.r[c][i] / terms[i]) / ((double)t.r[c][24] / terms[24]);
  }
  return p;
}

int refuse(char *err, size_t cap, int code, const std::string &m) {
  if (err && cap) snprintf(err, cap, "%s", m.c_str());
  return code;
}

bool read_file(const char *path, std::string &text) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
  std::fclose(f);
  return true;
}

// the report of a clip's record(s) into a file.  "" when fine
std::string write_report(const char *path, const g1s_measure_record_t &total, const g1s_measure_record_t *synth, uint64_t frames,
                         const g1s_y4m_info_t &info) {
  std::vector<char> buf(1 << 16);
  const long n = g1s_format_measure(&total, synth, frames, info.bit_depth, info.width, info.height, info.xdec, info.ydec, info.nplanes, buf.data(),
                                    buf.size());
  if (n < 0) return "formatting the report failed";
  FILE *f = std::fopen(path, "wb");
  if (!f) return std::string("cannot create ") + path;
  const bool ok = std::fwrite(buf.data(), 1, (size_t)n, f) == (size_t)n;
  if (std::fclose(f) != 0 || !ok) return std::string("cannot write ") + path;
  return "";
}

// the temporal report of a clip's temporal record(s) into a file.  "" when fine
std::string write_treport(const char *path, const g1s_measure_trecord_t &total, const g1s_measure_trecord_t *synth, uint64_t pairs,
                          const g1s_y4m_info_t &info) {
  std::vector<char> buf(1 << 16);
  const long n = g1s_format_measure_temporal(&total, synth, pairs, info.bit_depth, info.width, info.height, info.xdec, info.ydec, info.nplanes,
                                             buf.data(), buf.size());
  if (n < 0) return "formatting the temporal report failed";
  FILE *f = std::fopen(path, "wb");
  if (!f) return std::string("cannot create ") + path;
  const bool ok = std::fwrite(buf.data(), 1, (size_t)n, f) == (size_t)n;
  if (std::fclose(f) != 0 || !ok) return std::string("cannot write ") + path;
  return "";
}

// the cross report of a clip's cross record(s) into a file.  "" when fine
std::string write_xreport(const char *path, const g1s_measure_xrecord_t &total, const g1s_measure_xrecord_t *synth, uint64_t frames,
                          const g1s_y4m_info_t &info) {
  std::vector<char> buf(1 << 16);
  const long n = g1s_format_measure_cross(&total, synth, frames, info.bit_depth, info.width, info.height, info.xdec, info.ydec, buf.data(), buf.size());
  if (n < 0) return "formatting the cross report failed";
  FILE *f = std::fopen(path, "wb");
  if (!f) return std::string("cannot create ") + path;
  const bool ok = std::fwrite(buf.data(), 1, (size_t)n, f) == (size_t)n;
  if (std::fclose(f) != 0 || !ok) return std::string("cannot write ") + path;
  return "";
}

const char kCrossNeedsChroma[] = "--cross compares chroma with luma: the clip has no chroma planes";

bool same_clip_shape(const g1s_y4m_info_t &a, const g1s_y4m_info_t &b) {
  return a.width == b.width && a.height == b.height && a.bit_depth == b.bit_depth && a.xdec == b.xdec && a.ydec == b.ydec && a.nplanes == b.nplanes;
}

// the records the meter holds, added to `total`.  "" when fine
std::string take_records(g1s_measure_t *m, std::vector<g1s_measure_record_t> &scratch, g1s_measure_record_t &total) {
  size_t n = 0;
  int rc = g1s_measure_finish(m, nullptr, 0, &n);
  if (rc && rc != G1S_ERR_CAPACITY) return g1s_measure_last_error(m);
  scratch.resize(n + 1);
  scratch[n] = total;
  if (n && (rc = g1s_measure_finish(m, scratch.data(), n, &n)) != 0) return g1s_measure_last_error(m);
  if (g1s_measure_sum(scratch.data(), n + 1, &total) != 0) return "the clip's sums leave 64 bits";
  return "";
}

// the temporal records the meter holds, added to `total` and counted in `pairs`.  "" when fine
std::string take_trecords(g1s_measure_t *m, std::vector<g1s_measure_trecord_t> &scratch, g1s_measure_trecord_t &total, uint64_t &pairs) {
  size_t n = 0;
  int rc = g1s_measure_finish_temporal(m, nullptr, 0, &n);
  if (rc && rc != G1S_ERR_CAPACITY) return g1s_measure_last_error(m);
  scratch.resize(n + 1);
  scratch[n] = total;
  if (n && (rc = g1s_measure_finish_temporal(m, scratch.data(), n, &n)) != 0) return g1s_measure_last_error(m);
  if (g1s_measure_sum_temporal(scratch.data(), n + 1, &total) != 0) return "the clip's temporal sums leave 64 bits";
  pairs += n;
  return "";
}

// the cross records the meter holds, added to `total`.  "" when fine
std::string take_xrecords(g1s_measure_t *m, std::vector<g1s_measure_xrecord_t> &scratch, g1s_measure_xrecord_t &total) {
  size_t n = 0;
  int rc = g1s_measure_finish_cross(m, nullptr, 0, &n);
  if (rc && rc != G1S_ERR_CAPACITY) return g1s_measure_last_error(m);
  scratch.resize(n + 1);
  scratch[n] = total;
  if (n && (rc = g1s_measure_finish_cross(m, scratch.data(), n, &n)) != 0) return g1s_measure_last_error(m);
  if (g1s_measure_sum_cross(scratch.data(), n + 1, &total) != 0) return "the clip's cross sums leave 64 bits";
  return "";
}

// the printed values of plane c of a clip's temporal record (one operation a step, in the order of the grammar)
struct TProfile {
  bool has_bin[kBins];
  double bin[kBins];
  bool has_lag[kTLags];
  double lag[kTLags];
  int peak;  // the lag of largest |rho|, the first on ties; -1: none is defined
};

TProfile tprofile_of(const g1s_measure_trecord_t &t, int c, const double terms[kTLags]) {
  TProfile p{};
  uint64_t U = 0, V = 0;
  for (int k = 0; k < kBins; ++k) {
    U += t.u[c][k], V += t.v[c][k];
    p.has_bin[k] = t.u[c][k] != 0 && t.v[c][k] != 0;
    if (p.has_bin[k]) p.bin[k] = (double)t.x[c][k] / std::sqrt((double)t.u[c][k] * (double)t.v[c][k]);
  }
  const double T = terms[kTLags / 2];
  p.peak = -1;
  for (int i = 0; i < kTLags; ++i) {
    p.has_lag[i] = U != 0 && V != 0 && terms[i] > 0.0;
    if (!p.has_lag[i]) continue;
    p.lag[i] = ((double)t.c[c][i] / terms[i]) / std::sqrt(((double)U / T) * ((double)V / T));
    if (p.peak < 0 || std::fabs(p.lag[i]) > std::fabs(p.lag[p.peak])) p.peak = i;
  }
  return p;
}

std::string peak_text(const TProfile &p) {
  if (p.peak < 0) return "- - -";
  int dx, dy;
  temporal_offset(p.peak, &dx, &dy);
  return std::to_string(dx) + " " + std::to_string(dy) + " " + value(true, p.lag[p.peak]);
}

int not_temporal(g1s_measure_t *m) {
  m->err = "the meter was not made by g1s_measure_new_temporal";  // (not sticky: err_code stays 0)
  return G1S_ERR_INVALID;
}

int not_cross(g1s_measure_t *m) {
  m->err = "the meter was not made by g1s_measure_new_modes with G1S_MEASURE_CROSS";  // (not sticky: err_code stays 0)
  return G1S_ERR_INVALID;
}

int not_scales(g1s_measure_t *m) {
  m->err = "the meter was not made by g1s_measure_new_scales";  // (not sticky: err_code stays 0)
  return G1S_ERR_INVALID;
}

// the scale records the meter holds, added to `total`.  "" when fine
std::string take_srecords(g1s_measure_t *m, std::vector<g1s_measure_srecord_t> &scratch, g1s_measure_srecord_t &total) {
  size_t n = 0;
  int rc = g1s_measure_finish_scales(m, nullptr, 0, &n);
  if (rc && rc != G1S_ERR_CAPACITY) return g1s_measure_last_error(m);
  scratch.resize(n + 1);
  scratch[n] = total;
  if (n && (rc = g1s_measure_finish_scales(m, scratch.data(), n, &n)) != 0) return g1s_measure_last_error(m);
  if (g1s_measure_sum_scales(scratch.data(), n + 1, &total) != 0) return "the clip's scale sums leave 64 bits";
  return "";
}

// the scale report of a clip's plain and scale record(s) into a file.  "" when fine
std::string write_sreport(const char *path, const g1s_measure_record_t &total, const g1s_measure_srecord_t &stotal, const g1s_measure_record_t *synth,
                          const g1s_measure_srecord_t *ssynth, uint64_t frames, const g1s_y4m_info_t &info) {
  std::vector<char> buf(1 << 16);
  const long n = g1s_format_measure_scales(&total, &stotal, synth, ssynth, frames, info.bit_depth, info.nplanes, buf.data(), buf.size());
  if (n < 0) return "formatting the scale report failed";
  FILE *f = std::fopen(path, "wb");
  if (!f) return std::string("cannot create ") + path;
  const bool ok = std::fwrite(buf.data(), 1, (size_t)n, f) == (size_t)n;
  if (std::fclose(f) != 0 || !ok) return std::string("cannot write ") + path;
  return "";
}

// g1s_measure_new, g1s_measure_new_temporal, g1s_measure_new_modes and g1s_measure_new_scales: the same refusals, the same meter but for the buffers
// of the modes
g1s_measure_t *measure_new(uint32_t bit_depth, const g1s_measure_opts_t *opts, uint32_t modes, bool scales = false) {
  g1s_set_global_error_("");
  if (modes & ~(uint32_t)(G1S_MEASURE_TEMPORAL | G1S_MEASURE_CROSS)) {
    g1s_set_global_error_("unknown mode bits: g1s_measure_new_modes takes G1S_MEASURE_TEMPORAL and G1S_MEASURE_CROSS");
    return nullptr;
  }
  const bool temporal = (modes & G1S_MEASURE_TEMPORAL) != 0, cross = (modes & G1S_MEASURE_CROSS) != 0;
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) {
    g1s_set_global_error_("measure is defined for bit depths 8, 10 and 12");
    return nullptr;
  }
  if (opts && opts->struct_size != sizeof(g1s_measure_opts_t)) {
    g1s_set_global_error_("g1s_measure_opts_t.struct_size mismatch");
    return nullptr;
  }
  int device = 0;
  const std::string no_device = pick_device(opts ? opts->device : -1, "measure", &device);
  if (!no_device.empty()) {
    g1s_set_global_error_(no_device.c_str());
    return nullptr;
  }
  g1s_measure *m = new g1s_measure;
  m->temporal = temporal, m->cross = cross, m->scales = scales;
  bool ok = m->open(device, bit_depth, opts ? opts->batch_frames : 0);
  const uint32_t B = m->batch;
  for (Event &e : m->ev) ok = ok && hipEventCreate(&e.p) == hipSuccess;
  for (Event &e : m->ev_c) ok = ok && hipEventCreate(&e.p) == hipSuccess;
  ok = ok && m->p_jobs.alloc(B) && hipMalloc((void **)&m->d_recs.p, sizeof(g1s_measure_record_t) * B) == hipSuccess &&
       hipHostMalloc((void **)&m->h_recs.p, sizeof(g1s_measure_record_t) * B, hipHostMallocDefault) == hipSuccess;
  if (temporal) {
    for (Event &e : m->ev_t) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    for (Event &e : m->ev_tc) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    ok = ok && m->p_tjobs.alloc(B) && hipMalloc((void **)&m->d_trecs.p, sizeof(g1s_measure_trecord_t) * B) == hipSuccess &&
         hipHostMalloc((void **)&m->h_trecs.p, sizeof(g1s_measure_trecord_t) * B, hipHostMallocDefault) == hipSuccess;
  }
  if (cross) {
    for (Event &e : m->ev_x) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    ok = ok && hipMalloc((void **)&m->d_xrecs.p, sizeof(g1s_measure_xrecord_t) * B) == hipSuccess &&
         hipHostMalloc((void **)&m->h_xrecs.p, sizeof(g1s_measure_xrecord_t) * B, hipHostMallocDefault) == hipSuccess;
  }
  if (scales) {
    for (Event &e : m->ev_s) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    ok = ok && hipMalloc((void **)&m->d_srecs.p, sizeof(g1s_measure_srecord_t) * B) == hipSuccess &&
         hipHostMalloc((void **)&m->h_srecs.p, sizeof(g1s_measure_srecord_t) * B, hipHostMallocDefault) == hipSuccess;
  }
  if (!ok) {
    g1s_set_global_error_((std::string("HIP initialisation failed: ") + hipGetErrorString(hipGetLastError())).c_str());
    g1s_measure_free(m);
    return nullptr;
  }
  return m;
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
  if (m->scales && !scales_size_ok(m->bit_depth, noisy->width, noisy->height)) return m->fail(G1S_ERR_INVALID, scales_refusal_text());
  int rc;
  if (m->have_geom && !m->geom.same_shape(*noisy)) {
    // a new geometry: what is queued goes out and finishes first, the buffers are sized again
    if ((rc = m->flush()) != 0) return rc;
    m->have_geom = false;
  }
  if (!m->have_geom && (rc = m->set_geometry(*noisy)) != 0) return rc;
  MeasureJob job{};
  // a plain meter: the batch's slots; a temporal meter: rings of batch + 1 slots, so that the pair before the batch's first
  // pair is still there
  const uint32_t slots = m->temporal ? m->batch + 1 : m->batch, slot = m->temporal ? m->ring_at : (uint32_t)m->jobs.size();
  if ((rc = m->stage_in(*noisy, slot, slots, job.a, job.a_stride, 0)) != 0) return rc;
  if ((rc = m->stage_in(*clean, slot, slots, job.b, job.b_stride, 1)) != 0) return rc;
  if ((rc = m->wait_host_input(noisy->on_device == 0 ? *noisy : *clean)) != 0) return rc;
  m->jobs.push_back(job);
  if (m->temporal) {
    if (m->have_prev) m->tjobs.push_back(TemporalJob{job, m->prev});
    m->prev = job, m->have_prev = true, m->ring_at = (slot + 1) % slots;
    m->prev_staged[0] = noisy->on_device != 1, m->prev_staged[1] = clean->on_device != 1;
  }
  return m->jobs.size() >= m->batch ? m->flush() : G1S_OK;
}

int g1s_measure_cut(g1s_measure_t *m) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  if (!m->temporal) return not_temporal(m);
  (void)hipSetDevice(m->device);
  m->have_prev = false;
  return m->flush();
}

int g1s_measure_finish_temporal(g1s_measure_t *m, g1s_measure_trecord_t *per_pair, size_t cap, size_t *n_out) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  if (!m->temporal) return not_temporal(m);
  (void)hipSetDevice(m->device);
  int rc = m->flush();
  if (rc || (rc = m->keep_prev()) != 0) return rc;
  if (n_out) *n_out = m->trecords.size();
  if (m->trecords.size() > cap || (!per_pair && !m->trecords.empty())) return G1S_ERR_CAPACITY;  // (not sticky: the records stay)
  if (!m->trecords.empty()) std::memcpy(per_pair, m->trecords.data(), sizeof(g1s_measure_trecord_t) * m->trecords.size());
  m->trecords.clear();
  return G1S_OK;
}

int g1s_measure_finish_cross(g1s_measure_t *m, g1s_measure_xrecord_t *per_pair, size_t cap, size_t *n_out) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  if (!m->cross) return not_cross(m);
  (void)hipSetDevice(m->device);
  int rc = m->flush();
  if (rc || (rc = m->keep_prev()) != 0) return rc;
  if (n_out) *n_out = m->xrecords.size();
  if (m->xrecords.size() > cap || (!per_pair && !m->xrecords.empty())) return G1S_ERR_CAPACITY;  // (not sticky: the records stay)
  if (!m->xrecords.empty()) std::memcpy(per_pair, m->xrecords.data(), sizeof(g1s_measure_xrecord_t) * m->xrecords.size());
  m->xrecords.clear();
  return G1S_OK;
}

int g1s_measure_finish_scales(g1s_measure_t *m, g1s_measure_srecord_t *per_pair, size_t cap, size_t *n_out) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  if (!m->scales) return not_scales(m);
  (void)hipSetDevice(m->device);
  int rc = m->flush();
  if (rc || (rc = m->keep_prev()) != 0) return rc;
  if (n_out) *n_out = m->srecords.size();
  if (m->srecords.size() > cap || (!per_pair && !m->srecords.empty())) return G1S_ERR_CAPACITY;  // (not sticky: the records stay)
  if (!m->srecords.empty()) std::memcpy(per_pair, m->srecords.data(), sizeof(g1s_measure_srecord_t) * m->srecords.size());
  m->srecords.clear();
  return G1S_OK;
}

int g1s_measure_scales_timing(g1s_measure_t *m, double *ms_kernel, uint64_t *pairs) {
  if (!m) return G1S_ERR_INVALID;
  if (ms_kernel) *ms_kernel = m->ms_skernel;
  if (pairs) *pairs = m->spairs_timed;
  return G1S_OK;
}

int g1s_measure_cross_timing(g1s_measure_t *m, double *ms_kernel, uint64_t *pairs) {
  if (!m) return G1S_ERR_INVALID;
  if (ms_kernel) *ms_kernel = m->ms_xkernel;
  if (pairs) *pairs = m->xpairs_timed;
  return G1S_OK;
}

int g1s_measure_chroma_timing(g1s_measure_t *m, double *ms_chroma, double *ms_temporal_chroma) {
  if (!m) return G1S_ERR_INVALID;
  if (ms_chroma) *ms_chroma = m->ms_chroma;
  if (ms_temporal_chroma) *ms_temporal_chroma = m->ms_tchroma;
  return G1S_OK;
}

int g1s_measure_temporal_timing(g1s_measure_t *m, double *ms_kernel, uint64_t *pairs) {
  if (!m) return G1S_ERR_INVALID;
  if (ms_kernel) *ms_kernel = m->ms_tkernel;
  if (pairs) *pairs = m->pairs_timed;
  return G1S_OK;
}

int g1s_measure_finish(g1s_measure_t *m, g1s_measure_record_t *per_frame, size_t cap, size_t *n_out) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  (void)hipSetDevice(m->device);
  int rc = m->flush();
  if (rc || (rc = m->keep_prev()) != 0) return rc;
  if (n_out) *n_out = m->records.size();
  if (m->records.size() > cap || (!per_frame && !m->records.empty())) return G1S_ERR_CAPACITY;  // (not sticky: the records stay)
  if (!m->records.empty()) std::memcpy(per_frame, m->records.data(), sizeof(g1s_measure_record_t) * m->records.size());
  m->records.clear();
  return G1S_OK;
}

int g1s_measure_sum(const g1s_measure_record_t *recs, size_t n, g1s_measure_record_t *total) {
  if (!total || (n && !recs)) return G1S_ERR_INVALID;
  g1s_measure_record_t t;
  std::memset(&t, 0, sizeof t);
  bool ok = true;
  for (size_t f = 0; f < n; ++f)
    for (int c = 0; c < 3; ++c) {
      for (int k = 0; k < kBins; ++k)
        ok = checked_add(t.n[c][k], recs[f].n[c][k]) && checked_add(t.s1[c][k], recs[f].s1[c][k]) && checked_add(t.s2[c][k], recs[f].s2[c][k]) && ok;
      for (int i = 0; i < kLags; ++i) ok = checked_add(t.r[c][i], recs[f].r[c][i]) && ok;
    }
  if (!ok) return G1S_ERR_INVALID;
  *total = t;
  return G1S_OK;
}

long g1s_format_measure(const g1s_measure_record_t *total, const g1s_measure_record_t *synth, uint64_t frames, uint32_t bit_depth, uint32_t width,
                        uint32_t height, uint32_t xdec, uint32_t ydec, uint32_t nplanes, char *buf, size_t cap) {
  if (!total || (!buf && cap) || (nplanes != 1 && nplanes != 3) || xdec > 1 || ydec > xdec || width < 1 || height < 1) return G1S_ERR_INVALID;
  g1s_frame_t shape{};
  shape.width = width, shape.height = height, shape.xdec = (uint8_t)xdec, shape.ydec = (uint8_t)ydec, shape.nplanes = (uint8_t)nplanes;
  const PlaneGeom g(shape, 1);
  std::string s = "grainprofile1\n";
  s += "frames " + std::to_string(frames) + " bit_depth " + std::to_string(bit_depth) + " planes " + std::to_string(nplanes) + "\n";
  for (int c = 0; c < (int)nplanes; ++c) {
    s += "plane " + std::to_string(c) + "\n";
    double terms[kLags];
    for (int i = 0; i < kLags; ++i) {
      int dx, dy;
      lag_offset(i, &dx, &dy);
      const int64_t tw = (int64_t)g.pw(c) - std::abs(dx), th = (int64_t)g.ph(c) - std::abs(dy);
      terms[i] = tw > 0 && th > 0 ? (double)tw * (double)th * (double)frames : 0.0;
    }
    const Profile a = profile_of(*total, c, terms);
    Profile b{};
    if (synth) b = profile_of(*synth, c, terms);
    for (int k = 0; k < kBins; ++k) {
      if (!a.has[k]) continue;
      s += "bin " + std::to_string(k) + " " + std::to_string(total->n[c][k]) + " " + value(true, a.mean[k]) + " " + value(true, a.sigma[k]);
      if (synth) s += " " + value(b.has[k], b.mean[k]) + " " + value(b.has[k], b.sigma[k]);
      s += "\n";
    }
    for (int i = 0; i < 24; ++i) {
      int dx, dy;
      lag_offset(i, &dx, &dy);
      s += "lag " + std::to_string(dx) + " " + std::to_string(dy) + " " + value(a.has_rho[i], a.rho[i]);
      if (synth) s += " " + value(b.has_rho[i], b.rho[i]);
      s += "\n";
    }
    if (synth) {
      bool any = false;
      double worst = 0.0, num = 0.0, den = 0.0;
      for (int i = 0; i < 24; ++i)
        if (a.has_rho[i] && b.has_rho[i]) {
          const double e = std::fabs(b.rho[i] - a.rho[i]);
          worst = !any || e > worst ? e : worst, any = true;
        }
      s += "max_rho_diff " + value(any, worst) + "\n";
      for (int k = 0; k < kBins; ++k)
        if (a.has[k] && b.has[k] && a.sigma[k] > 0.0 && b.sigma[k] > 0.0) {
          const double n = (double)total->n[c][k];
          num += n * (b.sigma[k] / a.sigma[k]), den += n;
        }
      s += "sigma_ratio " + value(den > 0.0, den > 0.0 ? num / den : 0.0) + "\n";
    }
  }
  if (s.size() > cap) return G1S_ERR_CAPACITY;
  std::memcpy(buf, s.data(), s.size());
  return (long)s.size();
}

int g1s_measure_sum_temporal(const g1s_measure_trecord_t *recs, size_t n, g1s_measure_trecord_t *total) {
  if (!total || (n && !recs)) return G1S_ERR_INVALID;
  g1s_measure_trecord_t t;
  std::memset(&t, 0, sizeof t);
  bool ok = true;
  for (size_t f = 0; f < n; ++f)
    for (int c = 0; c < 3; ++c) {
      for (int k = 0; k < kBins; ++k)
        ok = checked_add(t.n[c][k], recs[f].n[c][k]) && checked_add(t.x[c][k], recs[f].x[c][k]) && checked_add(t.u[c][k], recs[f].u[c][k]) &&
             checked_add(t.v[c][k], recs[f].v[c][k]) && ok;
      for (int i = 0; i < kTLags; ++i) ok = checked_add(t.c[c][i], recs[f].c[c][i]) && ok;
    }
  if (!ok) return G1S_ERR_INVALID;
  *total = t;
  return G1S_OK;
}

long g1s_format_measure_temporal(const g1s_measure_trecord_t *total, const g1s_measure_trecord_t *synth, uint64_t pairs, uint32_t bit_depth,
                                 uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec, uint32_t nplanes, char *buf, size_t cap) {
  if (!total || (!buf && cap) || (nplanes != 1 && nplanes != 3) || xdec > 1 || ydec > xdec || width < 1 || height < 1) return G1S_ERR_INVALID;
  g1s_frame_t shape{};
  shape.width = width, shape.height = height, shape.xdec = (uint8_t)xdec, shape.ydec = (uint8_t)ydec, shape.nplanes = (uint8_t)nplanes;
  const PlaneGeom g(shape, 1);
  std::string s = "graintemporal1\n";
  s += "pairs " + std::to_string(pairs) + " bit_depth " + std::to_string(bit_depth) + " planes " + std::to_string(nplanes) + "\n";
  for (int c = 0; c < (int)nplanes; ++c) {
    s += "plane " + std::to_string(c) + "\n";
    if (!pairs) continue;
    double terms[kTLags];
    for (int i = 0; i < kTLags; ++i) {
      int dx, dy;
      temporal_offset(i, &dx, &dy);
      const int64_t tw = (int64_t)g.pw(c) - std::abs(dx), th = (int64_t)g.ph(c) - std::abs(dy);
      terms[i] = tw > 0 && th > 0 ? (double)pairs * (double)tw * (double)th : 0.0;
    }
    const TProfile a = tprofile_of(*total, c, terms);
    TProfile b{};
    if (synth) b = tprofile_of(*synth, c, terms);
    for (int k = 0; k < kBins; ++k) {
      if (!total->n[c][k]) continue;
      s += "bin " + std::to_string(k) + " " + std::to_string(total->n[c][k]) + " " + value(a.has_bin[k], a.bin[k]);
      if (synth) s += " " + value(b.has_bin[k], b.bin[k]);
      s += "\n";
    }
    for (int i = 0; i < kTLags; ++i) {
      int dx, dy;
      temporal_offset(i, &dx, &dy);
      s += "lag " + std::to_string(dx) + " " + std::to_string(dy) + " " + value(a.has_lag[i], a.lag[i]);
      if (synth) s += " " + value(b.has_lag[i], b.lag[i]);
      s += "\n";
    }
    s += "temporal_rho " + value(a.has_lag[kTLags / 2], a.lag[kTLags / 2]);
    if (synth) s += " " + value(b.has_lag[kTLags / 2], b.lag[kTLags / 2]);
    s += "\npeak_rho " + peak_text(a);
    if (synth) s += " " + peak_text(b);
    s += "\n";
  }
  if (s.size() > cap) return G1S_ERR_CAPACITY;
  std::memcpy(buf, s.data(), s.size());
  return (long)s.size();
}

int g1s_measure_sum_cross(const g1s_measure_xrecord_t *recs, size_t n, g1s_measure_xrecord_t *total) {
  return g1s_measure_sum_temporal(recs, n, total);  // (one type, one body: the pairing stands where the plane does)
}

long g1s_format_measure_cross(const g1s_measure_xrecord_t *total, const g1s_measure_xrecord_t *synth, uint64_t frames, uint32_t bit_depth,
                              uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec, char *buf, size_t cap) {
  if (!total || (!buf && cap) || xdec > 1 || ydec > xdec || width < 1 || height < 1) return G1S_ERR_INVALID;
  g1s_frame_t shape{};
  shape.width = width, shape.height = height, shape.xdec = (uint8_t)xdec, shape.ydec = (uint8_t)ydec, shape.nplanes = 3;
  const PlaneGeom g(shape, 1);
  static const char *const names[3] = {"cb_luma", "cr_luma", "cb_cr"};
  std::string s = "graincross1\n";
  s += "frames " + std::to_string(frames) + " bit_depth " + std::to_string(bit_depth) + "\n";
  double terms[kTLags];
  for (int i = 0; i < kTLags; ++i) {
    int dx, dy;
    temporal_offset(i, &dx, &dy);
    const int64_t tw = (int64_t)g.pw(1) - std::abs(dx), th = (int64_t)g.ph(1) - std::abs(dy);
    terms[i] = tw > 0 && th > 0 ? (double)frames * (double)tw * (double)th : 0.0;
  }
  // the printed values of a pairing of a record: rule 11's profile (the layouts are one), the slopes beside it
  struct XProfile {
    TProfile t;
    bool has_slope[kBins], has_beta;
    double slope[kBins], beta;
  };
  auto xprofile_of = [&](const g1s_measure_xrecord_t &r, int j) {
    XProfile p{};
    p.t = tprofile_of(r, j, terms);
    uint64_t V = 0;
    for (int k = 0; k < kBins; ++k) {
      V += r.v[j][k];
      p.has_slope[k] = r.v[j][k] != 0;
      if (p.has_slope[k]) p.slope[k] = (double)r.x[j][k] / (double)r.v[j][k];
    }
    p.has_beta = V != 0;
    if (p.has_beta) p.beta = (double)r.c[j][kTLags / 2] / (double)V;
    return p;
  };
  // partial_rho of the three zero_rho of a column
  auto partial = [](const XProfile q[3]) {
    const int z = kTLags / 2;
    if (!q[0].t.has_lag[z] || !q[1].t.has_lag[z] || !q[2].t.has_lag[z]) return value(false, 0.0);
    const double r0 = q[0].t.lag[z], r1 = q[1].t.lag[z], r2 = q[2].t.lag[z];
    const double f0 = 1.0 - r0 * r0, f1 = 1.0 - r1 * r1;
    if (f0 <= 0.0 || f1 <= 0.0) return value(false, 0.0);
    return value(true, (r2 - r0 * r1) / std::sqrt(f0 * f1));
  };
  XProfile a[3], b[3];
  for (int j = 0; j < 3; ++j) {
    s += std::string("pairing ") + names[j] + "\n";
    if (!frames) continue;
    a[j] = xprofile_of(*total, j);
    if (synth) b[j] = xprofile_of(*synth, j);
    for (int k = 0; k < kBins; ++k) {
      if (!total->n[j][k]) continue;
      s += "bin " + std::to_string(k) + " " + std::to_string(total->n[j][k]) + " " + value(a[j].t.has_bin[k], a[j].t.bin[k]) + " " +
           value(a[j].has_slope[k], a[j].slope[k]);
      if (synth) s += " " + value(b[j].t.has_bin[k], b[j].t.bin[k]) + " " + value(b[j].has_slope[k], b[j].slope[k]);
      s += "\n";
    }
    for (int i = 0; i < kTLags; ++i) {
      int dx, dy;
      temporal_offset(i, &dx, &dy);
      s += "lag " + std::to_string(dx) + " " + std::to_string(dy) + " " + value(a[j].t.has_lag[i], a[j].t.lag[i]);
      if (synth) s += " " + value(b[j].t.has_lag[i], b[j].t.lag[i]);
      s += "\n";
    }
    s += "zero_rho " + value(a[j].t.has_lag[kTLags / 2], a[j].t.lag[kTLags / 2]);
    if (synth) s += " " + value(b[j].t.has_lag[kTLags / 2], b[j].t.lag[kTLags / 2]);
    s += "\npeak_rho " + peak_text(a[j].t);
    if (synth) s += " " + peak_text(b[j].t);
    s += "\nbeta " + value(a[j].has_beta, a[j].beta);
    if (synth) s += " " + value(b[j].has_beta, b[j].beta);
    s += "\n";
    if (j == 2) {
      s += "partial_rho " + partial(a);
      if (synth) s += " " + partial(b);
      s += "\n";
    }
  }
  if (s.size() > cap) return G1S_ERR_CAPACITY;
  std::memcpy(buf, s.data(), s.size());
  return (long)s.size();
}

int g1s_measure_set_timing(g1s_measure_t *m, int enable, double *ms_kernel, uint64_t *frames) {
  if (!m) return G1S_ERR_INVALID;
  m->timing = enable != 0;
  if (ms_kernel) *ms_kernel = m->ms_kernel;
  if (frames) *frames = m->frames_timed;
  return G1S_OK;
}

const char *g1s_measure_last_error(const g1s_measure_t *m) { return m ? m->err.c_str() : ""; }

void g1s_measure_free(g1s_measure_t *m) { free_op(m); }

int64_t g1s_measure_y4m_files(const char *noisy, const char *clean, const char *out_report, const g1s_measure_opts_t *opts, int *unequal, char *err,
                              size_t cap) {
  return g1s_measure_y4m_files_temporal(noisy, clean, out_report, nullptr, opts, unequal, err, cap);
}

int64_t g1s_measure_y4m_files_temporal(const char *noisy, const char *clean, const char *out_report, const char *out_treport,
                                       const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap) {
  return g1s_measure_y4m_files_modes(noisy, clean, out_report, out_treport, nullptr, opts, unequal, err, cap);
}

int64_t g1s_measure_y4m_files_modes(const char *noisy, const char *clean, const char *out_report, const char *out_treport, const char *out_xreport,
                                    const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap) {
  return g1s_measure_y4m_files_scales(noisy, clean, out_report, out_treport, out_xreport, nullptr, opts, unequal, err, cap);
}

int64_t g1s_measure_y4m_files_scales(const char *noisy, const char *clean, const char *out_report, const char *out_treport, const char *out_xreport,
                                     const char *out_sreport, const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap) {
  if (unequal) *unequal = 0;
  if (!noisy || !clean || !out_report) return refuse(err, cap, G1S_ERR_INVALID, "null path");
  g1s_y4m_t *ya = g1s_y4m_open(noisy, err, cap);
  if (!ya) return G1S_ERR_INVALID;
  g1s_y4m_t *yb = g1s_y4m_open(clean, err, cap);
  if (!yb) {
    g1s_y4m_close(ya);
    return G1S_ERR_INVALID;
  }
  g1s_y4m_info_t ia, ib;
  g1s_y4m_get_info(ya, &ia), g1s_y4m_get_info(yb, &ib);
  g1s_measure_t *m = nullptr;
  int rc = G1S_OK;
  std::string why;
  int64_t frames = 0;
  g1s_measure_record_t total;
  std::memset(&total, 0, sizeof total);
  std::vector<g1s_measure_record_t> scratch;
  g1s_measure_trecord_t ttotal;
  std::memset(&ttotal, 0, sizeof ttotal);
  std::vector<g1s_measure_trecord_t> tscratch;
  uint64_t pairs = 0;
  g1s_measure_xrecord_t xtotal;
  std::memset(&xtotal, 0, sizeof xtotal);
  std::vector<g1s_measure_xrecord_t> xscratch;
  g1s_measure_srecord_t stotal;
  std::memset(&stotal, 0, sizeof stotal);
  std::vector<g1s_measure_srecord_t> sscratch;
  const uint32_t modes = (out_treport ? G1S_MEASURE_TEMPORAL : 0u) | (out_xreport ? G1S_MEASURE_CROSS : 0u);
  if (!same_clip_shape(ia, ib)) rc = G1S_ERR_DIM_MISMATCH, why = "the two clips differ in geometry or bit depth";
  if (!rc && out_xreport && ia.nplanes != 3) rc = G1S_ERR_INVALID, why = kCrossNeedsChroma;
  if (!rc && !(m = out_sreport ? g1s_measure_new_scales(ia.bit_depth, opts, modes) : g1s_measure_new_modes(ia.bit_depth, opts, modes)))
    rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
  while (!rc) {
    g1s_frame_t fa, fb;
    const int ga = g1s_y4m_next(ya, &fa), gb = g1s_y4m_next(yb, &fb);
    if (ga < 0 || gb < 0) {
      rc = ga < 0 ? ga : gb, why = "frame " + std::to_string(frames) + ": " + (ga < 0 ? g1s_y4m_last_error(ya) : g1s_y4m_last_error(yb));
      break;
    }
    if (ga == 0 || gb == 0) {  // the shorter file ends the clip; one alone: the warning of `diff`
      if (unequal) *unequal = (ga == 0) != (gb == 0);
      break;
    }
    fa.on_device = fb.on_device = 0;  // (the readers lend the frames until their next call: copied before the call returns)
    if ((rc = g1s_measure_frame(m, &fa, &fb)) != 0) {
      why = "frame " + std::to_string(frames) + ": " + g1s_measure_last_error(m);
      break;
    }
    ++frames;
    if (frames % m->batch == 0) {
      if (!(why = take_records(m, scratch, total)).empty()) rc = G1S_ERR_INVALID;
      else if (out_treport && !(why = take_trecords(m, tscratch, ttotal, pairs)).empty()) rc = G1S_ERR_INVALID;
      else if (out_xreport && !(why = take_xrecords(m, xscratch, xtotal)).empty()) rc = G1S_ERR_INVALID;
      else if (out_sreport && !(why = take_srecords(m, sscratch, stotal)).empty()) rc = G1S_ERR_INVALID;
    }
  }
  if (!rc && !(why = take_records(m, scratch, total)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_treport && !(why = take_trecords(m, tscratch, ttotal, pairs)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_xreport && !(why = take_xrecords(m, xscratch, xtotal)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_sreport && !(why = take_srecords(m, sscratch, stotal)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && !(why = write_report(out_report, total, nullptr, (uint64_t)frames, ia)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_treport && !(why = write_treport(out_treport, ttotal, nullptr, pairs, ia)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_xreport && !(why = write_xreport(out_xreport, xtotal, nullptr, (uint64_t)frames, ia)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_sreport && !(why = write_sreport(out_sreport, total, stotal, nullptr, nullptr, (uint64_t)frames, ia)).empty()) rc = G1S_ERR_INVALID;
  g1s_measure_free(m);
  g1s_y4m_close(ya);
  g1s_y4m_close(yb);
  return rc ? refuse(err, cap, rc, why) : frames;
}

int64_t g1s_check_y4m_files(const char *source, const char *denoised, const char *tbl, const char *out_report, const g1s_measure_opts_t *opts,
                            const g1s_grain_opts_t *gopts, int *unequal, char *err, size_t cap) {
  return g1s_check_y4m_files_temporal(source, denoised, tbl, out_report, nullptr, opts, gopts, unequal, err, cap);
}

int64_t g1s_check_y4m_files_temporal(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                     const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts, int *unequal, char *err, size_t cap) {
  return g1s_check_y4m_files_modes(source, denoised, tbl, out_report, out_treport, nullptr, opts, gopts, unequal, err, cap);
}

int64_t g1s_check_y4m_files_modes(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                  const char *out_xreport, const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts, int *unequal, char *err,
                                  size_t cap) {
  return g1s_check_y4m_files_scales(source, denoised, tbl, out_report, out_treport, out_xreport, nullptr, opts, gopts, unequal, err, cap);
}

int64_t g1s_check_y4m_files_scales(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                   const char *out_xreport, const char *out_sreport, const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts,
                                   int *unequal, char *err, size_t cap) {
  if (unequal) *unequal = 0;
  if (!source || !denoised || !tbl || !out_report) return refuse(err, cap, G1S_ERR_INVALID, "null path");
  // the table, as g1s_grain_y4m_file reads it
  std::string text;
  if (!read_file(tbl, text)) return refuse(err, cap, G1S_ERR_INVALID, std::string("cannot open ") + tbl);
  size_t nseg = 0;
  char perr[256] = "";
  std::vector<g1s_segment_t> segs(64);
  int rc = g1s_parse_tbl(text.data(), text.size(), segs.data(), segs.size(), &nseg, perr, sizeof perr);
  if (rc == G1S_ERR_CAPACITY) {
    segs.resize(nseg);
    rc = g1s_parse_tbl(text.data(), text.size(), segs.data(), segs.size(), &nseg, perr, sizeof perr);
  }
  if (rc) return refuse(err, cap, rc, std::string("grain table: ") + perr);
  g1s_y4m_t *ys = g1s_y4m_open(source, err, cap);
  if (!ys) return G1S_ERR_INVALID;
  g1s_y4m_t *yd = g1s_y4m_open(denoised, err, cap);
  if (!yd) {
    g1s_y4m_close(ys);
    return G1S_ERR_INVALID;
  }
  g1s_y4m_info_t is, id;
  g1s_y4m_get_info(ys, &is), g1s_y4m_get_info(yd, &id);
  const PlaneGeom pg(id);
  const Layout lay = staging_layout(pg);
  g1s_measure_t *ms = nullptr, *mr = nullptr;  // source - denoised; rendered - denoised
  g1s_grain_t *gr = nullptr;
  DevBuf<uint8_t> d_src, d_den, d_ren;  // a group of frames each: the source, the denoised, the rendered
  std::string why;
  int64_t frames = 0;
  uint32_t group = 0, in_group = 0;
  g1s_measure_record_t total_s, total_r;
  std::memset(&total_s, 0, sizeof total_s), std::memset(&total_r, 0, sizeof total_r);
  std::vector<g1s_measure_record_t> scratch;
  g1s_measure_trecord_t ttotal_s, ttotal_r;
  std::memset(&ttotal_s, 0, sizeof ttotal_s), std::memset(&ttotal_r, 0, sizeof ttotal_r);
  std::vector<g1s_measure_trecord_t> tscratch;
  uint64_t pairs_s = 0, pairs_r = 0;
  g1s_measure_xrecord_t xtotal_s, xtotal_r;
  std::memset(&xtotal_s, 0, sizeof xtotal_s), std::memset(&xtotal_r, 0, sizeof xtotal_r);
  std::vector<g1s_measure_xrecord_t> xscratch;
  g1s_measure_srecord_t stotal_s, stotal_r;
  std::memset(&stotal_s, 0, sizeof stotal_s), std::memset(&stotal_r, 0, sizeof stotal_r);
  std::vector<g1s_measure_srecord_t> sscratch;
  const uint32_t modes = (out_treport ? G1S_MEASURE_TEMPORAL : 0u) | (out_xreport ? G1S_MEASURE_CROSS : 0u);
  auto meter = [&]() { return out_sreport ? g1s_measure_new_scales(id.bit_depth, opts, modes) : g1s_measure_new_modes(id.bit_depth, opts, modes); };
  if (!same_clip_shape(is, id)) rc = G1S_ERR_DIM_MISMATCH, why = "the two clips differ in geometry or bit depth";
  if (!rc && out_xreport && id.nplanes != 3) rc = G1S_ERR_INVALID, why = kCrossNeedsChroma;
  if (!rc && (!(ms = meter()) || !(mr = meter()))) rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
  if (!rc) {
    g1s_grain_opts_t go{};
    if (gopts) go = *gopts;
    go.struct_size = sizeof go, go.device = ms->device, go.batch_frames = ms->batch;  // one device, one group size
    if (!(gr = g1s_grain_new(id.bit_depth, &go))) rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
  }
  if (!rc) {
    group = ms->batch;
    (void)hipSetDevice(ms->device);
    if (hipMalloc((void **)&d_src.p, lay.frame * group) != hipSuccess || hipMalloc((void **)&d_den.p, lay.frame * group) != hipSuccess ||
        hipMalloc((void **)&d_ren.p, lay.frame * group) != hipSuccess)
      rc = G1S_ERR_HIP, why = "hipMalloc of the frame buffers failed";
  }
  g1s_frame_t shape{};
  shape.width = id.width, shape.height = id.height, shape.xdec = (uint8_t)id.xdec, shape.ydec = (uint8_t)id.ydec, shape.nplanes = (uint8_t)id.nplanes;
  shape.bytes_per_sample = (uint8_t)pg.bps, shape.on_device = 1;
  auto slot = [&](const DevBuf<uint8_t> &buf, uint32_t k) {
    g1s_frame_t f = shape;
    lay.point(f, buf + lay.frame * k, pg.nplanes);
    return f;
  };
  // a group is through: its renders complete (the synthesizer has a stream of its own) before the meters read them, both
  // meters' batches out and waited for, so that the group's buffers are free again
  auto end_group = [&]() {
    if ((rc = g1s_grain_sync(gr)) != 0) why = std::string("render: ") + g1s_grain_last_error(gr);
    for (uint32_t k = 0; k < in_group && !rc; ++k) {
      const g1s_frame_t s = slot(d_src, k), d = slot(d_den, k), r = slot(d_ren, k);
      if ((rc = g1s_measure_frame(ms, &s, &d)) != 0) why = std::string("measure: ") + g1s_measure_last_error(ms);
      else if ((rc = g1s_measure_frame(mr, &r, &d)) != 0) why = std::string("measure: ") + g1s_measure_last_error(mr);
    }
    // (a temporal meter keeps a copy of the group's last pair on the device: the group's buffers are free again all the same)
    for (int k = 0; k < 2 && !rc; ++k)
      if (!(why = take_records(k ? mr : ms, scratch, k ? total_r : total_s)).empty()) rc = G1S_ERR_INVALID;
      else if (out_treport && !(why = take_trecords(k ? mr : ms, tscratch, k ? ttotal_r : ttotal_s, k ? pairs_r : pairs_s)).empty()) rc = G1S_ERR_INVALID;
      else if (out_xreport && !(why = take_xrecords(k ? mr : ms, xscratch, k ? xtotal_r : xtotal_s)).empty()) rc = G1S_ERR_INVALID;
      else if (out_sreport && !(why = take_srecords(k ? mr : ms, sscratch, k ? stotal_r : stotal_s)).empty()) rc = G1S_ERR_INVALID;
    in_group = 0;
  };
  while (!rc) {
    g1s_frame_t fs, fd;
    const int gs = g1s_y4m_next(ys, &fs), gd = g1s_y4m_next(yd, &fd);
    if (gs < 0 || gd < 0) {
      rc = gs < 0 ? gs : gd, why = "frame " + std::to_string(frames) + ": " + (gs < 0 ? g1s_y4m_last_error(ys) : g1s_y4m_last_error(yd));
      break;
    }
    if (gs == 0 || gd == 0) {
      if (unequal) *unequal = (gs == 0) != (gd == 0);
      break;
    }
    // both frames to the device, once (the readers lend them until their next call)
    const g1s_frame_t s = slot(d_src, in_group), d = slot(d_den, in_group);
    g1s_frame_t r = slot(d_ren, in_group);
    bool copied = true;
    for (int c = 0; c < pg.nplanes; ++c)
      copied = copied &&
               hipMemcpy2D(const_cast<void *>(s.data[c]), lay.row[c], fs.data[c], fs.stride_bytes[c], pg.row_bytes(c), pg.ph(c), hipMemcpyHostToDevice) == hipSuccess &&
               hipMemcpy2D(const_cast<void *>(d.data[c]), lay.row[c], fd.data[c], fd.stride_bytes[c], pg.row_bytes(c), pg.ph(c), hipMemcpyHostToDevice) == hipSuccess;
    if (!copied) {
      rc = G1S_ERR_HIP, why = "copy of a frame pair to the device failed";
      break;
    }
    // the table's lookup at the frame's presentation time, as `render` makes it; no segment: rendered = denoised
    const long si = g1s_tbl_segment_for(segs.data(), nseg, g1s::frame_time((uint64_t)frames, id.fps_num, id.fps_den));
    if ((rc = g1s_grain_frame(gr, si < 0 ? nullptr : &segs[(size_t)si], &d, &r)) != 0) {
      why = "frame " + std::to_string(frames) + ": render: " + g1s_grain_last_error(gr);
      break;
    }
    ++frames;
    if (++in_group == group) end_group();
  }
  if (!rc && in_group) end_group();
  if (!rc && !(why = write_report(out_report, total_s, &total_r, (uint64_t)frames, id)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_treport && !(why = write_treport(out_treport, ttotal_s, &ttotal_r, pairs_s, id)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_xreport && !(why = write_xreport(out_xreport, xtotal_s, &xtotal_r, (uint64_t)frames, id)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_sreport && !(why = write_sreport(out_sreport, total_s, stotal_s, &total_r, &stotal_r, (uint64_t)frames, id)).empty()) rc = G1S_ERR_INVALID;
  if (ms) (void)hipSetDevice(ms->device);
  g1s_grain_free(gr);
  g1s_measure_free(mr);
  g1s_measure_free(ms);
  g1s_y4m_close(ys);
  g1s_y4m_close(yd);
  return rc ? refuse(err, cap, rc, why) : frames;
}

}  // extern "C"
