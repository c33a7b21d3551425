// nlf_lags.hip -- lagged noise levels: the lagged products of a pair's frame difference over the samples that stand still, on
// the device.
//
// The sums are defined in include/g1s_diff.h ("lagged noise levels", rules L1 - L5); tests/nlf_lags_ref.py restates them in
// numpy; what is done with a record off the device is nlf_table.h.  The meter that queues the pairs and owns the records is
// nlf.hip; here are the two kernels and their launches (nlf_lags.h).
//
//   k_nlf_lags<BPS, B, CHROMA>  a workgroup per tile of 64 x 32 (luma) or 64 x 16 (chroma, both planes in one launch) samples.
//                    It stages both frames of its tile with the ring the lags and the stencil need (7 columns to either
//                    side, 1 row above, 4 below) in LDS, forms T1's e and L1's g once per sample of the tile and its lag
//                    window (6 columns to either side, 3 rows below) into one int16, (e << 1) | g, zero where g = 0 -- so a
//                    product needs no mask and g(p) g(p + d) is the AND of two low bits -- and then every lane walks a column
//                    of the tile, a row of 13 lags at a time.  The chroma launch also stages the two luma frames under its
//                    tile and forms L4's Lbar and gL the same way, (Lbar << 1) | gL, for the 25 cross products.
//   k_nlf_lags_tail  a workgroup per (plane, pair) sums the tiles' partial records into the record.
// That is the meters' scheme: exact, independent of the order anything ran in, no atomics.
//
// A pair (p, p + d) belongs to the tile of p, its upper end, and is counted there once; a cross pair (p, p + delta) belongs to
// the tile of p + delta, the chroma sample, and p lies at or below it in the window the tile has anyway.  What lies outside the
// plane is staged as zero: skipped, not clamped.
// The widths: |e| <= 4095, so (e << 1) | g fits int16 and one product is below 2^24.  A lane adds at most 8 of them to a 32-bit
// sum (below 2^27), the wave's sum crosses the lanes as two 16-bit halves (wave_sum_wide), and from the wave's sum on
// everything is 64 bits.  Counts: a lane's is at most 8, a wave's at most 512: three of them share a register and a reduction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/g1s_diff.h"
#include "nlf_lags.h"
#include "strip_walk.hip.h"
#include "wave_sum.hip.h"

namespace {

using g1s_op::TailParams;
using namespace g1s_nlf_lags;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kBoxGate = 144;  // T2
// the record as 64-bit words
constexpr int kRecN = 0, kRecR = kRecN + 3 * kLags, kRecS = kRecR + 3 * kLags, kRecXn = kRecS + 3, kRecXr = kRecXn + 2 * kCross, kRecLn = kRecXr + 2 * kCross;
static_assert(sizeof(g1s_nlf_lrecord_t) == 8 * (kRecLn + 3), "k_nlf_lags_tail writes the record as 64-bit words");
// a partial record
constexpr int kPartN = 0, kPartR = kLags, kPartS = 2 * kLags, kPartXn = kPartS + 1, kPartXr = kPartXn + kCross, kPartLn = kPartXr + kCross;
static_assert(kPartLn + 3 == kEntries, "a partial record's words");

struct LagParams {
  const NlfTJob *jobs;
  unsigned long long *partials;  // [pair][tiles_frame][kEntries]
  int pw, ph;                    // the class's plane size
  int W, H, xdec, ydec;          // luma size and chroma decimation (read by the chroma launch)
  int tiles_x;
  uint32_t tiles_frame, tile_base, tiles_plane;
};

template <int BPS>
__device__ __forceinline__ uint16_t sample_at(const uint8_t *plane, uint32_t stride, int x, int y) {
  const est_gptr row = est_global(plane) + (size_t)y * stride;
  return BPS == 2 ? ((const EST_GLOBAL uint16_t *)row)[x] : (uint16_t)row[x];
}

// a w x h window of a plane pw x ph from (x_first, y_first) into LDS rows of `pitch`; coordinates outside the plane read the
// nearest sample (no sample that counts looks at those)
template <int BPS>
__device__ __forceinline__ void stage(uint16_t *dst, int pitch, const uint8_t *plane, uint32_t stride, int x_first, int y_first, int w, int h, int pw, int ph,
                                      int tid) {
  for (int i = tid; i < w * h; i += kThreads) {
    const int ry = i / w, rx = i - ry * w;
    dst[ry * pitch + rx] = sample_at<BPS>(plane, stride, min(max(x_first + rx, 0), pw - 1), min(max(y_first + ry, 0), ph - 1));
  }
}

__device__ __forceinline__ Nine nine_at(const uint16_t *s, int pitch, int rx, int ry) {
  const uint16_t *a = s + (ry - 1) * pitch + rx, *b = a + pitch, *c = b + pitch;
  return {a[-1], a[0], a[1], b[-1], b[0], b[1], c[-1], c[0], c[1]};
}

// T2 at a sample whose neighbourhoods in the two frames are m and o
template <int B>
__device__ __forceinline__ bool counts(const Nine &m, const Nine &o) {
  constexpr int shift = B - 8, half = shift ? 1 << (shift - 1) : 0;
  return stencil_gate(m, half, shift) < kEdgeThreshold && stencil_gate(o, half, shift) < kEdgeThreshold &&
         abs(stencil_box(m) - stencil_box(o)) < (kBoxGate << shift);
}

template <int BPS, int B, bool CHROMA>
__global__ __launch_bounds__(kThreads) void k_nlf_lags(LagParams p) {
  constexpr int TH = CHROMA ? kTileRowsChroma : kTileRowsLuma, RPT = TH / kWaves;
  constexpr int RW = kTileW + 14, RH = TH + 5;  // the staged frames: the lag window and the stencil's ring
  constexpr int PW = kTileW + 12, PH = TH + 3;  // the packed window
  constexpr int LW = CHROMA ? 2 * (kTileW + 6) + 2 : 1, LH = CHROMA ? 2 * (TH + 3) + 2 : 1;  // the luma under it, at 4:2:0
  static_assert(RPT * kWaves == TH && RPT <= 8, "a lane's 32-bit sums hold 8 products");
  __shared__ uint16_t s_now[RH * RW], s_before[RH * RW];
  __shared__ uint16_t s_lnow[LH * LW], s_lbefore[LH * LW];
  __shared__ int16_t s_e[PH][PW], s_l[CHROMA ? PH : 1][CHROMA ? PW : 1];
  __shared__ unsigned long long s_acc[kWaves][kEntries];

  const NlfTJob &job = p.jobs[blockIdx.z];
  const int c = CHROMA ? 1 + (int)blockIdx.y : 0;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
  const int x0 = tx * kTileW, y0 = ty * TH, pw = p.pw, ph = p.ph;

  for (int i = tid; i < kWaves * kEntries; i += kThreads) (&s_acc[0][0])[i] = 0;
  stage<BPS>(s_now, RW, job.now.p[c], job.now.stride[c], x0 - 7, y0 - 1, RW, RH, pw, ph, tid);
  stage<BPS>(s_before, RW, job.before.p[c], job.before.stride[c], x0 - 7, y0 - 1, RW, RH, pw, ph, tid);
  // the luma under chroma columns x0 - 3 .. x0 + 66 and rows y0 .. y0 + TH + 2, with the stencil's ring
  const int lx0 = ((x0 - 3) << p.xdec) - 1, ly0 = (y0 << p.ydec) - 1;
  const int lw = ((kTileW + 6) << p.xdec) + 2, lh = ((TH + 3) << p.ydec) + 2;
  if constexpr (CHROMA) {
    stage<BPS>(s_lnow, LW, job.now.p[0], job.now.stride[0], lx0, ly0, lw, lh, p.W, p.H, tid);
    stage<BPS>(s_lbefore, LW, job.before.p[0], job.before.stride[0], lx0, ly0, lw, lh, p.W, p.H, tid);
  }
  __syncthreads();

  // L1 and T1 of every sample of the packed window
  for (int i = tid; i < PH * PW; i += kThreads) {
    const int py = i / PW, px = i - py * PW, x = x0 - 6 + px, y = y0 + py;
    int v = 0;
    if (x >= 1 && x <= pw - 2 && y >= 1 && y <= ph - 2) {
      const Nine m = nine_at(s_now, RW, px + 1, py + 1), o = nine_at(s_before, RW, px + 1, py + 1);
      if (counts<B>(m, o)) v = 2 * (m.m11 - o.m11) + 1;
    }
    s_e[py][px] = (int16_t)v;
    if constexpr (CHROMA) {
      // L4 at chroma sample (x, y): the box of luma differences, Round2 with an arithmetic shift, the clamp
      int l = 0;
      if (px >= 3 && px < PW - 3 && x >= 0 && x < pw && y < ph) {
        int sum = 0;
        bool all = true;
        for (int bi = 0; bi <= p.ydec; ++bi)
          for (int bj = 0; bj <= p.xdec; ++bj) {
            const int X = min((x << p.xdec) + bj, p.W - 1), Y = min((y << p.ydec) + bi, p.H - 1);
            const Nine m = nine_at(s_lnow, LW, X - lx0, Y - ly0), o = nine_at(s_lbefore, LW, X - lx0, Y - ly0);
            all = all && X >= 1 && X <= p.W - 2 && Y >= 1 && Y <= p.H - 2 && counts<B>(m, o);
            sum += m.m11 - o.m11;
          }
        const int s = p.xdec + p.ydec;
        if (all) l = 2 * ((sum + ((1 << s) >> 1)) >> s) + 1;
      }
      s_l[py][px] = (int16_t)l;
    }
  }
  __syncthreads();

  // the lane's column of the tile: rows [wave RPT, wave RPT + RPT)
  unsigned long long *mine = s_acc[wave];
  const int row0 = wave * RPT;
  // One row of lags (dy) at a time, dx = K0 - 6 .. 6: 13 - K0 product sums, and the pair counts three to a register in fields
  // of 10 bits (a lane's count is at most 8, the wave's at most 512).
  auto pass = [&](auto K0c, int dy) __attribute__((always_inline)) {
    constexpr int K0 = decltype(K0c)::value, NK = 13 - K0, NP = (NK + 2) / 3;
    int r[NK], n3[NP];
#pragma unroll
    for (int k = 0; k < NK; ++k) r[k] = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) n3[k] = 0;
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      const int v0 = s_e[row0 + rr][lane + 6], e0 = v0 >> 1;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int w = s_e[row0 + rr + dy][lane + K0 + k];
        r[k] += e0 * (w >> 1), n3[k / 3] += (v0 & w & 1) << (10 * (k % 3));
      }
    }
    int sn3[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) sn3[k] = wave_sum(n3[k]);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int i = dy ? 7 + 13 * (dy - 1) + k : k;  // (K0 = 0 for dy > 0; dy = 0: i = dx)
      const long long sr = wave_sum_wide(r[k]);
      if (lane == 0) mine[kPartN + i] = (unsigned long long)((sn3[k / 3] >> (10 * (k % 3))) & 1023), mine[kPartR + i] = (unsigned long long)sr;
    }
  };
  pass(std::integral_constant<int, 6>(), 0);  // dy = 0: one of each +- pair
#pragma unroll 1
  for (int dy = 1; dy < 4; ++dy) pass(std::integral_constant<int, 0>(), dy);
  {
    int s_sum = 0;
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) s_sum += s_e[row0 + rr][lane + 6] >> 1;
    const int ss = wave_sum(s_sum);
    if (lane == 0) mine[kPartS] = (unsigned long long)(long long)ss;
  }
  if constexpr (CHROMA) {
    // the chroma sample q = p + delta_j is the lane's; Lbar is read at q - delta_j, at or below it
    int xr[kCross], xn[kCross];
#pragma unroll
    for (int j = 0; j < kCross; ++j) xr[j] = xn[j] = 0;
    int ln = 0, ls = 0;
    unsigned long long l2 = 0;
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      const int vq = s_e[row0 + rr][lane + 6], eq = vq >> 1;
#pragma unroll
      for (int j = 0; j < kCross; ++j) {
        const int dxj = j % 7 - 3, dyj = j / 7 - 3;
        const int l = s_l[row0 + rr - dyj][lane + 6 - dxj];
        xr[j] += (l >> 1) * eq, xn[j] += l & vq & 1;
      }
      const int l = s_l[row0 + rr][lane + 6], lb = l >> 1;
      ln += l & 1, ls += lb, l2 += (unsigned long long)(lb * lb);
    }
#pragma unroll
    for (int j = 0; j < kCross; ++j) {
      const int sn = wave_sum(xn[j]);
      const long long sr = wave_sum_wide(xr[j]);
      if (lane == 0) mine[kPartXn + j] = (unsigned long long)sn, mine[kPartXr + j] = (unsigned long long)sr;
    }
    if (blockIdx.y == 0) {  // once a frame
      const int sn = wave_sum(ln), sl = wave_sum(ls);
      const unsigned long long s2 = wave_sum_u64(l2);
      if (lane == 0) mine[kPartLn] = (unsigned long long)sn, mine[kPartLn + 1] = (unsigned long long)(long long)sl, mine[kPartLn + 2] = s2;
    }
  }
  __syncthreads();
  if (tid < kEntries) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += s_acc[w][tid];
    const size_t at = (size_t)blockIdx.z * p.tiles_frame + p.tile_base + (size_t)blockIdx.y * p.tiles_plane + blockIdx.x;
    p.partials[at * kEntries + tid] = t;
  }
}

// the pair's record from its tiles' partial records: grid (plane, pair); a plane without tiles gets zeros
constexpr int kTailGroups = 4, kTailLanes = (int)kTailThreads / kTailGroups;
static_assert(kTailLanes >= kEntries, "a thread a word");
__global__ __launch_bounds__(kTailThreads) void k_nlf_lags_tail(TailParams p) {
  __shared__ unsigned long long s_sum[kTailGroups][kTailLanes];
  const int c = (int)blockIdx.x, i = (int)threadIdx.x % kTailLanes, g = (int)threadIdx.x / kTailLanes;
  const unsigned long long *src = p.partials + ((size_t)blockIdx.y * p.units_frame + p.unit_base[c]) * kEntries;
  unsigned long long t = 0;
  if (i < kEntries)
    for (uint32_t k = (uint32_t)g; k < p.units[c]; k += kTailGroups) t += src[(size_t)k * kEntries + i];
  s_sum[g][i] = t;
  __syncthreads();
  if (g == 0 && i < kEntries) {
    for (int v = 1; v < kTailGroups; ++v) t += s_sum[v][i];
    unsigned long long *rec = p.records + (size_t)blockIdx.y * (sizeof(g1s_nlf_lrecord_t) / 8);
    if (i < kPartR) rec[kRecN + c * kLags + i] = t;
    else if (i < kPartS) rec[kRecR + c * kLags + (i - kPartR)] = t;
    else if (i == kPartS) rec[kRecS + c] = t;
    else if (i < kPartXr) {
      if (c) rec[kRecXn + (c - 1) * kCross + (i - kPartXn)] = t;
    } else if (i < kPartLn) {
      if (c) rec[kRecXr + (c - 1) * kCross + (i - kPartXr)] = t;
    } else if (c == 1) {
      rec[kRecLn + (i - kPartLn)] = t;
    }
  }
}

}  // namespace

namespace g1s_nlf_lags {

void cut(const g1s_op::PlaneGeom &g, g1s_op::Units &tiles) { tiles.cut(g, kTileW, kTileRowsLuma, kTileRowsChroma); }

hipError_t launch(bool chroma, const NlfTJob *d_jobs, uint32_t pairs, unsigned long long *partials, const g1s_op::PlaneGeom &g, const g1s_op::Units &tiles,
                  uint32_t bit_depth, hipStream_t stream) {
  const int c = chroma ? 1 : 0;
  if (!pairs || !tiles.n[c]) return hipSuccess;
  LagParams p{};
  p.jobs = d_jobs, p.partials = partials;
  p.pw = (int)g.pw(c), p.ph = (int)g.ph(c), p.W = g.W, p.H = g.H, p.xdec = g.subx, p.ydec = g.suby;
  p.tiles_x = (p.pw + kTileW - 1) / kTileW;
  p.tiles_frame = tiles.frame, p.tile_base = tiles.base[c], p.tiles_plane = tiles.n[c];
  const dim3 grid(tiles.n[c], chroma ? 2u : 1u, pairs);
  if (chroma) {
    const auto kernel = bit_depth == 8 ? &k_nlf_lags<1, 8, true> : bit_depth == 10 ? &k_nlf_lags<2, 10, true> : &k_nlf_lags<2, 12, true>;
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, p);
  } else {
    const auto kernel = bit_depth == 8 ? &k_nlf_lags<1, 8, false> : bit_depth == 10 ? &k_nlf_lags<2, 10, false> : &k_nlf_lags<2, 12, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, p);
  }
  return hipGetLastError();
}

void (*tail())(g1s_op::TailParams) { return &k_nlf_lags_tail; }

}  // namespace g1s_nlf_lags
