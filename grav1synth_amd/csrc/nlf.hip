// nlf.hip -- the noise level function: the estimator's stencil, summed per intensity bin and per plane on the device.
//
// The sums are defined in include/g1s_diff.h ("noise levels", rules N1 - N8); tests/nlf_ref.py restates them in numpy; what
// is done with a record off the device (N4's sum, N5 - N8) is nlf.h.  The gate is the estimator's and has its bias: above
// about sigma = 5 eight-bit code values it thins the sample and keeps the quieter part (a numpy run of N1 - N3 on a noisy
// ramp kept 64 % of the samples at sigma = 8, the per-bin sigma within 2.3 % of the truth).  It is not corrected for.
// Two kernels:
//
//   k_nlf<BPS, B, CHROMA>  k_estimate's structure (estimate.hip): a wave owns 62 x 8 output columns of a strip of 32 rows and
//                    walks it top to bottom with the three rows of the stencil in registers, a word of 8 samples a lane
//                    (16-byte loads where the address allows), the neighbours of a word's ends from the adjacent lanes.
//                    Luma bins by the box sum of the nine samples it already holds; chroma (both planes in one launch) reads
//                    the luma under the lane's samples for `measure`'s rule 2.  A workgroup of 4 waves writes one partial
//                    record with plain stores.
//   k_nlf_tail       a workgroup per (plane, frame) sums the partial records into the frame's record.
//   k_nlf_t<BPS, B, CHROMA>  k_nlf's strip walk on two frames at once ("temporal noise levels", rules T1 - T4): both frames'
//                    three-row windows in registers, both gates and both box sums from them, for chroma both frames'
//                    averageLuma summed as they are read.  The running (k, n, s, q) of a lane goes the same way: s is
//                    signed and at most 256 x 4095 < 2^20 a lane, which hand_on's 32-bit sum carries as two's complement
//                    (a partial record's word is then the i64 of it); one e^2 is below 2^24 and 256 of them reach 2^32, so q
//                    is 64 bits from the first add.  A partial record has k_nlf's layout with s in the place of a, and sums
//                    of two's complement words are the signed sums, so k_nlf_tail sums these too.
// That is `measure`'s scheme: exact, independent of the order anything ran in, no atomics.
//
// The bins: 96 sums a plane.  A lane does not hold 96 accumulators, and 64 lanes do not meet at one LDS word: a lane keeps
// the running (k, n, a, q) of the bin its samples are in, across samples and rows, for as long as k holds; when k changes it
// hands the sums on, and handing on is done by the wave -- for every distinct bin among the lanes that hand on, one masked
// DPP reduction and one LDS update by one lane (km_measure's loop).  A plane of one intensity costs a wave one such update a
// strip.
// The widths: a lane's run lasts a strip at the most, 256 samples: n <= 256, a <= 256 x 2040 < 2^20 fit 32 bits, and their
// sums over 64 lanes do.  One L^2 reaches 32760^2 > 2^30 (a 0 / 4095 checkerboard, which passes the gate): five of them leave
// u32, so q is 64 bits from the first add (below 2^38 a lane) and crosses the lanes as two 16-bit pieces and the rest
// (wave_sum_u64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "est_load.hip.h"
#include "frame_op.h"
#include "nlf.h"
#include "wave_sum.hip.h"

namespace {

constexpr int kEdgeThreshold = 50;  // the estimator's EDGE_THRESHOLD
constexpr int kStripRows = 32;      // output rows per wave strip (+ 2 halo rows)
constexpr int kWavesPerWg = 4, kThreads = 64 * kWavesPerWg;
constexpr int kColsPerWave = 62 * 8;
constexpr int kBins = g1s_nl::kBins, kEntries = 3 * kBins;  // a partial record: n[32], a[32], q[32]
constexpr int kTailGroups = 4;
static_assert(sizeof(g1s_nlf_record_t) == 8 * 3 * kEntries, "k_nlf_tail writes the record as 64-bit words");
static_assert(sizeof(g1s_nlf_trecord_t) == sizeof(g1s_nlf_record_t), "k_nlf_tail writes a temporal record the same way");
constexpr int kBoxGate = 144;  // T2: |S9_t - S9_(t-1)| < 144 2^sh
static_assert((long long)kStripRows * 8 * 4095 * 64 < (1ll << 31), "a wave's sum of e over a strip fits int");
static_assert((long long)kStripRows * 8 * 8 * 255 * 64 < (1ll << 31), "a wave's sum of a over a strip fits int");

struct NlfJob {
  const uint8_t *p[3];
  uint32_t stride[3];  // bytes
};

struct NlfParams {
  const NlfJob *jobs;
  unsigned long long *partials;  // [frame][wgs_frame][kEntries]
  int pw, ph;                    // the class's plane size
  int W, H, xdec, ydec;          // luma size and chroma decimation (read by the chroma launch)
  int col_strips, row_strips;
  uint32_t wgs_frame, wg_base, wgs_plane;
};

// frame t (p) and frame t - 1 (q) of a pair
struct NlfTJob {
  const uint8_t *p[3], *q[3];
  uint32_t stride[3], qstride[3];  // bytes
};

struct NlfTParams {
  const NlfTJob *jobs;
  unsigned long long *partials;  // [pair][wgs_frame][kEntries]
  int pw, ph;
  int W, H, xdec, ydec;
  int col_strips, row_strips;
  uint32_t wgs_frame, wg_base, wgs_plane;
};

struct TailParams {
  const unsigned long long *partials;
  unsigned long long *records;  // [frame] g1s_nlf_record_t
  uint32_t wgs_frame, wgs[3], wg_base[3];
};

// hands on the bin sums of the lanes with `go` set: a reduction and an update a distinct bin.  Wave-uniform control flow.
// (`a` is summed as int and widened with its sign: k_nlf_t's signed s rides in it as two's complement.)
__device__ __forceinline__ void hand_on(bool go, int &cur, uint32_t &n, uint32_t &a, unsigned long long &q, unsigned long long *mine, int lane) {
  unsigned long long todo = __builtin_amdgcn_ballot_w64(go);
  while (todo) {
    const int b = __builtin_amdgcn_readlane(cur, (int)__builtin_ctzll(todo));
    const bool m = go && cur == b;
    todo &= ~__builtin_amdgcn_ballot_w64(m);
    const int sn = wave_sum(m ? (int)n : 0), sa = wave_sum(m ? (int)a : 0);
    const unsigned long long sq = wave_sum_u64(m ? q : 0ull);
    if (lane == 0) {
      mine[b] += (unsigned long long)sn;
      mine[kBins + b] += (unsigned long long)sa;
      mine[2 * kBins + b] += sq;
    }
    if (m) cur = -1, n = a = 0u, q = 0ull;
  }
}

template <int BPS, int B, bool CHROMA>
__global__ __launch_bounds__(kThreads) void k_nlf(NlfParams p) {
  __shared__ unsigned long long s_acc[kWavesPerWg][kEntries];
  constexpr int shift = B - 8, half = shift ? 1 << (shift - 1) : 0;
  const NlfJob &job = p.jobs[blockIdx.z];
  const int c = CHROMA ? 1 + (int)blockIdx.y : 0;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < kWavesPerWg * kEntries; i += kThreads) (&s_acc[0][0])[i] = 0;
  __syncthreads();
  const int strip = (int)blockIdx.x * kWavesPerWg + wave;
  if (strip < p.col_strips * p.row_strips) {  // (uniform in the wave)
    // (column strips are the fast index: the waves of a workgroup read adjacent kilobytes of the same rows)
    const int cs = strip % p.col_strips, rs = strip / p.col_strips;
    const uint8_t *plane = job.p[c], *luma = job.p[0];
    const uint32_t stride = job.stride[c], lstride = job.stride[0];
    const int pw = p.pw, ph = p.ph;
    // output columns of the wave: [cs * 496, cs * 496 + 496) (less the plane's first and last column); lane l holds the
    // word at x0 = cs * 496 - 8 + 8 l, lanes 0 and 63 the halo words
    const int x0 = cs * kColsPerWave - 8 + 8 * lane;
    const int y_first = 1 + rs * kStripRows, y_last = min(y_first + kStripRows, ph - 1);  // output rows [y_first, y_last)
    const bool out_lane = lane >= 1 && lane <= 62;
    int ra[8], rb[8], rc[8];  // rows y - 1, y, y + 1
    est_load<BPS>(plane + (size_t)(y_first - 1) * stride, x0, pw, true, ra);
    est_load<BPS>(plane + (size_t)y_first * stride, x0, pw, y_first < ph, rb);
    int cur = -1;  // the bin the lane's run is in and its sums so far (cur < 0: none)
    uint32_t bn = 0, ba = 0;
    unsigned long long bq = 0;
    unsigned long long *mine = s_acc[wave];
    for (int y = y_first; y < y_last; ++y) {
      est_load<BPS>(plane + (size_t)(y + 1) * stride, x0, pw, y + 1 < ph, rc);
      int l0[8], l1[8];  // chroma: the luma under the lane's samples
      if (CHROMA) {
        const uint8_t *lrow = luma + (size_t)min(y << p.ydec, p.H - 1) * lstride;
        const int lx0 = p.xdec ? 2 * x0 : x0;
        est_load<BPS>(lrow, lx0, p.W, out_lane, l0);
        est_load<BPS>(lrow, lx0 + 8, p.W, out_lane && p.xdec, l1);
      }
      // the column left of the word (the neighbour lane's last sample) and right of it (its first), for the three rows
      const int al = __shfl_up(ra[7], 1), bl = __shfl_up(rb[7], 1), cl = __shfl_up(rc[7], 1);
      const int ar = __shfl_down(ra[0], 1), br = __shfl_down(rb[0], 1), cr = __shfl_down(rc[0], 1);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int x = x0 + k;
        const int m00 = k ? ra[k - 1] : al, m01 = ra[k], m02 = k < 7 ? ra[k + 1] : ar;
        const int m10 = k ? rb[k - 1] : bl, m11 = rb[k], m12 = k < 7 ? rb[k + 1] : br;
        const int m20 = k ? rc[k - 1] : cl, m21 = rc[k], m22 = k < 7 ? rc[k + 1] : cr;
        const int gx = (m00 - m02) + (m20 - m22) + 2 * (m10 - m12);
        const int gy = (m00 - m20) + (m02 - m22) + 2 * (m01 - m21);
        const int ga = (abs(gx) + abs(gy) + half) >> shift;
        const int v = 4 * m11 - 2 * (m01 + m21 + m10 + m12) + (m00 + m02 + m20 + m22);
        const bool on = out_lane && x >= 1 && x < pw - 1 && ga < kEdgeThreshold;
        int bin;
        if (CHROMA) {  // `measure`'s rule 2 on the frame's own luma
          int I;
          if (p.xdec) {
            const int e = 2 * k, i0 = e < 8 ? l0[e & 7] : l1[e & 7], i1 = e < 8 ? l0[(e + 1) & 7] : l1[(e + 1) & 7];
            I = (i0 + ((x << 1) + 1 < p.W ? i1 : i0) + 1) >> 1;
          } else {
            I = l0[k];
          }
          bin = I >> (B - 5);
        } else {
          bin = ((m00 + m01 + m02) + (m10 + m11 + m12) + (m20 + m21 + m22)) / (9 << (B - 5));
        }
        bin = min(bin, kBins - 1);  // (a sample above the depth's maximum: the caller's error, not a wild index)
        const bool change = on && cur >= 0 && bin != cur;
        if (__builtin_amdgcn_ballot_w64(change)) hand_on(change, cur, bn, ba, bq, mine, lane);
        if (on) {
          const uint32_t av = (uint32_t)abs(v);
          cur = bin, bn += 1u, ba += (av + (uint32_t)half) >> shift, bq += (unsigned long long)(av * av);
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        ra[k] = rb[k];
        rb[k] = rc[k];
      }
    }
    hand_on(cur >= 0, cur, bn, ba, bq, mine, lane);
  }
  __syncthreads();
  if (tid < kEntries) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerWg; ++w) t += s_acc[w][tid];
    const size_t at = (size_t)blockIdx.z * p.wgs_frame + p.wg_base + (size_t)blockIdx.y * p.wgs_plane + blockIdx.x;
    p.partials[at * kEntries + tid] = t;
  }
}

// N1's gate value and the box sum of a 3 x 3 neighbourhood
__device__ __forceinline__ void gate_and_box(int m00, int m01, int m02, int m10, int m11, int m12, int m20, int m21, int m22, int half, int shift, int &ga,
                                             int &s9) {
  const int gx = (m00 - m02) + (m20 - m22) + 2 * (m10 - m12);
  const int gy = (m00 - m20) + (m02 - m22) + 2 * (m01 - m21);
  ga = (abs(gx) + abs(gy) + half) >> shift;
  s9 = (m00 + m01 + m02) + (m10 + m11 + m12) + (m20 + m21 + m22);
}

// a[k] += N2's averageLuma of the lane's 8 chroma samples from column x0, the luma row being lrow
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

template <int BPS, int B, bool CHROMA>
__global__ __launch_bounds__(kThreads) void k_nlf_t(NlfTParams p) {
  __shared__ unsigned long long s_acc[kWavesPerWg][kEntries];
  constexpr int shift = B - 8, half = shift ? 1 << (shift - 1) : 0;
  const NlfTJob &job = p.jobs[blockIdx.z];
  const int c = CHROMA ? 1 + (int)blockIdx.y : 0;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < kWavesPerWg * kEntries; i += kThreads) (&s_acc[0][0])[i] = 0;
  __syncthreads();
  const int strip = (int)blockIdx.x * kWavesPerWg + wave;
  if (strip < p.col_strips * p.row_strips) {  // (uniform in the wave)
    const int cs = strip % p.col_strips, rs = strip / p.col_strips;
    const uint8_t *plane = job.p[c], *before = job.q[c];
    const uint32_t stride = job.stride[c], qstride = job.qstride[c];
    const int pw = p.pw, ph = p.ph;
    const int x0 = cs * kColsPerWave - 8 + 8 * lane;
    const int y_first = 1 + rs * kStripRows, y_last = min(y_first + kStripRows, ph - 1);  // output rows [y_first, y_last)
    const bool out_lane = lane >= 1 && lane <= 62;
    int ra[8], rb[8], rc[8];  // frame t: rows y - 1, y, y + 1
    int qa[8], qb[8], qc[8];  // frame t - 1
    est_load<BPS>(plane + (size_t)(y_first - 1) * stride, x0, pw, true, ra);
    est_load<BPS>(plane + (size_t)y_first * stride, x0, pw, y_first < ph, rb);
    est_load<BPS>(before + (size_t)(y_first - 1) * qstride, x0, pw, true, qa);
    est_load<BPS>(before + (size_t)y_first * qstride, x0, pw, y_first < ph, qb);
    int cur = -1;  // the bin the lane's run is in and its sums so far (cur < 0: none); bs is s as two's complement
    uint32_t bn = 0, bs = 0;
    unsigned long long bq = 0;
    unsigned long long *mine = s_acc[wave];
    for (int y = y_first; y < y_last; ++y) {
      est_load<BPS>(plane + (size_t)(y + 1) * stride, x0, pw, y + 1 < ph, rc);
      est_load<BPS>(before + (size_t)(y + 1) * qstride, x0, pw, y + 1 < ph, qc);
      int al2[8];  // chroma: a_t + a_(t-1) under the lane's samples
      if (CHROMA) {
#pragma unroll
        for (int k = 0; k < 8; ++k) al2[k] = 0;
        const size_t lrow = (size_t)min(y << p.ydec, p.H - 1);
        add_average_luma<BPS>(job.p[0] + lrow * job.stride[0], x0, p.W, p.xdec, out_lane, al2);
        add_average_luma<BPS>(job.q[0] + lrow * job.qstride[0], x0, p.W, p.xdec, out_lane, al2);
      }
      const int al = __shfl_up(ra[7], 1), bl = __shfl_up(rb[7], 1), cl = __shfl_up(rc[7], 1);
      const int ar = __shfl_down(ra[0], 1), br = __shfl_down(rb[0], 1), cr = __shfl_down(rc[0], 1);
      const int pal = __shfl_up(qa[7], 1), pbl = __shfl_up(qb[7], 1), pcl = __shfl_up(qc[7], 1);
      const int par = __shfl_down(qa[0], 1), pbr = __shfl_down(qb[0], 1), pcr = __shfl_down(qc[0], 1);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int x = x0 + k;
        int ga, s9, gb, t9;
        gate_and_box(k ? ra[k - 1] : al, ra[k], k < 7 ? ra[k + 1] : ar, k ? rb[k - 1] : bl, rb[k], k < 7 ? rb[k + 1] : br, k ? rc[k - 1] : cl, rc[k],
                     k < 7 ? rc[k + 1] : cr, half, shift, ga, s9);
        gate_and_box(k ? qa[k - 1] : pal, qa[k], k < 7 ? qa[k + 1] : par, k ? qb[k - 1] : pbl, qb[k], k < 7 ? qb[k + 1] : pbr, k ? qc[k - 1] : pcl, qc[k],
                     k < 7 ? qc[k + 1] : pcr, half, shift, gb, t9);
        const bool on = out_lane && x >= 1 && x < pw - 1 && ga < kEdgeThreshold && gb < kEdgeThreshold && abs(s9 - t9) < (kBoxGate << shift);
        int bin = CHROMA ? al2[k] >> (B - 4) : (s9 + t9) / (18 << (B - 5));
        bin = min(bin, kBins - 1);  // (a sample above the depth's maximum: the caller's error, not a wild index)
        const bool change = on && cur >= 0 && bin != cur;
        if (__builtin_amdgcn_ballot_w64(change)) hand_on(change, cur, bn, bs, bq, mine, lane);
        if (on) {
          const int e = rb[k] - qb[k];
          cur = bin, bn += 1u, bs += (uint32_t)e, bq += (unsigned long long)(uint32_t)(e * e);
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        ra[k] = rb[k], rb[k] = rc[k];
        qa[k] = qb[k], qb[k] = qc[k];
      }
    }
    hand_on(cur >= 0, cur, bn, bs, bq, mine, lane);
  }
  __syncthreads();
  if (tid < kEntries) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerWg; ++w) t += s_acc[w][tid];
    const size_t at = (size_t)blockIdx.z * p.wgs_frame + p.wg_base + (size_t)blockIdx.y * p.wgs_plane + blockIdx.x;
    p.partials[at * kEntries + tid] = t;
  }
}

// the frame's record from its workgroups' partial records: grid (plane, frame); a plane without workgroups gets zeros
__global__ __launch_bounds__(128 * kTailGroups) void k_nlf_tail(TailParams p) {
  __shared__ unsigned long long s_sum[kTailGroups][128];
  const int c = (int)blockIdx.x, i = (int)threadIdx.x & 127, g = (int)threadIdx.x >> 7;
  const unsigned long long *src = p.partials + ((size_t)blockIdx.y * p.wgs_frame + p.wg_base[c]) * kEntries;
  unsigned long long t = 0;
  if (i < kEntries)
    for (uint32_t k = (uint32_t)g; k < p.wgs[c]; k += kTailGroups) t += src[(size_t)k * kEntries + i];
  s_sum[g][i] = t;
  __syncthreads();
  if (g == 0 && i < kEntries) {
    for (int v = 1; v < kTailGroups; ++v) t += s_sum[v][i];
    // g1s_nlf_record_t as 64-bit words: n[3][32], a[3][32], q[3][32]
    unsigned long long *rec = p.records + (size_t)blockIdx.y * (sizeof(g1s_nlf_record_t) / 8);
    const int field = i / kBins, k = i - field * kBins;
    rec[field * 3 * kBins + c * kBins + k] = t;
  }
}

}  // namespace

// =============================================================== host engine =====
using namespace g1s_op;

struct g1s_nlf : BatchedOp {
  Event ev[6];  // (3 - 5: around the temporal launches)
  std::vector<NlfJob> jobs;  // the batch being filled
  ParamSets<NlfJob> p_jobs;
  DevBuf<unsigned long long> d_partials;
  size_t partials_cap = 0;
  int col_strips[2] = {0, 0}, row_strips[2] = {0, 0};  // per plane class: luma, chroma
  uint32_t wgs[3] = {0, 0, 0}, wg_base[3] = {0, 0, 0}, wgs_frame = 0;
  DevBuf<g1s_nlf_record_t> d_recs;
  PinnedBuf<g1s_nlf_record_t> h_recs;
  std::vector<g1s_nlf_record_t> records;  // since the last hand-over
  double ms_luma = 0, ms_chroma = 0;
  uint64_t frames_timed = 0;
  // A temporal meter (rules T1 - T5) pairs every frame of a run but the first with the frame before.  Host frames then go
  // round a ring of batch + 1 slots, so that the last frame of a batch is still there under the first of the next; of a
  // caller's device frame that is a batch's last the flush keeps a copy (d_prev).
  bool temporal = false;
  uint64_t run = 0;        // frames of the run so far
  uint32_t next_slot = 0;  // of the input ring
  const uint8_t *prev_p[3] = {nullptr, nullptr, nullptr};  // the frame before: where its planes are read
  uint32_t prev_stride[3] = {0, 0, 0};
  bool prev_is_callers = false;
  std::vector<NlfTJob> tjobs;  // the pairs of the batch being filled
  ParamSets<NlfTJob> p_tjobs;
  DevBuf<unsigned long long> d_tpartials;
  size_t tpartials_cap = 0;
  DevBuf<uint8_t> d_prev;
  DevBuf<g1s_nlf_trecord_t> d_trecs;
  PinnedBuf<g1s_nlf_trecord_t> h_trecs;
  std::vector<g1s_nlf_trecord_t> trecords;  // since the last hand-over
  double ms_tluma = 0, ms_tchroma = 0;
  uint64_t pairs_timed = 0;

  int set_geometry(const g1s_frame_t &f);
  int flush();
  int flush_temporal(int set);
  template <bool CHROMA>
  void launch(const NlfParams &np, dim3 grid);
  template <bool CHROMA>
  void launch_t(const NlfTParams &np, dim3 grid);
};

int g1s_nlf::set_geometry(const g1s_frame_t &f) {
  set_frame_geometry(f);
  wgs_frame = 0;
  for (int c = 0; c < 3; ++c) {
    const int cls = c ? 1 : 0;
    const long pw = c < geom.nplanes ? (long)geom.pw(c) : 0, ph = c < geom.nplanes ? (long)geom.ph(c) : 0;
    // a plane without interior samples (a side shorter than 3) launches nothing
    const bool any = pw >= 3 && ph >= 3;
    col_strips[cls] = any ? (int)((pw - 1 + kColsPerWave - 1) / kColsPerWave) : 0;
    row_strips[cls] = any ? (int)((ph - 2 + kStripRows - 1) / kStripRows) : 0;
    wgs[c] = (uint32_t)((col_strips[cls] * (long)row_strips[cls] + kWavesPerWg - 1) / kWavesPerWg);
    wg_base[c] = wgs_frame;
    wgs_frame += wgs[c];
  }
  const size_t need = (size_t)wgs_frame * kEntries * batch;
  if (need > partials_cap) {
    d_partials = DevBuf<unsigned long long>();
    G1S_OP_TRY(hipMalloc((void **)&d_partials.p, need * sizeof(unsigned long long)));
    partials_cap = need;
  }
  run = 0, d_prev = DevBuf<uint8_t>();
  if (temporal && need > tpartials_cap) {
    d_tpartials = DevBuf<unsigned long long>();
    G1S_OP_TRY(hipMalloc((void **)&d_tpartials.p, need * sizeof(unsigned long long)));
    tpartials_cap = need;
  }
  return G1S_OK;
}

template <bool CHROMA>
void g1s_nlf::launch(const NlfParams &np, dim3 grid) {
  if (bit_depth == 8) hipLaunchKernelGGL((k_nlf<1, 8, CHROMA>), grid, dim3(kThreads), 0, stream, np);
  else if (bit_depth == 10) hipLaunchKernelGGL((k_nlf<2, 10, CHROMA>), grid, dim3(kThreads), 0, stream, np);
  else hipLaunchKernelGGL((k_nlf<2, 12, CHROMA>), grid, dim3(kThreads), 0, stream, np);
}

template <bool CHROMA>
void g1s_nlf::launch_t(const NlfTParams &np, dim3 grid) {
  if (bit_depth == 8) hipLaunchKernelGGL((k_nlf_t<1, 8, CHROMA>), grid, dim3(kThreads), 0, stream, np);
  else if (bit_depth == 10) hipLaunchKernelGGL((k_nlf_t<2, 10, CHROMA>), grid, dim3(kThreads), 0, stream, np);
  else hipLaunchKernelGGL((k_nlf_t<2, 12, CHROMA>), grid, dim3(kThreads), 0, stream, np);
}

// the queued pairs behind the batch's ordinary launches: the same three launches, the temporal records back; then the copy
// of the batch's last frame where its planes are the caller's
int g1s_nlf::flush_temporal(int set) {
  const uint32_t P = (uint32_t)tjobs.size();
  if (P) {
    std::memcpy(p_tjobs.h[set], tjobs.data(), sizeof(NlfTJob) * P);
    G1S_OP_TRY(p_tjobs.upload(set, P, stream));
    NlfTParams np{};
    np.jobs = p_tjobs.d[set], np.partials = d_tpartials;
    np.W = geom.W, np.H = geom.H, np.xdec = geom.subx, np.ydec = geom.suby, np.wgs_frame = wgs_frame;
    if (timing) G1S_OP_TRY(hipEventRecord(ev[3], stream));
    if (wgs[0]) {
      np.pw = geom.W, np.ph = geom.H, np.col_strips = col_strips[0], np.row_strips = row_strips[0];
      np.wg_base = wg_base[0], np.wgs_plane = wgs[0];
      launch_t<false>(np, dim3(wgs[0], 1u, P));
      G1S_OP_TRY(hipGetLastError());
    }
    if (timing) G1S_OP_TRY(hipEventRecord(ev[4], stream));
    if (wgs[1]) {
      np.pw = (int)geom.pw(1), np.ph = (int)geom.ph(1), np.col_strips = col_strips[1], np.row_strips = row_strips[1];
      np.wg_base = wg_base[1], np.wgs_plane = wgs[1];
      launch_t<true>(np, dim3(wgs[1], 2u, P));
      G1S_OP_TRY(hipGetLastError());
    }
    if (timing) G1S_OP_TRY(hipEventRecord(ev[5], stream));
    TailParams tp{};
    tp.partials = d_tpartials, tp.records = reinterpret_cast<unsigned long long *>(d_trecs.p), tp.wgs_frame = wgs_frame;
    for (int c = 0; c < 3; ++c) tp.wgs[c] = wgs[c], tp.wg_base[c] = wg_base[c];
    hipLaunchKernelGGL(k_nlf_tail, dim3(3u, P), dim3(128 * kTailGroups), 0, stream, tp);
    G1S_OP_TRY(hipGetLastError());
    G1S_OP_TRY(hipMemcpyAsync(h_trecs, d_trecs, sizeof(g1s_nlf_trecord_t) * P, hipMemcpyDeviceToHost, stream));
  }
  if (prev_is_callers) {
    if (!d_prev) G1S_OP_TRY(hipMalloc((void **)&d_prev.p, stage.frame));
    for (int c = 0; c < geom.nplanes; ++c) {
      G1S_OP_TRY(hipMemcpy2DAsync(d_prev + stage.off[c], stage.row[c], prev_p[c], prev_stride[c], geom.row_bytes(c), geom.ph(c), hipMemcpyDeviceToDevice, stream));
      prev_p[c] = d_prev + stage.off[c], prev_stride[c] = (uint32_t)stage.row[c];
    }
    prev_is_callers = false;
  }
  return G1S_OK;
}

// the queued frames as one batch: a launch per plane class, the summing launch, the records back, all waited for
int g1s_nlf::flush() {
  const uint32_t B = (uint32_t)jobs.size();
  if (!B) return G1S_OK;
  int set, rc = next_set(&set);
  if (rc) return rc;
  std::memcpy(p_jobs.h[set], jobs.data(), sizeof(NlfJob) * B);
  G1S_OP_TRY(p_jobs.upload(set, B, stream));
  NlfParams np{};
  np.jobs = p_jobs.d[set], np.partials = d_partials;
  np.W = geom.W, np.H = geom.H, np.xdec = geom.subx, np.ydec = geom.suby, np.wgs_frame = wgs_frame;
  if (timing) G1S_OP_TRY(hipEventRecord(ev[0], stream));
  if (wgs[0]) {
    np.pw = geom.W, np.ph = geom.H, np.col_strips = col_strips[0], np.row_strips = row_strips[0];
    np.wg_base = wg_base[0], np.wgs_plane = wgs[0];
    launch<false>(np, dim3(wgs[0], 1u, B));
    G1S_OP_TRY(hipGetLastError());
  }
  if (timing) G1S_OP_TRY(hipEventRecord(ev[1], stream));
  if (wgs[1]) {
    np.pw = (int)geom.pw(1), np.ph = (int)geom.ph(1), np.col_strips = col_strips[1], np.row_strips = row_strips[1];
    np.wg_base = wg_base[1], np.wgs_plane = wgs[1];
    launch<true>(np, dim3(wgs[1], 2u, B));
    G1S_OP_TRY(hipGetLastError());
  }
  if (timing) G1S_OP_TRY(hipEventRecord(ev[2], stream));
  TailParams tp{};
  tp.partials = d_partials, tp.records = reinterpret_cast<unsigned long long *>(d_recs.p), tp.wgs_frame = wgs_frame;
  for (int c = 0; c < 3; ++c) tp.wgs[c] = wgs[c], tp.wg_base[c] = wg_base[c];
  hipLaunchKernelGGL(k_nlf_tail, dim3(3u, B), dim3(128 * kTailGroups), 0, stream, tp);
  G1S_OP_TRY(hipGetLastError());
  G1S_OP_TRY(hipMemcpyAsync(h_recs, d_recs, sizeof(g1s_nlf_record_t) * B, hipMemcpyDeviceToHost, stream));
  if (temporal && (rc = flush_temporal(set)) != 0) return rc;
  if ((rc = set_done(set)) != 0 || (rc = wait()) != 0) return rc;
  if (timing) {
    float ms = 0;
    G1S_OP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    ms_luma += ms;
    G1S_OP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
    ms_chroma += ms, frames_timed += B;
    if (!tjobs.empty()) {
      G1S_OP_TRY(hipEventElapsedTime(&ms, ev[3], ev[4]));
      ms_tluma += ms;
      G1S_OP_TRY(hipEventElapsedTime(&ms, ev[4], ev[5]));
      ms_tchroma += ms, pairs_timed += tjobs.size();
    }
  }
  records.insert(records.end(), h_recs.p, h_recs.p + B);
  trecords.insert(trecords.end(), h_trecs.p, h_trecs.p + tjobs.size());
  jobs.clear(), tjobs.clear();
  return G1S_OK;
}

namespace {

int refuse(char *err, size_t cap, int code, const std::string &m) {
  if (err && cap) snprintf(err, cap, "%s", m.c_str());
  return code;
}

// the records the meter holds, added to `total`.  "" when fine
std::string take_records(g1s_nlf_t *m, std::vector<g1s_nlf_record_t> &scratch, g1s_nlf_record_t &total) {
  size_t n = 0;
  int rc = g1s_nlf_finish(m, nullptr, 0, &n);
  if (rc && rc != G1S_ERR_CAPACITY) return g1s_nlf_last_error(m);
  scratch.resize(n + 1);
  scratch[n] = total;
  if (n && (rc = g1s_nlf_finish(m, scratch.data(), n, &n)) != 0) return g1s_nlf_last_error(m);
  if (!g1s_nl::sum(scratch.data(), n + 1, &total)) return g1s_nl::kSumsLeave64;
  return "";
}

// the same for the temporal records of a temporal meter
std::string take_trecords(g1s_nlf_t *m, std::vector<g1s_nlf_trecord_t> &scratch, g1s_nlf_trecord_t &total, uint64_t &pairs) {
  size_t n = 0;
  int rc = g1s_nlf_finish_temporal(m, nullptr, 0, &n);
  if (rc && rc != G1S_ERR_CAPACITY) return g1s_nlf_last_error(m);
  scratch.resize(n + 1);
  scratch[n] = total;
  if (n && (rc = g1s_nlf_finish_temporal(m, scratch.data(), n, &n)) != 0) return g1s_nlf_last_error(m);
  if (!g1s_nl::sum_t(scratch.data(), n + 1, &total)) return g1s_nl::kSumsLeave64;
  pairs += n;
  return "";
}

std::string write_text(const char *path, const std::string &text) {
  FILE *fo = std::fopen(path, "wb");
  if (!fo) return std::string("cannot create ") + path;
  const bool ok = std::fwrite(text.data(), 1, text.size(), fo) == text.size();
  return std::fclose(fo) != 0 || !ok ? std::string("cannot write ") + path : "";
}

g1s_nlf_t *nlf_new(uint32_t bit_depth, const g1s_nlf_opts_t *opts, bool temporal) {
  g1s_set_global_error_("");
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) {
    g1s_set_global_error_("noise levels are defined for bit depths 8, 10 and 12");
    return nullptr;
  }
  if (opts && opts->struct_size != sizeof(g1s_nlf_opts_t)) {
    g1s_set_global_error_("g1s_nlf_opts_t.struct_size mismatch");
    return nullptr;
  }
  int device = 0;
  const std::string no_device = pick_device(opts ? opts->device : -1, "noise levels", &device);
  if (!no_device.empty()) {
    g1s_set_global_error_(no_device.c_str());
    return nullptr;
  }
  g1s_nlf *m = new g1s_nlf;
  m->temporal = temporal;
  bool ok = m->open(device, bit_depth, opts ? opts->batch_frames : 0);
  const uint32_t B = m->batch;
  for (Event &e : m->ev) ok = ok && hipEventCreate(&e.p) == hipSuccess;
  ok = ok && m->p_jobs.alloc(B) && hipMalloc((void **)&m->d_recs.p, sizeof(g1s_nlf_record_t) * B) == hipSuccess &&
       hipHostMalloc((void **)&m->h_recs.p, sizeof(g1s_nlf_record_t) * B, hipHostMallocDefault) == hipSuccess;
  if (temporal)
    ok = ok && m->p_tjobs.alloc(B) && hipMalloc((void **)&m->d_trecs.p, sizeof(g1s_nlf_trecord_t) * B) == hipSuccess &&
         hipHostMalloc((void **)&m->h_trecs.p, sizeof(g1s_nlf_trecord_t) * B, hipHostMallocDefault) == hipSuccess;
  if (!ok) {
    g1s_set_global_error_((std::string("HIP initialisation failed: ") + hipGetErrorString(hipGetLastError())).c_str());
    g1s_nlf_free(m);
    return nullptr;
  }
  return m;
}

// a .y4m file through a meter (`temporal`: a temporal one, the file one run): the reports, the clip's records
int64_t nlf_y4m_file(const char *source, const char *out_report, const char *out_treport, const g1s_nlf_opts_t *opts, uint64_t max_frames,
                     g1s_nlf_record_t *total_out, g1s_nlf_trecord_t *ttotal_out, bool temporal, char *err, size_t cap) {
  if (!source) return refuse(err, cap, G1S_ERR_INVALID, "null path");
  g1s_y4m_t *y = g1s_y4m_open(source, err, cap);
  if (!y) return G1S_ERR_INVALID;
  g1s_y4m_info_t info;
  g1s_y4m_get_info(y, &info);
  int rc = G1S_OK;
  std::string why;
  int64_t frames = 0;
  uint64_t pairs = 0;
  g1s_nlf_record_t total, first;  // first: the clip's first frame alone, which has no predecessor
  g1s_nlf_trecord_t ttotal;
  std::memset(&total, 0, sizeof total), std::memset(&first, 0, sizeof first), std::memset(&ttotal, 0, sizeof ttotal);
  bool have_first = false;
  std::vector<g1s_nlf_record_t> scratch;
  std::vector<g1s_nlf_trecord_t> tscratch;
  g1s_nlf_t *m = temporal ? g1s_nlf_new_temporal(info.bit_depth, opts) : g1s_nlf_new(info.bit_depth, opts);
  auto take_all = [&]() -> std::string {
    std::string no = take_records(m, scratch, total);
    if (no.empty() && !have_first && scratch.size() > 1) first = scratch[0], have_first = true;
    if (no.empty() && temporal) no = take_trecords(m, tscratch, ttotal, pairs);
    return no;
  };
  if (!m) rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
  while (!rc && (!max_frames || (uint64_t)frames < max_frames)) {
    g1s_frame_t f;
    const int got = g1s_y4m_next(y, &f);
    if (got < 0) {
      rc = got, why = "frame " + std::to_string(frames) + ": " + g1s_y4m_last_error(y);
      break;
    }
    if (got == 0) break;
    f.on_device = 0;  // (the reader lends the frame until its next call: copied before the call returns)
    if ((rc = g1s_nlf_frame(m, &f)) != 0) {
      why = "frame " + std::to_string(frames) + ": " + g1s_nlf_last_error(m);
      break;
    }
    ++frames;
    if (frames % m->batch == 0 && !(why = take_all()).empty()) rc = G1S_ERR_INVALID;
  }
  if (!rc && !(why = take_all()).empty()) rc = G1S_ERR_INVALID;
  if (!rc && out_report && !(why = write_text(out_report, g1s_nl::report(total, (uint64_t)frames, info.bit_depth, info.nplanes, 0))).empty())
    rc = G1S_ERR_INVALID;
  if (!rc && out_treport) {
    g1s_nlf_record_t later = total;  // the ordinary record of the frames with a predecessor
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < kBins; ++k) later.n[c][k] -= first.n[c][k], later.a[c][k] -= first.a[c][k], later.q[c][k] -= first.q[c][k];
    if (!(why = write_text(out_treport, g1s_nl::report_t(ttotal, &later, pairs, info.bit_depth, info.nplanes, 0))).empty()) rc = G1S_ERR_INVALID;
  }
  if (!rc && total_out) *total_out = total;
  if (!rc && ttotal_out) *ttotal_out = ttotal;
  g1s_nlf_free(m);
  g1s_y4m_close(y);
  return rc ? refuse(err, cap, rc, why) : frames;
}

}  // namespace

extern "C" {

g1s_nlf_t *g1s_nlf_new(uint32_t bit_depth, const g1s_nlf_opts_t *opts) { return nlf_new(bit_depth, opts, false); }

g1s_nlf_t *g1s_nlf_new_temporal(uint32_t bit_depth, const g1s_nlf_opts_t *opts) { return nlf_new(bit_depth, opts, true); }

int g1s_nlf_cut(g1s_nlf_t *m) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  m->run = 0;
  return G1S_OK;
}

int g1s_nlf_frame(g1s_nlf_t *m, const g1s_frame_t *f) {
  if (!m || !f) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  (void)hipSetDevice(m->device);
  const Refusal no = check_frame_pair(*f, *f, m->bps, 65536u, "g1s_nlf_new",
                                      "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)");
  if (no.code) return m->fail(no.code, no.text);
  int rc;
  if (m->have_geom && !m->geom.same_shape(*f)) {
    // a new geometry: what is queued goes out and finishes first, the buffers are sized again
    if ((rc = m->flush()) != 0) return rc;
    m->have_geom = false;
  }
  if (!m->have_geom && (rc = m->set_geometry(*f)) != 0) return rc;
  NlfJob job{};
  // (a temporal meter: the ring has a slot more than a batch, and the slots go round)
  const uint32_t slots = m->temporal ? m->batch + 1 : m->batch, slot = m->temporal ? m->next_slot : (uint32_t)m->jobs.size();
  if ((rc = m->stage_in(*f, slot, slots, job.p, job.stride)) != 0) return rc;
  if ((rc = m->wait_host_input(*f)) != 0) return rc;
  m->jobs.push_back(job);
  if (m->temporal) {
    if (f->on_device != 1) m->next_slot = (slot + 1) % slots;
    if (m->run) {
      NlfTJob pair{};
      for (int c = 0; c < m->geom.nplanes; ++c)
        pair.p[c] = job.p[c], pair.stride[c] = job.stride[c], pair.q[c] = m->prev_p[c], pair.qstride[c] = m->prev_stride[c];
      m->tjobs.push_back(pair);
    }
    for (int c = 0; c < m->geom.nplanes; ++c) m->prev_p[c] = job.p[c], m->prev_stride[c] = job.stride[c];
    m->prev_is_callers = f->on_device == 1;
    ++m->run;
  }
  return m->jobs.size() >= m->batch ? m->flush() : G1S_OK;
}

int g1s_nlf_finish(g1s_nlf_t *m, g1s_nlf_record_t *per_frame, size_t cap, size_t *n_out) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  (void)hipSetDevice(m->device);
  const int rc = m->flush();
  if (rc) return rc;
  if (n_out) *n_out = m->records.size();
  if (m->records.size() > cap || (!per_frame && !m->records.empty())) return G1S_ERR_CAPACITY;  // (not sticky: the records stay)
  if (!m->records.empty()) std::memcpy(per_frame, m->records.data(), sizeof(g1s_nlf_record_t) * m->records.size());
  m->records.clear();
  return G1S_OK;
}

int g1s_nlf_finish_temporal(g1s_nlf_t *m, g1s_nlf_trecord_t *per_pair, size_t cap, size_t *n_out) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  if (!m->temporal) {
    m->err = "not a temporal meter: make it with g1s_nlf_new_temporal";  // (the text alone: not sticky)
    return G1S_ERR_INVALID;
  }
  (void)hipSetDevice(m->device);
  const int rc = m->flush();
  if (rc) return rc;
  if (n_out) *n_out = m->trecords.size();
  if (m->trecords.size() > cap || (!per_pair && !m->trecords.empty())) return G1S_ERR_CAPACITY;  // (not sticky: the records stay)
  if (!m->trecords.empty()) std::memcpy(per_pair, m->trecords.data(), sizeof(g1s_nlf_trecord_t) * m->trecords.size());
  m->trecords.clear();
  return G1S_OK;
}

int g1s_nlf_temporal_times(g1s_nlf_t *m, double *ms_luma, double *ms_chroma, uint64_t *pairs) {
  if (!m) return G1S_ERR_INVALID;
  if (ms_luma) *ms_luma = m->ms_tluma;
  if (ms_chroma) *ms_chroma = m->ms_tchroma;
  if (pairs) *pairs = m->pairs_timed;
  return G1S_OK;
}

int g1s_nlf_set_timing(g1s_nlf_t *m, int enable, double *ms_luma, double *ms_chroma, uint64_t *frames) {
  if (!m) return G1S_ERR_INVALID;
  m->timing = enable != 0;
  if (ms_luma) *ms_luma = m->ms_luma;
  if (ms_chroma) *ms_chroma = m->ms_chroma;
  if (frames) *frames = m->frames_timed;
  return G1S_OK;
}

const char *g1s_nlf_last_error(const g1s_nlf_t *m) { return m ? m->err.c_str() : ""; }

void g1s_nlf_free(g1s_nlf_t *m) { free_op(m); }

int64_t g1s_nlf_y4m_file(const char *source, const char *out_report, const g1s_nlf_opts_t *opts, uint64_t max_frames, g1s_nlf_record_t *total_out,
                         char *err, size_t cap) {
  return nlf_y4m_file(source, out_report, nullptr, opts, max_frames, total_out, nullptr, false, err, cap);
}

int64_t g1s_nlf_y4m_file_temporal(const char *source, const char *out_report, const char *out_treport, const g1s_nlf_opts_t *opts, uint64_t max_frames,
                                  g1s_nlf_record_t *total_out, g1s_nlf_trecord_t *ttotal_out, char *err, size_t cap) {
  return nlf_y4m_file(source, out_report, out_treport, opts, max_frames, total_out, ttotal_out, true, err, cap);
}

}  // extern "C"
