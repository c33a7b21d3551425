// latest.hip -- k4_latest: the per-frame half of the fold (fold.cpp: compute_latest) on the device.
//
// What the reference does per frame after the pixel work (av1-grain diff/solver.rs NoiseModel::update, the part before the
// combined model is touched: the latest state's AR solve, the noise-strength measurements of the flat blocks, the 20-bin
// strength solve) is f64 arithmetic in a fixed order on a few hundred KB of exact integers.  On the host it costs 72 - 85 us of
// a core per 4K frame and needs the whole 285 KB record over PCIe; here one workgroup per frame does it and the host receives
// the 27 KB latest-state blob of fold.h -- the same bytes compute_latest + latest_to_blob produce
// (tests/test_gpu_parity.py::test_device_latest_*):
//   * every f64 operation is the host's operation on the host's operands (-ffp-contract=off on both sides; IEEE divide and
//     square root; int64 -> f64 in one rounding);
//   * every f64 SUM runs in the host's order.
// The kernel is built around SHORT serial chains:
//   * a linear system is solved by ONE wave with the rows in registers (lane = row, columns statically indexed): the
//     reference's "bubble the larger magnitude up" pivoting is a suffix arg-max over the column (the element carried past
//     position i is the first maximum of positions i .. n - 1, position i keeps the loser of its comparison), taken with four
//     DPP row shifts and one v_readlane step across the two rows of 16 -- nothing in the search waits for LDS but the gather
//     of the column by position and the winner's row; the pivot row travels by v_readlane; back substitution by every lane on
//     its own row, the wanted lane's result broadcast.  No barrier.  The three planes' AR systems are solved by three waves at
//     once;
//   * the strength system's entries are sums over the measured blocks in raster order.  Entry (k, k), (k + 1, k) = (k, k + 1)
//     and b[k] only ever meet blocks of bins k - 1 and k: the blocks are taken a STAGE of 512 at a time, their terms computed a
//     thread a block, partitioned by bin IN ORDER into lists in LDS (ballots and popcounts: a stable partition), and lane k adds
//     its list front to back -- one LDS read and one addition an element, no selection, no memory latency in the chain; `total`
//     is one sum over all blocks: one more list (every measured block, in block order), one more lane.  Both chroma planes go
//     through one pass (same blocks, same bins);
//   * the partition and the chains are a two-stage pipeline with ONE barrier a stage: eight partition waves (512 threads) place
//     stage t + 1's terms into list buffer (t + 1) & 1 and then measure and rank stage t + 2 (those stay in registers across
//     the barrier; only the counts go to LDS, double-buffered), while two chain waves add the lists of stage t from buffer
//     t & 1.  The chains are the true serial part (one dependent f64 addition a measured block); the partition of a stage
//     depends on nothing the chains produce.  DESIGN 4.8, profiles/latest_pipeline.txt.
#include "latest_dev.h"

#include "fold.h"

#include <stdio.h>

namespace g1s {
namespace {

// (640 threads: eight partition waves, whose blocks of a stage are base + kPT * r + tid as before, and two chain waves, 8 and 9,
//  that do nothing but add lists.  A stage is 512 blocks: two list buffers of 1 024-block stages for two chroma planes would
//  be 158 KB of a CU's 160; two of 512 are today's footprint.  The lists' order is the blocks' order: rounds first, then waves,
//  then lanes.  profiles/latest_pipeline.txt)
constexpr int kPT = 512, kPW = kPT / 64;            // the partition's threads and waves
constexpr int kCW = 2;                              // chain waves, behind the partition's
constexpr int kT = kPT + 64 * kCW, kWaves = kT / 64;
constexpr int kStage = 512, kRounds = kStage / kPT;  // blocks a stage; a thread's blocks of a stage: base + kPT * r + tid
constexpr double kTinyD = 1.0e-16;                  // TINY_NEAR_ZERO
constexpr double kNorm2D = 255.0 * 255.0;           // BLOCK_NORMALIZATION^2
constexpr int kNL = 2 * kNumBins;                   // lists of a stage: D 0 .. 19 (bins k - 1 and k), L 20 .. 38 (bin k alone), T 39 (every block)
constexpr int kArenaD = 2 * kStage + 8 * kNumBins + 8, kArenaL = kStage + 8 * kNumBins + 8, kArenaT = kStage + 8;
static_assert(kNumBins == 20 && kMaxN == 25, "latest.hip: the solvers' static sizes");
static_assert(kArenaD % 2 == 0 && kArenaL % 2 == 0 && kArenaT % 2 == 0, "latest.hip: the chains read the arenas as double2");

struct Shared {
  // a stage's partitioned terms, in two buffers: stage t's in buffer t & 1
  // (a list's slots start at a multiple of 8 and are zero-filled up to the next one: the chains add whole groups of eight --
  //  a +0.0 changes no sum that is >= +0 or NaN -- and read one group ahead)
  alignas(16) double D[2][kArenaD];  // matrix diagonal terms, list k at [beg[k], end[k])
  double Lw[2][kArenaL];     // off-diagonal terms, list 20 + k
  double Bv[2][2][kArenaD];  // [buffer][plane of the pass]: b terms, the D lists' slots
  double Tv[2][2][kArenaT];  // [buffer][plane of the pass]: noise stds in block order (list 39)
  uint16_t cnt[2][kRounds][kPW][kNL];  // (at most 64 each.  The workgroup's LDS: 90 KB of a CU's 160, one workgroup a CU)
  uint32_t beg[2][kNL], end[2][kNL];
  // results
  double arx[3][kMaxN + 1];
  double gain[3];
  long long nobs[3];
  int ar_ok[3];
  double diag[kNumBins], low[kNumBins], bsum[2][kNumBins], total[2];
  double sb[2][kNumBins], sx[2][kNumBins];
  int st_ok[2];
  double luma_x[kNumBins];
  uint32_t ne;
  uint32_t wsum[kWaves];
};

__device__ __forceinline__ double readlane_f64(double v, int j) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, j), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), j);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// DPP moves of an f64 and of an index (a compile-time control word; lanes whose source lies outside keep `old`)
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double old, double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v), o = (unsigned long long)__double_as_longlong(old);
  const uint32_t lo = (uint32_t)dpp_i32<CTRL>((int)(uint32_t)o, (int)(uint32_t)u), hi = (uint32_t)dpp_i32<CTRL>((int)(uint32_t)(o >> 32), (int)(uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// one step of the suffix arg-max inside a row of 16: the pair D lanes up (row_shl: lane i <- lane i + D; past the row's end
// the -1.0 that no magnitude is below), taken only if strictly larger: the smaller position wins a tie
template <int D>
__device__ __forceinline__ void argmax_step(double &val, int &idx) {
  const double v2 = dpp_f64<0x100 + D>(-1.0, val);
  const int i2 = dpp_i32<0x100 + D>(0, idx);
  if (v2 > val) {
    val = v2;
    idx = i2;
  }
}

// gauss_solve of fold.cpp by one wave: lane r < n holds row r (a[j], j < n) and b of the system; x comes back in every lane
// (x must come in as what a failed solve leaves behind: the caller's cleared x).  The rows stay in their lanes; `rap` (lane p:
// the row at position p) is what the reference's row swaps move.
//   bubble pass over column k, bottom up:  before step i position i holds w(i), the first maximum of |column| over positions
//   i .. n - 1 (`!(up < carried)` moves on to the upper element on a tie), position i - 1 its own element; the larger moves
//   to i - 1.  So after the pass position k holds w(k) and position i > k holds (|c[i - 1]| < |c[w(i)]|) ? row(i - 1) : w(i).
//   w(.) is a suffix arg-max with the smaller position winning ties.  n <= 32: four row shifts give it inside each row of 16
//   lanes, the first row then meets lane 16's (the second row's whole suffix) by v_readlane; the neighbour above comes by
//   wave_shr:1.  Per step two things still go through LDS: |column k| gathered by position and the winner's row.  (No NaN can
//   arise: the pivot is the column's largest magnitude, every multiplier is <= 1 in magnitude.)
template <int NMAX>
__device__ __forceinline__ bool wave_gauss(const int n, double (&a)[NMAX], double b, double (&x)[NMAX], const int lane) {
  static_assert(NMAX <= 32, "wave_gauss: the pivot search covers two rows of 16 lanes");
  int rap = lane;
  bool done = false, ok = true;  // (ok: wave-uniform; a failed solve runs on without touching anything -- no early return out of the unrolled loops, which would send the rows to scratch memory)
#pragma unroll
  for (int k = 0; k < NMAX - 1; ++k) {
    if (k < n - 1 && ok) {
      // |column k| by position
      const double ck = fabs(a[k]);
      double cp = __shfl(ck, rap, 64);
      if (lane < k || lane >= n) cp = -1.0;
      double val = cp;
      int idx = lane;
      argmax_step<1>(val, idx);
      argmax_step<2>(val, idx);
      argmax_step<4>(val, idx);
      argmax_step<8>(val, idx);
      {
        const double v2 = readlane_f64(val, 16);
        const int i2 = __builtin_amdgcn_readlane(idx, 16);
        if (lane < 16 && v2 > val) {
          val = v2;
          idx = i2;
        }
      }
      const int rap_w = __shfl(rap, idx, 64);
      const int rap_up = dpp_i32<0x138>(0, rap);       // wave_shr:1: lane i <- lane i - 1
      const double cp_up = dpp_f64<0x138>(-1.0, cp);
      if (lane >= k && lane < n) rap = (lane == k) ? rap_w : ((cp_up < val) ? rap_up : rap_w);
      const int pr = __builtin_amdgcn_readlane(rap, k);
      const double pk = readlane_f64(a[k], pr), bk = readlane_f64(b, pr);
      if (fabs(pk) < kTinyD) {
        ok = false;
      } else {
        if (lane == pr) done = true;
        const bool active = lane < n && !done;
        const double c = a[k] / pk;
#pragma unroll
        for (int j = k + 1; j < NMAX; ++j) {
          const double pj = readlane_f64(a[j], pr);
          const double t = c * pj;
          if (active && j < n) a[j] = a[j] - t;
        }
        const double t = c * bk;
        if (active) b = b - t;
      }
    }
  }
#pragma unroll
  for (int i = NMAX - 1; i >= 0; --i) {
    if (i < n && ok) {
      const int r = __builtin_amdgcn_readlane(rap, i);
      const double piv = readlane_f64(a[i], r);
      if (fabs(piv) < kTinyD) {
        ok = false;
      } else {
        double c = 0;
#pragma unroll
        for (int j = i + 1; j < NMAX; ++j) {
          const double t = a[j] * x[j];  // (j >= n: a column of zeros times the cleared x: adds +0.0 to a sum that is not -0.0 ... kept out all the same)
          if (j < n) c += t;
        }
        const double xi = (b - c) / a[i];
        x[i] = readlane_f64(xi, r);  // (a broadcast into vector registers: 25 solutions as scalar pairs do not fit the scalar file)
      }
    }
  }
  return ok;
}

__device__ inline double dev_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ inline double dev_bin_index(double value) { return (kNumBins - 1) * dev_clamp(value, 0.0, 255.0) / 255.0; }

// v / count: a division by a power of two (whole blocks' sample counts) is the scaling by it, bit for bit
__device__ __forceinline__ double div_count(double v, int count) {
  return (count & (count - 1)) == 0 ? __builtin_ldexp(v, -__builtin_ctz((unsigned)count)) : v / count;
}

__device__ inline void put_text(char *dst, const char *msg) {
  int i = 0;
  for (; msg[i] && i < 103; ++i) dst[i] = msg[i];
  dst[i] = 0;
}

#ifdef G1S_LATEST_TIMERS
#define K4_TICK(slot)                                 \
  do {                                                \
    __syncthreads();                                  \
    if (tid == 0 && frame == 0) {                     \
      const unsigned long long now_ = wall_clock64(); \
      k4_dbg[slot] += (double)(now_ - k4_t);          \
      k4_t = now_;                                    \
    }                                                 \
  } while (0)
// a wave's own busy time inside the pipeline: no barrier, added up in a register of the wave's lane 0 and written at the pass' end
#define K4_BUSY_BEGIN() const unsigned long long busy_t_ = wall_clock64()
#define K4_BUSY_END(var) (var) += wall_clock64() - busy_t_
#else
#define K4_TICK(slot) \
  do {                \
  } while (0)
#define K4_BUSY_BEGIN() \
  do {                  \
  } while (0)
#define K4_BUSY_END(var) \
  do {                   \
  } while (0)
#endif

struct FrameCtx {
  const uint8_t *rec;
  const uint8_t *mask;
  const uint32_t *luma_sum;
  int nb, nbw, W, H;
};

// One pass over the frame's blocks for the planes c0 .. c0 + NP - 1 (one geometry): the strength system's sums.
// Out: sh.diag / low (the matrix side: bins alone), sh.bsum[q], sh.total[q], sh.ne.
//
// A two-stage pipeline, one barrier a step, every wave at every barrier.  In step t (t = -2 .. stages - 1)
//   the partition waves  PLACE stage t + 1: read its counts (written before the last barrier), work out the offsets, scatter the
//                        terms they hold in registers into list buffer (t + 1) & 1, leave the lists' bounds and zero padding;
//                        then MEASURE stage t + 2: keys, terms, ranks into registers, counts into cnt[t & 1];
//   the chain waves      add the lists of stage t from buffer t & 1.
// Buffer (t + 1) & 1 was last read by the chains in step t - 1 and cnt[t & 1] by the partition in step t - 1: one barrier
// between every write and the reads before and after it.
template <int NP>
__device__ __forceinline__ void strength_pass(Shared &sh, const LatestJob &job, const FrameCtx &fc, const int c0, const int tid, double *k4_dbg, const int frame) {
  const int lane = tid & 63, wave = tid >> 6;
  const bool chain_wave = wave >= kPW;
  const int cw = wave - kPW;  // chain wave 0: the (k, k) sums and the b sums; 1: the (k + 1, k) sums and the totals
  const bool is_chroma = c0 != 0;
  const int sx = is_chroma ? job.xdec : 0, sy = is_chroma ? job.ydec : 0;
  const int bw = kBlock >> sx, bh = kBlock >> sy;
  const int pw = job.W >> sx, ph = job.H >> sy;
  const int32_t *sum_d[NP];
  const uint32_t *sum_d2[NP];
  double noise_gain[NP], corr[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    sum_d[q] = reinterpret_cast<const int32_t *>(fc.rec + job.L.off_sum_d[c0 + q]);
    sum_d2[q] = reinterpret_cast<const uint32_t *>(fc.rec + job.L.off_sum_d2[c0 + q]);
    noise_gain[q] = sh.gain[c0 + q];
    corr[q] = is_chroma ? sh.arx[c0 + q][job.n] : 0;
  }
  const double luma_gain = sh.gain[0];
  const int stages = (fc.nb + kStage - 1) / kStage;
#ifdef G1S_LATEST_TIMERS
  unsigned long long busy_place = 0, busy_measure = 0, busy_chain = 0;
#endif

  // ---- the chain waves' side ----
  // (one chain a lane -- chain wave 0: lanes 0 .. 19 the (k, k) sums, 20 .. 39 plane 0's b[k], 40 .. 59 plane 1's; chain wave 1:
  //  lanes 0 .. 18 the (k + 1, k) sums, lanes 19 and 20 the planes' totals (list 39: every measured block, in block order): an
  //  addition waits for the one before it, the chains next to each other in a wave cost nothing)
  constexpr int kLowLanes = kNumBins - 1;
  const int arr = cw == 0 ? lane / kNumBins : (lane < kLowLanes ? 3 : 4 + (lane - kLowLanes));
  const int li = cw == 0 ? lane % kNumBins : (lane < kLowLanes ? kNumBins + lane : kNL - 1);
  const bool on = chain_wave && (cw == 0 ? arr <= NP : lane < kLowLanes + NP);
  // the lane's arena in buffer 0 and the way to buffer 1, in double2
  const double2 *const src0 = reinterpret_cast<const double2 *>(arr == 0 ? sh.D[0] : arr == 1 ? sh.Bv[0][0] : arr == 2 ? sh.Bv[0][NP - 1] : arr == 3 ? sh.Lw[0] : arr == 4 ? sh.Tv[0][0] : sh.Tv[0][NP - 1]);
  const uint32_t buf_stride = (arr == 0 ? kArenaD : arr <= 2 ? 2 * kArenaD : arr == 3 ? kArenaL : 2 * kArenaT) / 2;
  double acc = 0;
  uint32_t ne = 0;
  if (chain_wave) __builtin_amdgcn_s_setprio(3);  // (the serial part: its additions go ahead of the partition waves on the same SIMD)

  // ---- the partition waves' side: raw words of a stage (requested a stage ahead), the measured stage's terms and ranks ----
  struct Raw {
    uint32_t m, ls;
    int32_t sd[NP];
    uint32_t sd2[NP];
  };
  Raw nxt[kRounds];
  auto fetch = [&](int base) {
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int bi = base + kPT * r + tid;
      const bool in = bi < fc.nb;
      nxt[r].m = in ? fc.mask[bi] : 0u;
      nxt[r].ls = in ? fc.luma_sum[bi] : 0u;
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        nxt[r].sd[q] = in ? sum_d[q][bi] : 0;
        nxt[r].sd2[q] = in ? sum_d2[q][bi] : 0u;
      }
    }
  };
  int key[kRounds];
  double tU[kRounds], tW[kRounds], tV[kRounds], tP[kRounds][NP], tQ[kRounds][NP], tS[kRounds][NP];
  uint32_t rk_own[kRounds], rk_prev[kRounds], rk_low[kRounds], rk_all[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    key[r] = -1;
    tU[r] = tW[r] = tV[r] = 0;
    rk_own[r] = rk_prev[r] = rk_low[r] = rk_all[r] = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q) tP[r][q] = tQ[r][q] = tS[r][q] = 0;
  }
  if (!chain_wave) fetch(0);

  for (int t = -2; t < stages; ++t) {
    if (!chain_wave) {
      if (t >= -1 && t + 1 < stages) {
        // ======== PLACE stage t + 1 ========
        K4_BUSY_BEGIN();
        const int pb = (t + 1) & 1;
        // ---- offsets: list l's slots of (round, wave), rounds first (block order) ----
        // (every wave works them out for itself from the counts, lane l list l, and keeps its own rounds' in registers: no
        //  barrier between the offsets and the scatter; wave 0 leaves the lists' bounds and the zeros behind them for the chains)
        uint32_t my_off[kRounds];
        uint32_t run = 0;
#pragma unroll
        for (int r = 0; r < kRounds; ++r) my_off[r] = 0;
        if (lane < kNL) {
#pragma unroll
          for (int r = 0; r < kRounds; ++r)
#pragma unroll
            for (int w = 0; w < kPW; ++w) {
              if (w == wave) my_off[r] = run;
              run += sh.cnt[pb][r][w][lane];
            }
        }
        {
          // the lists' bases inside their arenas (each list's room a multiple of 8): D lists 0 .. 19 one behind the other, L lists
          // 20 .. 38 likewise, T at 0
          const uint32_t room = (run + 7u) & ~7u;
          uint32_t incl = room;
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += o;
          }
          const uint32_t upto19 = (uint32_t)__shfl((int)incl, kNumBins - 1, 64);
          uint32_t bse = incl - room;
          if (lane >= kNumBins) bse -= upto19;
          if (lane == kNL - 1) bse = 0;
#pragma unroll
          for (int r = 0; r < kRounds; ++r) my_off[r] += bse;
          if (wave == 0 && lane < kNL) {
            sh.beg[pb][lane] = bse;
            sh.end[pb][lane] = bse + run;
            // the zeros behind the list
            if (lane < kNumBins) {
              for (uint32_t i = bse + run; i < bse + room; ++i) {
                sh.D[pb][i] = 0.0;
#pragma unroll
                for (int q = 0; q < NP; ++q) sh.Bv[pb][q][i] = 0.0;
              }
            } else if (lane < kNL - 1) {
              for (uint32_t i = bse + run; i < bse + room; ++i) sh.Lw[pb][i] = 0.0;
            } else {
              for (uint32_t i = run; i < room; ++i) {
#pragma unroll
                for (int q = 0; q < NP; ++q) sh.Tv[pb][q][i] = 0.0;
              }
            }
          }
        }
        // ---- the terms into their lists (a list's base for this wave's round: from the lane that holds it) ----
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
          const int kk = key[r], kq = max(kk, 0);
          const uint32_t o_own = (uint32_t)__shfl((int)my_off[r], kq, 64);
          const uint32_t o_prev = (uint32_t)__shfl((int)my_off[r], min(kq + 1, kNumBins - 1), 64);
          const uint32_t o_low = (uint32_t)__shfl((int)my_off[r], kNumBins + min(kq, kNumBins - 2), 64);
          const uint32_t o_all = (uint32_t)__shfl((int)my_off[r], kNL - 1, 64);
          if (kk < 0) continue;
          const uint32_t so = o_own + rk_own[r];
          sh.D[pb][so] = tU[r];
#pragma unroll
          for (int q = 0; q < NP; ++q) sh.Bv[pb][q][so] = tP[r][q];
          if (kk < kNumBins - 1) {
            const uint32_t sp = o_prev + rk_prev[r];
            sh.D[pb][sp] = tV[r];
#pragma unroll
            for (int q = 0; q < NP; ++q) sh.Bv[pb][q][sp] = tQ[r][q];
            const uint32_t sl = o_low + rk_low[r];
            sh.Lw[pb][sl] = tW[r];
          }
          const uint32_t st = o_all + rk_all[r];
#pragma unroll
          for (int q = 0; q < NP; ++q) sh.Tv[pb][q][st] = tS[r][q];
        }
        K4_BUSY_END(busy_place);
      }
      if (t + 2 < stages) {
        // ======== MEASURE stage t + 2 ========
        K4_BUSY_BEGIN();
        const int base = (t + 2) * kStage, cb = t & 1;
        Raw cur[kRounds];
#pragma unroll
        for (int r = 0; r < kRounds; ++r) cur[r] = nxt[r];
        if (base + kStage < fc.nb) fetch(base + kStage);
        // ---- a thread a block: the measurement and its terms ----
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
          const int bi = base + kPT * r + tid;
          key[r] = -1;
          tU[r] = tW[r] = tV[r] = 0;
#pragma unroll
          for (int q = 0; q < NP; ++q) tP[r][q] = tQ[r][q] = tS[r][q] = 0;
          if (cur[r].m == 0) continue;
          const int by = bi / fc.nbw, bx = bi - by * fc.nbw;
          const int shh = min(ph - by * bh, bh), sw = min(pw - bx * bw, bw);
          if (!(sw * shh > kBlock)) continue;
          const int lw = min(fc.W - bx * kBlock, kBlock), lh = min(fc.H - by * kBlock, kBlock);
          const double block_mean = div_count((double)cur[r].ls, lw * lh);
          const double bin = dev_bin_index(block_mean);
          const int i0 = (int)bin;  // (bin >= 0: the floor)
          const int i1 = min(kNumBins - 1, i0 + 1);
          const double a = bin - i0;
          key[r] = i0;
          tU[r] = (1.0 - a) * (1.0 - a);
          tW[r] = a * (1.0 - a);
          tV[r] = a * a;
          const double luma_strength = is_chroma ? luma_gain * ((1.0 - a) * sh.luma_x[i0] + a * sh.luma_x[i1]) : 0;
#pragma unroll
          for (int q = 0; q < NP; ++q) {
            double noise_mean = (double)cur[r].sd[q];
            const double noise_sq = (double)cur[r].sd2[q];
            noise_mean = div_count(noise_mean, sw * shh);
            const double noise_var = div_count(noise_sq, sw * shh) - noise_mean * noise_mean;
            const double cl = corr[q] * luma_strength;
            const double t0 = noise_var / 16, t1 = noise_var - cl * cl;
            const double uncorr_std = sqrt(t0 > t1 ? t0 : t1);
            const double noise_std = uncorr_std / noise_gain[q];
            tS[r][q] = noise_std;
            tP[r][q] = (1.0 - a) * noise_std;
            tQ[r][q] = a * noise_std;
          }
        }
        // ---- stable partition by bin: ranks inside the wave by ballots ----
        // list k (D): blocks of bin k ("own": the (k, k) term (1 - a)^2, the b term (1 - a) std) and of bin k - 1 ("prev": a^2, a std)
        // list 20 + k (L): blocks of bin k alone (a (1 - a)); list 39 (T): every measured block.
        // A block of the last bin is its own neighbour (i1 = i0 = 19) -- and sits exactly on it: bin = 19 means a = 0, so what the
        // reference adds besides (1 - a)^2 and (1 - a) std are zeros (a (1 - a), a^2, a std with a finite or NaN std), which change
        // no sum that is >= +0 or NaN: the block goes to list 19 as "own" only.
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
          unsigned long long prevB = 0;
          uint32_t mycnt = 0;
          rk_own[r] = rk_prev[r] = rk_low[r] = rk_all[r] = 0;
          const int kk = key[r];
#pragma unroll
          for (int k = 0; k < kNumBins; ++k) {
            const unsigned long long Bk = __ballot(kk == k);
            const unsigned long long M = Bk | prevB;
            if (M == 0) continue;  // (a frame's blocks sit in a few bins: most lists of a stage are empty)
            const uint32_t preM = __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
            const uint32_t preB = __builtin_amdgcn_mbcnt_hi((uint32_t)(Bk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)Bk, 0u));
            if (kk == k) rk_own[r] = preM, rk_low[r] = preB;
            if (kk == k - 1) rk_prev[r] = preM;
            if (lane == k) mycnt = (uint32_t)__popcll(M);
            if (lane == kNumBins + k) mycnt = (uint32_t)__popcll(Bk);
            prevB = Bk;
          }
          {
            const unsigned long long Ma = __ballot(kk >= 0);
            rk_all[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(Ma >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)Ma, 0u));
            if (lane == kNL - 1) mycnt = (uint32_t)__popcll(Ma);
          }
          if (lane < kNL) sh.cnt[cb][r][wave][lane] = (uint16_t)mycnt;
        }
        K4_BUSY_END(busy_measure);
      }
    } else if (t >= 0) {
      // ======== the chains: the lists of stage t front to back ========
      // Groups of eight, the next group's reads in flight while this one is added.
      K4_BUSY_BEGIN();
      const int rb = t & 1;
      if (on) {
        const double2 *src = src0 + (rb ? buf_stride : 0u);
        uint32_t i = sh.beg[rb][li] >> 1;
        const uint32_t e = (sh.end[rb][li] + 1) >> 1;
        double2 va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) va[u] = src[i + u];
        while (i < e) {
#pragma unroll
          for (int u = 0; u < 4; ++u) vb[u] = src[i + 4 + u];
#pragma unroll
          for (int u = 0; u < 4; ++u) acc += va[u].x, acc += va[u].y;
          i += 4;
          if (i < e) {
#pragma unroll
            for (int u = 0; u < 4; ++u) va[u] = src[i + 4 + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += vb[u].x, acc += vb[u].y;
            i += 4;
          }
        }
        if (cw == 1 && lane == kLowLanes) ne += sh.end[rb][kNL - 1];
      }
      K4_BUSY_END(busy_chain);
    }
    __syncthreads();  // (the one barrier of a step)
  }
  if (chain_wave) __builtin_amdgcn_s_setprio(0);
  if (chain_wave && cw == 0) {
    const int k = lane % kNumBins;
    if (arr == 0) sh.diag[k] = acc;
    else if (arr <= NP) sh.bsum[arr - 1][k] = acc;
  } else if (chain_wave) {
    if (lane < kLowLanes) sh.low[lane] = acc;
    else if (lane < kLowLanes + NP) sh.total[lane - kLowLanes] = acc;
    if (lane == kLowLanes) sh.ne = ne;
  }
#ifdef G1S_LATEST_TIMERS
  // (wave 0's measure and place, the two chain waves' additions: each wave's own clock, no barrier)
  if (frame == 0 && lane == 0) {
    if (wave == 0) k4_dbg[6] += (double)busy_measure, k4_dbg[7] += (double)busy_place;
    if (chain_wave) k4_dbg[8 + cw] += (double)busy_chain;
  }
#endif
  __syncthreads();
}

// StrengthSolver::solve of plane q of the pass by the calling wave: b += mean / 8192 (kept: the reference does not undo it), the
// regularised copy of A, the elimination.  Out: sh.sb[q], sh.sx[q], sh.st_ok[q].
__device__ __forceinline__ void strength_solve(Shared &sh, const int q, const int lane) {
  const uint32_t ne = sh.ne;
  double r[kNumBins], x[kNumBins];
  const int i = lane < kNumBins ? lane : 0, nn = kNumBins;
  const double mean = sh.total[q] / (int)ne;
  const double sb = sh.bsum[q][i] + mean / 8192.;
  const double alpha = 2.0 * (double)(int)ne / nn;
  const int lo = max(0, i - 1), hi = min(nn - 1, i + 1);
#pragma unroll
  for (int j = 0; j < kNumBins; ++j) {
    double v = 0.0;
    if (i == j) v = sh.diag[i];
    else if (i == j + 1) v = sh.low[j];
    else if (j == i + 1) v = sh.low[i];
    r[j] = v;
    x[j] = 0.0;
  }
  // (the reference's three updates in its order; lo or hi may be i itself)
#pragma unroll
  for (int j = 0; j < kNumBins; ++j)
    if (j == lo) r[j] -= alpha;
#pragma unroll
  for (int j = 0; j < kNumBins; ++j)
    if (j == i) r[j] += 2 * alpha;
#pragma unroll
  for (int j = 0; j < kNumBins; ++j)
    if (j == hi) r[j] -= alpha;
#pragma unroll
  for (int j = 0; j < kNumBins; ++j)
    if (j == i) r[j] += 1.0 / 8192.;
  const bool ok = wave_gauss<kNumBins>(kNumBins, r, sb, x, lane);
  if (lane < kNumBins) {
    sh.sb[q][lane] = sb;
    double xv = 0.0;
#pragma unroll
    for (int j = 0; j < kNumBins; ++j)
      if (j == lane) xv = x[j];
    sh.sx[q][lane] = xv;
  }
  if (lane == 0) sh.st_ok[q] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kT) void k4_latest(LatestJob job) {
  __shared__ Shared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, frame = blockIdx.x;
  const uint8_t *rec = job.records + job.L.size * (size_t)frame;
  uint8_t *blob = job.blobs + job.blob_bytes * (size_t)frame;
  const int nb = (int)job.L.nblocks;
  const int n = job.n, ncm = n + 1;
  FrameCtx fc;
  fc.rec = rec;
  fc.mask = rec + job.L.off_mask;
  fc.luma_sum = reinterpret_cast<const uint32_t *>(rec + job.L.off_luma_sum);
  fc.nb = nb;
  fc.nbw = job.nbw;
  fc.W = job.W;
  fc.H = job.H;

  double *k4_dbg = reinterpret_cast<double *>(job.scratch);  // (a -DG1S_LATEST_TIMERS build: frame 0's phases, 100 MHz ticks = us x 100)
#ifdef G1S_LATEST_TIMERS
  unsigned long long k4_t = wall_clock64();
  if (tid < 16 && frame == 0) k4_dbg[tid] = 0.0;
  __syncthreads();
#endif
  // ---- the blob: zeros, the header, every plane "cleared" (ar_gain 1) ----
  for (size_t k = tid; k < job.blob_bytes / 8; k += kT) reinterpret_cast<unsigned long long *>(blob)[k] = 0ull;
  LatestHeader *hdr = reinterpret_cast<LatestHeader *>(blob);
  auto plane_head = [&](int c) { return reinterpret_cast<LatestPlaneHead *>(blob + sizeof(LatestHeader) + c * plane_blob_bytes(ncm)); };
  auto plane_doubles = [&](int c) { return reinterpret_cast<double *>(blob + sizeof(LatestHeader) + c * plane_blob_bytes(ncm) + sizeof(LatestPlaneHead)); };
  // flat blocks of the frame
  uint32_t nflat_t = 0;
  for (int b = tid; b < nb; b += kT) nflat_t += fc.mask[b] != 0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) nflat_t += (uint32_t)__shfl_down((int)nflat_t, d, 64);
  if (lane == 0) sh.wsum[wave] = nflat_t;
  __syncthreads();  // (also: the zeros of the blob are behind every later store of this workgroup)
  uint32_t num_flat = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) num_flat += sh.wsum[w];
  if (tid == 0) {
    hdr->magic = kLatestMagic;
    hdr->lag = (uint32_t)job.lag;
    hdr->nplanes = (uint32_t)job.nplanes;
    hdr->status = G1S_OK;
    hdr->size_bytes = (uint32_t)job.blob_bytes;
    hdr->reserved = num_flat;  // (not part of the state: the caller's statistics)
    for (int c = 0; c < 3; ++c) plane_head(c)->ar_gain = 1.0;
  }
  if (num_flat <= 1) {
    if (tid == 0) {
      hdr->status = G1S_ERR_NOT_ENOUGH_FLAT;
      put_text(hdr->err, "Not enough flat blocks to update noise estimate");
    }
    return;
  }
  K4_TICK(0);

  // ---- the planes' AR systems: wave c solves plane c's (exact integer sums -> f64 normal equations, one rounding each) ----
  // den(i, j): 255^2, times ns for the row and for the column of the chroma regressor
  auto ar_entry = [&](int c, int i, int j) -> double {
    const bool is_chroma = c != 0;
    const int nc = n + (is_chroma ? 1 : 0);
    const int64_t *S = reinterpret_cast<const int64_t *>(rec + job.L.off_ar[c]);
    const double ns = is_chroma ? (double)((1 << job.xdec) * (1 << job.ydec)) : 1.0;
    double den = kNorm2D;
    if (is_chroma && i == nc - 1) den *= ns;
    if (is_chroma && j == nc - 1) den *= ns;
    const int64_t s = j == nc ? S[(size_t)nc * nc + i] : (i <= j ? S[i * nc + j] : S[j * nc + i]);  // (j == nc: the b side)
    return (double)s / den;
  };
  if (wave < job.nplanes) {
    const int c = wave;
    const bool is_chroma = c != 0;
    const int nc = n + (is_chroma ? 1 : 0);
    const int row = lane < nc ? lane : 0;
    double a[kMaxN], x[kMaxN];
#pragma unroll
    for (int j = 0; j < kMaxN; ++j) {
      a[j] = j < nc ? ar_entry(c, row, j) : 0.0;
      x[j] = 0.0;
    }
    const double b0 = ar_entry(c, row, nc);
    const double a_diag = ar_entry(c, row, row), a_last = ar_entry(c, row, nc - 1);
    const int64_t nobs = reinterpret_cast<const int64_t *>(rec + job.L.off_ar[c])[(size_t)nc * nc + nc];
    const bool ok = wave_gauss<kMaxN>(nc, a, b0, x, lane);
    // ar_solve's gain (fold.cpp), the sums in its order: lane i holds the i-th term
    double gain = 1.0;
    if (ok) {
      const int m = nc - (is_chroma ? 1 : 0);
      double x_mine = 0.0;
#pragma unroll
      for (int j = 0; j < kMaxN; ++j)
        if (j == lane) x_mine = x[j];
      const double tv = a_diag / nobs;
      double bi = b0, x_last = 0.0;
#pragma unroll
      for (int j = 0; j < kMaxN; ++j)
        if (j == nc - 1) x_last = x[j];
      if (is_chroma) bi -= a_last * x_last;
      const double tc = (bi * x_mine) / nobs;
      double var = 0, sum_covar = 0;
      for (int i = 0; i < m; ++i) var += readlane_f64(tv, i);
      var /= m;
      for (int i = 0; i < m; ++i) sum_covar += readlane_f64(tc, i);
      const double t = var - sum_covar;
      const double noise_var = t > 1e-6 ? t : 1e-6;
      const double q = var / noise_var;
      const double g = sqrt(q > 1e-6 ? q : 1e-6);
      gain = 1 > g ? 1 : g;
    } else if (is_chroma) {  // chroma_fallback: zero AR coefficients, keep only the luma correlation
      const int last = nc - 1;
      const double all = readlane_f64(a_diag, last), bl = readlane_f64(b0, last);
#pragma unroll
      for (int j = 0; j < kMaxN; ++j) x[j] = 0.0;
      if (fabs(all) > 1e-6) {
        const double xl = bl / all;
#pragma unroll
        for (int j = 0; j < kMaxN; ++j)
          if (j == last) x[j] = xl;
      }
    }
    if (lane < nc) {
      double xv = 0.0;
#pragma unroll
      for (int j = 0; j < kMaxN; ++j)
        if (j == lane) xv = x[j];
      sh.arx[c][lane] = xv;
    }
    if (lane == 0) {
      sh.gain[c] = gain;
      sh.nobs[c] = nobs;
      sh.ar_ok[c] = ok ? 1 : 0;
    }
  }
  __syncthreads();
  K4_TICK(1);
  // a plane's AR side into the blob (the host has loaded and solved a plane's system by the time it refuses the frame in that
  // plane's strength solve, and has not touched the planes behind it: each plane's is written when the host would have)
  auto write_ar = [&](int c) {
    const bool is_chroma = c != 0;
    const int nc = n + (is_chroma ? 1 : 0);
    double *pd = plane_doubles(c);
    for (int e = tid; e < nc * nc + nc; e += kT) {
      if (e < nc * nc) {
        const int i = e / nc, j = e - i * nc;
        pd[e] = ar_entry(c, i, j);
      } else {
        const int i = e - nc * nc;
        pd[ncm * ncm + i] = ar_entry(c, i, nc);
        pd[ncm * ncm + ncm + i] = sh.arx[c][i];
      }
    }
    if (tid == 0) {
      LatestPlaneHead *ph = plane_head(c);
      ph->num_observations = sh.nobs[c];
      ph->ar_gain = sh.gain[c];
    }
  };
  auto write_strength = [&](int c, int q) {
    double *qd = plane_doubles(c) + ncm * ncm + 2 * ncm;
    for (int e = tid; e < kNumBins * kNumBins; e += kT) {
      const int i = e / kNumBins, j = e - i * kNumBins;
      double v = 0.0;
      if (i == j) v = sh.diag[i];
      else if (i == j + 1) v = sh.low[j];
      else if (j == i + 1) v = sh.low[i];
      qd[e] = v;
    }
    if (tid < kNumBins) {
      qd[kNumBins * kNumBins + tid] = sh.sb[q][tid];
      qd[kNumBins * kNumBins + kNumBins + tid] = sh.sx[q][tid];
    }
    if (tid == 0) {
      LatestPlaneHead *ph = plane_head(c);
      ph->num_equations = (int32_t)sh.ne;
      ph->total = sh.total[q];
    }
  };
  write_ar(0);
  if (!sh.ar_ok[0]) {
    if (tid == 0) {
      hdr->status = G1S_ERR_SOLVE;
      put_text(hdr->err, "Solving latest noise equation system failed 0!");
    }
    return;
  }
  // ---- luma: noise strength vs. intensity ----
  strength_pass<1>(sh, job, fc, 0, tid, k4_dbg, frame);
  K4_TICK(2);
  if (wave == 0) strength_solve(sh, 0, lane);
  __syncthreads();
  write_strength(0, 0);
  if (tid < kNumBins) sh.luma_x[tid] = sh.sx[0][tid];
  if (!sh.st_ok[0]) {
    if (tid == 0) {
      hdr->status = G1S_ERR_SOLVE;
      put_text(hdr->err, "Solving latest noise strength failed!");
    }
    return;
  }
  __syncthreads();
  K4_TICK(3);
  if (job.nplanes < 3) return;
  // ---- both chroma planes: one pass (the same blocks, the same bins), two solves side by side ----
  strength_pass<2>(sh, job, fc, 1, tid, k4_dbg, frame);
  K4_TICK(4);
  if (wave < 2) strength_solve(sh, wave, lane);
  __syncthreads();
  write_ar(1);
  write_strength(1, 0);
  if (!sh.st_ok[0]) {
    if (tid == 0) {
      hdr->status = G1S_ERR_SOLVE;
      put_text(hdr->err, "Solving latest noise strength failed!");
    }
    return;
  }
  write_ar(2);
  write_strength(2, 1);
  if (!sh.st_ok[1]) {
    if (tid == 0) {
      hdr->status = G1S_ERR_SOLVE;
      put_text(hdr->err, "Solving latest noise strength failed!");
    }
  }
  K4_TICK(5);
}

}  // namespace

size_t latest_scratch_bytes(uint32_t) { return 256; }  // (the timers of a -DG1S_LATEST_TIMERS build; the kernel keeps everything else in LDS)
const char *latest_kernel_name() { return "k4_latest"; }

hipError_t launch_latest(const LatestJob &job, int frames, hipStream_t stream) {
  if (frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(k4_latest, dim3(frames), dim3(kT), 0, stream, job);
#ifdef G1S_LATEST_TIMERS
  {
    double t[16];
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(t, job.scratch, sizeof(t), hipMemcpyDeviceToHost);
    fprintf(stderr, "k4_latest phases, us (frame 0): head %.1f  ar solves %.1f  luma pass %.1f  luma solve %.1f  chroma pass %.1f  chroma solves %.1f | busy inside both passes, each wave's own clock: "
                    "wave 0 measure %.1f  place %.1f  chain wave 8 %.1f  chain wave 9 %.1f\n",
            t[0] / 100, t[1] / 100, t[2] / 100, t[3] / 100, t[4] / 100, t[5] / 100, t[6] / 100, t[7] / 100, t[8] / 100, t[9] / 100);
  }
#endif
  return hipGetLastError();
}

}  // namespace g1s
