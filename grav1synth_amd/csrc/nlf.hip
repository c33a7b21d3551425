// nlf.hip -- the noise level function: the estimator's stencil, summed per intensity bin and per plane on the device.
//
// The sums are defined in include/g1s_diff.h ("noise levels", rules N1 - N8, and "temporal noise levels", rules T1 - T4);
// tests/nlf_ref.py and tests/nlf_t_ref.py restate them in numpy; what is done with a record off the device is nlf.h, the
// file commands are nlf_file.cpp.  The gate is the estimator's and has its bias: above about sigma = 5 eight-bit code values
// it thins the sample and keeps the quieter part (a numpy run of N1 - N3 on a noisy ramp kept 64 % of the samples at sigma =
// 8, the per-bin sigma within 2.3 % of the truth).  It is not corrected for.
//
// The strip walk -- a wave's strip, the three-row window of a plane in registers, the stencil, averageLuma under a word of
// chroma -- is strip_walk.hip.h, shared with k_estimate.  The two strip kernels here differ in the windows they hold, in
// which samples count, in the bin and in the two values a sample adds; the rest (BinRun, the workgroup's sums) is one text:
//
//   k_nlf<BPS, B, CHROMA>    one window.  Luma bins by the box sum of the nine samples it already holds; chroma (both planes
//                    in one launch) by the luma under the lane's samples, `measure`'s rule 2.  A sample adds |L| rounded to
//                    8-bit scale and L^2.
//   k_nlf_t<BPS, B, CHROMA>  two windows, frame t and frame t - 1 of a pair: both gates, the two box sums against each other,
//                    the bin by both box sums or both frames' averageLuma.  A sample adds e and e^2 of the difference e.  e is
//                    signed: a lane's sum is at most 256 x 4095 < 2^20, which the 32-bit sums carry as two's complement (a
//                    partial record's word is then the i64 of it), and sums of two's complement words are the signed sums.
//   k_nlf_tail       a workgroup per (plane, frame or pair) sums the partial records of either kernel into the record.
// That is `measure`'s scheme: exact, independent of the order anything ran in, no atomics.
//
// The bins: 96 sums a plane.  A lane does not hold 96 accumulators, and 64 lanes do not meet at one LDS word: a lane keeps
// the running (k, n, a, q) of the bin its samples are in, across samples and rows, for as long as k holds; when k changes it
// hands the sums on, and handing on is done by the wave -- for every distinct bin among the lanes that hand on, one masked
// DPP reduction and one LDS update by one lane (km_measure's loop).  A plane of one intensity costs a wave one such update a
// strip.
// The widths: a lane's run lasts a strip at the most, 256 samples: n <= 256, a <= 256 x 2040 < 2^20 fit 32 bits, and their
// sums over 64 lanes do.  One L^2 reaches 32760^2 > 2^30 (a 0 / 4095 checkerboard, which passes the gate): five of them leave
// u32, and 256 e^2 below 2^24 each reach 2^32, so q is 64 bits from the first add (below 2^38 a lane) and crosses the lanes as
// two 16-bit pieces and the rest (wave_sum_u64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "meter_op.h"
#include "nlf.h"
#include "nlf_lags.h"
#include "strip_walk.hip.h"
#include "wave_sum.hip.h"

namespace {

using g1s_op::TailParams;

constexpr int kBins = g1s_nl::kBins, kEntries = 3 * kBins;  // a partial record: n[32], a[32], q[32]
constexpr int kTailGroups = 4;
static_assert(sizeof(g1s_nlf_record_t) == 8 * 3 * kEntries, "k_nlf_tail writes the record as 64-bit words");
static_assert(sizeof(g1s_nlf_trecord_t) == sizeof(g1s_nlf_record_t), "k_nlf_tail writes a temporal record the same way");
constexpr int kBoxGate = 144;  // T2: |S9_t - S9_(t-1)| < 144 2^sh
static_assert((long long)kStripRows * 8 * 4095 * 64 < (1ll << 31), "a wave's sum of e over a strip fits int");
static_assert((long long)kStripRows * 8 * 8 * 255 * 64 < (1ll << 31), "a wave's sum of a over a strip fits int");

// what a strip kernel is launched with; Job: NlfJob (k_nlf) or NlfTJob (k_nlf_t)
template <class Job>
struct NlfParams {
  const Job *jobs;
  unsigned long long *partials;  // [frame or pair][wgs_frame][kEntries]
  int pw, ph;                    // the class's plane size
  int W, H, xdec, ydec;          // luma size and chroma decimation (read by the chroma launch)
  int col_strips, row_strips;
  uint32_t wgs_frame, wg_base, wgs_plane;
};

// A lane's run: the bin its samples are in and their sums so far (cur < 0: none), and the wave's sums in LDS they go to.
// (`a` is summed as int and widened with its sign: k_nlf_t's signed s rides in it as two's complement.)
struct BinRun {
  int cur = -1;
  uint32_t n = 0, a = 0;
  unsigned long long q = 0;
  unsigned long long *mine;
  int lane;
  __device__ __forceinline__ BinRun(unsigned long long *mine_, int lane_) : mine(mine_), lane(lane_) {}
  // hands on the bin sums of the lanes with `go` set: a reduction and an update a distinct bin.  Wave-uniform control flow.
  __device__ __forceinline__ void hand_on(bool go) {
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
  // where `on`: a sample of bin `bin` that adds av and qv
  __device__ __forceinline__ void add(bool on, int bin, uint32_t av, unsigned long long qv) {
    bin = min(bin, kBins - 1);  // (a sample above the depth's maximum: the caller's error, not a wild index)
    const bool change = on && cur >= 0 && bin != cur;
    if (__builtin_amdgcn_ballot_w64(change)) hand_on(change);
    if (on) cur = bin, n += 1u, a += av, q += qv;
  }
  __device__ __forceinline__ void flush() { hand_on(cur >= 0); }
};

// The workgroup's frame around the strips of its waves: the waves' sums in LDS start at zero; at the end their sum is the
// workgroup's partial record, written with plain stores.
typedef unsigned long long WgSums[kWavesPerWg][kEntries];
__device__ __forceinline__ void wg_begin(WgSums &s_acc, int tid) {
  for (int i = tid; i < kWavesPerWg * kEntries; i += kStripThreads) (&s_acc[0][0])[i] = 0;
  __syncthreads();
}
template <class Job>
__device__ __forceinline__ void wg_end(const WgSums &s_acc, int tid, const NlfParams<Job> &p) {
  __syncthreads();
  if (tid < kEntries) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerWg; ++w) t += s_acc[w][tid];
    const size_t at = (size_t)blockIdx.z * p.wgs_frame + p.wg_base + (size_t)blockIdx.y * p.wgs_plane + blockIdx.x;
    p.partials[at * kEntries + tid] = t;
  }
}

// a frame's luma plane, and the row of it under chroma row y
struct LumaUnder {
  const uint8_t *luma;
  uint32_t stride;
  int ydec, H;
  template <class Job>
  __device__ __forceinline__ LumaUnder(const NlfJob &f, const NlfParams<Job> &p) : luma(f.p[0]), stride(f.stride[0]), ydec(p.ydec), H(p.H) {}
  __device__ __forceinline__ const uint8_t *row(int y) const { return luma + (size_t)min(y << ydec, H - 1) * stride; }
};

template <int BPS, int B, bool CHROMA>
__global__ __launch_bounds__(kStripThreads) void k_nlf(NlfParams<NlfJob> p) {
  __shared__ WgSums s_acc;
  constexpr int shift = B - 8, half = shift ? 1 << (shift - 1) : 0;
  const NlfJob &job = p.jobs[blockIdx.z];
  const int c = CHROMA ? 1 + (int)blockIdx.y : 0;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  wg_begin(s_acc, tid);
  const int strip = (int)blockIdx.x * kWavesPerWg + wave;
  if (strip < p.col_strips * p.row_strips) {  // (uniform in the wave)
    const StripCoords s = strip_coords(strip, p.col_strips, lane, p.ph);
    const int pw = p.pw;
    RowWindow<BPS> w;
    w.prime(job.p[c], job.stride[c], s.x0, pw, p.ph, s.y_first);
    const LumaUnder under(job, p);
    BinRun run(s_acc[wave], lane);
    for (int y = s.y_first; y < s.y_last; ++y) {
      w.load(y);
      int lum[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // chroma: the averageLuma of the lane's samples
      if (CHROMA) add_average_luma<BPS>(under.row(y), s.x0, p.W, p.xdec, s.out_lane, lum);
      w.fetch();
      each_of_word([&](auto K) __attribute__((always_inline)) {
        constexpr int k = decltype(K)::value;
        const Nine m = w.template at<k>();
        const int x = s.x0 + k, ga = stencil_gate(m, half, shift);
        const bool on = s.out_lane & (x >= 1) & (x < pw - 1) & (ga < kEdgeThreshold);  // (`&`: no branch a condition)
        const int bin = CHROMA ? lum[k] >> (B - 5) : stencil_box(m) / (9 << (B - 5));
        const uint32_t av = (uint32_t)abs(stencil_laplacian(m));
        run.add(on, bin, (av + (uint32_t)half) >> shift, (unsigned long long)(av * av));
      });
      w.rotate();
    }
    run.flush();
  }
  wg_end(s_acc, tid, p);
}

template <int BPS, int B, bool CHROMA>
__global__ __launch_bounds__(kStripThreads) void k_nlf_t(NlfParams<NlfTJob> p) {
  __shared__ WgSums s_acc;
  constexpr int shift = B - 8, half = shift ? 1 << (shift - 1) : 0;
  const NlfTJob &job = p.jobs[blockIdx.z];
  const int c = CHROMA ? 1 + (int)blockIdx.y : 0;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  wg_begin(s_acc, tid);
  const int strip = (int)blockIdx.x * kWavesPerWg + wave;
  if (strip < p.col_strips * p.row_strips) {  // (uniform in the wave)
    const StripCoords s = strip_coords(strip, p.col_strips, lane, p.ph);
    const int pw = p.pw;
    RowWindow<BPS> w, v;  // frame t, frame t - 1
    w.prime(job.now.p[c], job.now.stride[c], s.x0, pw, p.ph, s.y_first);
    v.prime(job.before.p[c], job.before.stride[c], s.x0, pw, p.ph, s.y_first);
    const LumaUnder under(job.now, p), under_before(job.before, p);
    BinRun run(s_acc[wave], lane);
    for (int y = s.y_first; y < s.y_last; ++y) {
      w.load(y);
      v.load(y);
      int lum2[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // chroma: a_t + a_(t-1) of the lane's samples
      if (CHROMA) {
        add_average_luma<BPS>(under.row(y), s.x0, p.W, p.xdec, s.out_lane, lum2);
        add_average_luma<BPS>(under_before.row(y), s.x0, p.W, p.xdec, s.out_lane, lum2);
      }
      w.fetch();
      v.fetch();
      each_of_word([&](auto K) __attribute__((always_inline)) {
        constexpr int k = decltype(K)::value;
        const Nine m = w.template at<k>(), o = v.template at<k>();
        const int x = s.x0 + k, ga = stencil_gate(m, half, shift), gb = stencil_gate(o, half, shift), s9 = stencil_box(m), t9 = stencil_box(o);
        const bool on = s.out_lane & (x >= 1) & (x < pw - 1) & (ga < kEdgeThreshold) & (gb < kEdgeThreshold) & (abs(s9 - t9) < (kBoxGate << shift));
        const int bin = CHROMA ? lum2[k] >> (B - 4) : (s9 + t9) / (18 << (B - 5));
        const int e = m.m11 - o.m11;
        run.add(on, bin, (uint32_t)e, (unsigned long long)(uint32_t)(e * e));
      });
      w.rotate();
      v.rotate();
    }
    run.flush();
  }
  wg_end(s_acc, tid, p);
}

// the kernel of a job type at <BPS, B, CHROMA>
template <int BPS, int B, bool CHROMA>
auto strip_kernel(const NlfParams<NlfJob> &) { return &k_nlf<BPS, B, CHROMA>; }
template <int BPS, int B, bool CHROMA>
auto strip_kernel(const NlfParams<NlfTJob> &) { return &k_nlf_t<BPS, B, CHROMA>; }

// the frame's record from its workgroups' partial records: grid (plane, frame); a plane without workgroups gets zeros
__global__ __launch_bounds__(128 * kTailGroups) void k_nlf_tail(TailParams p) {
  __shared__ unsigned long long s_sum[kTailGroups][128];
  const int c = (int)blockIdx.x, i = (int)threadIdx.x & 127, g = (int)threadIdx.x >> 7;
  const unsigned long long *src = p.partials + ((size_t)blockIdx.y * p.units_frame + p.unit_base[c]) * kEntries;
  unsigned long long t = 0;
  if (i < kEntries)
    for (uint32_t k = (uint32_t)g; k < p.units[c]; k += kTailGroups) t += src[(size_t)k * kEntries + i];
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

// What the meter keeps per kind of record: frames (NlfJob, g1s_nlf_record_t, k_nlf) and pairs (NlfTJob, g1s_nlf_trecord_t,
// k_nlf_t): a RecordLane (meter_op.h) with its queued jobs, timed as two intervals, luma and chroma.  A batch of either goes
// through g1s_nlf::run.
template <class Job, class Record>
struct Kind : RecordLane<Record, 2> {
  JobQueue<Job> queue;
  bool alloc(uint32_t B) { return !this->on || (queue.alloc(B) && RecordLane<Record, 2>::alloc(B)); }
};

struct g1s_nlf : BatchedOp {
  Kind<NlfJob, g1s_nlf_record_t> frames;
  int col_strips[2] = {0, 0}, row_strips[2] = {0, 0};  // per plane class: luma, chroma
  Units wgs;                                           // the workgroups of a frame's planes
  // A temporal meter (rules T1 - T5; pairs.on) pairs every frame of a run but the first with the frame before.  Host
  // frames then go round the ring, which moves on with every frame that is not the caller's; of a caller's device frame that
  // is a batch's last the flush keeps a copy.
  Kind<NlfTJob, g1s_nlf_trecord_t> pairs;
  NlfJob prev{};  // the frame before: where its planes are read
  FrameBefore<1> before;
  // A lag meter (rules L1 - L5; lags.on) is a temporal meter that also keeps a lag record a pair: the pairs' queued jobs go
  // through the two lag launches (nlf_lags.hip) behind k_nlf_t's, into a lane of their own.
  RecordLane<g1s_nlf_lrecord_t, 2> lags;
  Units lag_tiles;

  int set_geometry(const g1s_frame_t &f);
  int flush();
  int settle() { return flush(); }
  template <class K>
  int run(K &k, int set);
  int run_lags(int set);
  template <class K>
  int collect(K &k);
  template <bool CHROMA, class Params>
  void launch(const Params &np, dim3 grid);
};

int g1s_nlf::set_geometry(const g1s_frame_t &f) {
  set_frame_geometry(f);
  for (int c = 0; c < 3; ++c) {
    const int cls = c ? 1 : 0;
    const long pw = c < geom.nplanes ? (long)geom.pw(c) : 0, ph = c < geom.nplanes ? (long)geom.ph(c) : 0;
    // a plane without interior samples (a side shorter than 3) launches nothing
    const bool any = pw >= 3 && ph >= 3;
    col_strips[cls] = any ? (int)((pw - 1 + kColsPerWave - 1) / kColsPerWave) : 0;
    row_strips[cls] = any ? (int)((ph - 2 + kStripRows - 1) / kStripRows) : 0;
    wgs.n[c] = (uint32_t)((col_strips[cls] * (long)row_strips[cls] + kWavesPerWg - 1) / kWavesPerWg);
  }
  wgs.lay();
  const size_t need = (size_t)wgs.frame * kEntries * batch;
  G1S_OP_TRY(frames.size_partials(need));
  G1S_OP_TRY(pairs.size_partials(need));
  g1s_nlf_lags::cut(geom, lag_tiles);
  G1S_OP_TRY(lags.size_partials((size_t)lag_tiles.frame * g1s_nlf_lags::kEntries * batch));
  before.reset();
  return G1S_OK;
}

template <bool CHROMA, class Params>
void g1s_nlf::launch(const Params &np, dim3 grid) {
  const auto kernel = bit_depth == 8 ? strip_kernel<1, 8, CHROMA>(np) : bit_depth == 10 ? strip_kernel<2, 10, CHROMA>(np) : strip_kernel<2, 12, CHROMA>(np);
  hipLaunchKernelGGL(kernel, grid, dim3(kStripThreads), 0, stream, np);
}

// the kind's queued jobs as one batch on the stream: the jobs up, a launch per plane class between the lane's three events,
// the summing launch (which writes every word of a record: no zeros in front), the records back
template <class K>
int g1s_nlf::run(K &k, int set) {
  const uint32_t B = (uint32_t)k.queue.jobs.size();
  if (!B) return G1S_OK;
  G1S_OP_TRY(k.queue.upload(set, stream));
  NlfParams<typename decltype(k.queue.jobs)::value_type> np{};
  np.jobs = k.queue.sets.d[set], np.partials = k.d_partials;
  np.W = geom.W, np.H = geom.H, np.xdec = geom.subx, np.ydec = geom.suby, np.wgs_frame = wgs.frame;
  G1S_OP_TRY(k.mark(0, timing, stream));
  if (wgs.n[0]) {
    np.pw = geom.W, np.ph = geom.H, np.col_strips = col_strips[0], np.row_strips = row_strips[0];
    np.wg_base = wgs.base[0], np.wgs_plane = wgs.n[0];
    launch<false>(np, dim3(wgs.n[0], 1u, B));
    G1S_OP_TRY(hipGetLastError());
  }
  G1S_OP_TRY(k.mark(1, timing, stream));
  if (wgs.n[1]) {
    np.pw = (int)geom.pw(1), np.ph = (int)geom.ph(1), np.col_strips = col_strips[1], np.row_strips = row_strips[1];
    np.wg_base = wgs.base[1], np.wgs_plane = wgs.n[1];
    launch<true>(np, dim3(wgs.n[1], 2u, B));
    G1S_OP_TRY(hipGetLastError());
  }
  G1S_OP_TRY(k.mark(2, timing, stream));
  G1S_OP_TRY(k.sum(k_nlf_tail, 3u, B, 128 * kTailGroups, wgs, stream));
  G1S_OP_TRY(k.copy_back(B, stream));
  return G1S_OK;
}

// the pairs that run(pairs, set) sent up, through the lag launches: luma and chroma between the lane's three events, the
// summing launch (which writes every word of a record), the records back
int g1s_nlf::run_lags(int set) {
  const uint32_t B = (uint32_t)pairs.queue.jobs.size();
  if (!B) return G1S_OK;
  const NlfTJob *jobs = pairs.queue.sets.d[set];
  G1S_OP_TRY(lags.mark(0, timing, stream));
  G1S_OP_TRY(g1s_nlf_lags::launch(false, jobs, B, lags.d_partials, geom, lag_tiles, bit_depth, stream));
  G1S_OP_TRY(lags.mark(1, timing, stream));
  G1S_OP_TRY(g1s_nlf_lags::launch(true, jobs, B, lags.d_partials, geom, lag_tiles, bit_depth, stream));
  G1S_OP_TRY(lags.mark(2, timing, stream));
  G1S_OP_TRY(lags.sum(g1s_nlf_lags::tail(), 3u, B, g1s_nlf_lags::kTailThreads, lag_tiles, stream));
  G1S_OP_TRY(lags.copy_back(B, stream));
  return G1S_OK;
}

// once the stream is through: the batch's times and records, the queue empty again
template <class K>
int g1s_nlf::collect(K &k) {
  const uint32_t B = (uint32_t)k.queue.jobs.size();
  if (timing && B) G1S_OP_TRY(k.clock(B));
  k.collect(B);
  k.queue.jobs.clear();
  return G1S_OK;
}

// the queued frames as one batch, behind them the queued pairs and, where the last frame's planes are the caller's, the copy
// of it, all waited for
int g1s_nlf::flush() {
  if (frames.queue.jobs.empty()) return G1S_OK;
  int set, rc = next_set(&set);
  if (rc) return rc;
  if ((rc = run(frames, set)) != 0) return rc;
  if (pairs.on) {
    if ((rc = run(pairs, set)) != 0) return rc;
    if (lags.on && (rc = run_lags(set)) != 0) return rc;
    G1S_OP_TRY(before.room(0, stage));
    G1S_OP_TRY(before.keep(0, geom, stage, prev.p, prev.stride, stream));
  }
  if ((rc = set_done(set)) != 0 || (rc = wait()) != 0) return rc;
  if ((rc = collect(frames)) != 0) return rc;
  if (lags.on) {
    const uint32_t B = (uint32_t)pairs.queue.jobs.size();
    if (timing && B) G1S_OP_TRY(lags.clock(B));
    lags.collect(B);
  }
  return collect(pairs);
}

namespace {

g1s_nlf_t *nlf_new(uint32_t bit_depth, const g1s_nlf_opts_t *opts, bool temporal, bool lags = false) {
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return refuse_new("noise levels are defined for bit depths 8, 10 and 12");
  return new_op<g1s_nlf>("noise levels", opts, "g1s_nlf_opts_t", bit_depth, [&](g1s_nlf &m, std::string &) {
    m.frames.on = true, m.pairs.on = temporal, m.lags.on = lags;
    return m.frames.alloc(m.batch) && m.pairs.alloc(m.batch) && m.lags.alloc(m.batch);
  });
}

}  // namespace

extern "C" {

g1s_nlf_t *g1s_nlf_new(uint32_t bit_depth, const g1s_nlf_opts_t *opts) { return nlf_new(bit_depth, opts, false); }

g1s_nlf_t *g1s_nlf_new_temporal(uint32_t bit_depth, const g1s_nlf_opts_t *opts) { return nlf_new(bit_depth, opts, true); }

g1s_nlf_t *g1s_nlf_new_lags(uint32_t bit_depth, const g1s_nlf_opts_t *opts) { return nlf_new(bit_depth, opts, true, true); }

int g1s_nlf_cut(g1s_nlf_t *m) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  m->before.have = false;
  return G1S_OK;
}

int g1s_nlf_frame(g1s_nlf_t *m, const g1s_frame_t *f) {
  if (!m || !f) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  (void)hipSetDevice(m->device);
  const Refusal no = check_frame_pair(*f, *f, m->bps, 65536u, "g1s_nlf_new",
                                      "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)");
  if (no.code) return m->fail(no.code, no.text);
  int rc = take_shape(*m, *f);
  if (rc) return rc;
  NlfJob job{};
  // (a temporal meter: the ring has a slot more than a batch, and the slots go round)
  const bool temporal = m->pairs.on;
  const uint32_t slots = temporal ? m->before.slots(m->batch) : m->batch, slot = temporal ? m->before.next_slot : (uint32_t)m->frames.queue.jobs.size();
  if ((rc = m->stage_in(*f, slot, slots, job.p, job.stride)) != 0) return rc;
  if ((rc = m->wait_host_input(*f)) != 0) return rc;
  m->frames.queue.jobs.push_back(job);
  if (temporal) {
    if (f->on_device != 1) m->before.advance(m->batch);
    if (m->before.have) m->pairs.queue.jobs.push_back(NlfTJob{job, m->prev});
    m->prev = job, m->before.have = true, m->before.callers[0] = f->on_device == 1;
  }
  return m->frames.queue.jobs.size() >= m->batch ? m->flush() : G1S_OK;
}

int g1s_nlf_finish(g1s_nlf_t *m, g1s_nlf_record_t *per_frame, size_t cap, size_t *n_out) {
  return finish_kind(m, &g1s_nlf::frames, kAlwaysMade, per_frame, cap, n_out);
}

int g1s_nlf_finish_temporal(g1s_nlf_t *m, g1s_nlf_trecord_t *per_pair, size_t cap, size_t *n_out) {
  return finish_kind(m, &g1s_nlf::pairs, "not a temporal meter: make it with g1s_nlf_new_temporal", per_pair, cap, n_out);
}

int g1s_nlf_temporal_times(g1s_nlf_t *m, double *ms_luma, double *ms_chroma, uint64_t *pairs) {
  return m ? m->pairs.times(ms_luma, ms_chroma, pairs) : G1S_ERR_INVALID;
}

int g1s_nlf_finish_lags(g1s_nlf_t *m, g1s_nlf_lrecord_t *per_pair, size_t cap, size_t *n_out) {
  return finish_kind(m, &g1s_nlf::lags, "not a lag meter: make it with g1s_nlf_new_lags", per_pair, cap, n_out);
}

int g1s_nlf_lag_times(g1s_nlf_t *m, double *ms_luma, double *ms_chroma, uint64_t *pairs) {
  return m ? m->lags.times(ms_luma, ms_chroma, pairs) : G1S_ERR_INVALID;
}

int g1s_nlf_set_timing(g1s_nlf_t *m, int enable, double *ms_luma, double *ms_chroma, uint64_t *frames) {
  if (!m) return G1S_ERR_INVALID;
  m->timing = enable != 0;
  return m->frames.times(ms_luma, ms_chroma, frames);
}

const char *g1s_nlf_last_error(const g1s_nlf_t *m) { return m ? m->err.c_str() : ""; }

void g1s_nlf_free(g1s_nlf_t *m) { free_op(m); }

}  // extern "C"
