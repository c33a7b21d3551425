// denoise.hip -- `denoise`: the project's integer-exact non-local-means filter on the device.
//
// The filter is defined in include/g1s_diff.h ("denoise", rules 1 - 4); tests/denoise_ref.py restates it in numpy.  It is
// this project's own definition of non-local means: ffmpeg's nlmeans and KNLMeansCL have the same structure, not the
// same bits.  One filter kernel, kd_nlm<Form, S, BPS>, a workgroup per (tile, plane of the class, frame), the phases of
// denoise_tile.hip.h: Form::kPlain is one frame on its own (temporal radius 0, rules 1 - 4), Form::kTemporal goes on over the
// frames around it (rules 5 - 7), Form::kMotion reads them where kd_motion's vectors point (rules 16 - 20).  A batch of frames
// goes out as one launch per plane class (luma; the two chroma planes) on the denoiser's own stream.  Under
// G1S_DENOISE_JOINT_CHROMA (rules 8 - 11) the chroma launch is kd_nlm_j<Form, S, BPS> instead: a workgroup per (chroma tile,
// frame) that filters both chroma planes with one weight; with a chroma gain (rules 21 - 24) kd_nlm_j<Form, S, BPS, GainArg>.
// Planes are independent (under the flag the chroma launch also reads the luma input), but `out` must not overlap `in`: a
// tile reads the halo its neighbours write.
//
// The engine numbers the frames handed over since the denoiser was made.  With temporal radius D a frame is launched once
// the D frames after it are there (or the clip ends), so the queue holds the frames not yet launched and, in front of
// them, the last D that were: their planes are the neighbours of what comes next.
//
// This file: the kernels, the engine and the per-frame ABI.  The file commands are denoise_file.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/g1s_diff.h"
#include "curve.h"
#include "curve_row.hip.h"
#include "denoise_tile.hip.h"
#include "frame_op.h"
#include "levels_row.hip.h"

namespace {

using namespace g1s_dn;

constexpr int kMaxLevels = 2;  // coarse levels (rule 28)

struct DenoiseJob {
  const uint8_t *in[3];
  uint8_t *out[3];
  uint32_t in_stride[3], out_stride[3];  // bytes
};

// the temporal kernels' job: the frame and, per plane, the 2 D frames around it (null: the clip has no such frame)
struct DenoiseJobT {
  DenoiseJob f;
  const uint8_t *nb[3][2 * kMaxD];
  uint32_t nb_stride[3][2 * kMaxD];
};

// the same under motion (rules 16 - 20): the frame's vectors, per plane [2 D][blocks of the plane] pairs of int8 (mx, my);
// kd_motion writes them, the filter kernels of Form::kMotion read them.  Under the joint flag mv[2] is mv[1].
struct DenoiseJobTM {
  DenoiseJobT t;
  int8_t *mv[3];
};

// a job begins with the job of the form before it: the host fills the widest and uploads the part a form's kernels index
static_assert(std::is_standard_layout<DenoiseJob>::value && std::is_standard_layout<DenoiseJobT>::value && std::is_standard_layout<DenoiseJobTM>::value,
              "the jobs are copied as bytes");
static_assert(offsetof(DenoiseJobT, f) == 0 && offsetof(DenoiseJobTM, t) == 0, "a job is a prefix of the next form's");

// what a filter kernel does beyond one frame on its own (rules 1 - 4): the frames around it (rules 5 - 7), those where
// their tiles' vectors point (rules 16 - 20).  The form picks the job: jobs[] is indexed with the form's own stride.
enum class Form { kPlain, kTemporal, kMotion };
template <Form F>
using JobOf = std::conditional_t<F == Form::kPlain, DenoiseJob, std::conditional_t<F == Form::kTemporal, DenoiseJobT, DenoiseJobTM>>;

__device__ inline const DenoiseJob &frame_of(const DenoiseJob &j) { return j; }
__device__ inline const DenoiseJob &frame_of(const DenoiseJobT &j) { return j.f; }
__device__ inline const DenoiseJob &frame_of(const DenoiseJobTM &j) { return j.t.f; }
__device__ inline const DenoiseJobT &around_of(const DenoiseJobT &j) { return j; }
__device__ inline const DenoiseJobT &around_of(const DenoiseJobTM &j) { return j.t; }

// the planes of a class, one at a time (kd_nlm).  nnb and blocks are read by the forms that have them.
template <class Job>
struct PlaneParams {
  const Job *jobs;
  const uint16_t *table;  // the class's 1024 weights
  int q, A;
  int W, H, tiles_x;  // the class's plane size
  int plane0;         // first plane of the class: 0 luma, 1 chroma
  int nnb;            // 2 D
  int blocks;         // tiles of the class's plane
};

// the two chroma planes with one weight (kd_nlm_j)
template <class Job>
struct JointParams {
  const Job *jobs;
  const uint16_t *table;  // rule 10's 1024 weights
  int q, A;
  JointShape s;
  int tiles_x;
  int nnb;
  int blocks;
};

// a workgroup per (block, plane of the class or joint chroma pair, frame and neighbour): the block's vector towards that neighbour
struct MotionParams {
  const DenoiseJobTM *jobs;
  int M;
  int W, H, tiles_x;  // the class's plane size
  int plane0;
  int nnb;
  int blocks;
};

template <int BPS, int NA>
__global__ __launch_bounds__(kThreads) void kd_motion(MotionParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dn_lds[];
  const int f = (int)blockIdx.z / p.nnb, k = (int)blockIdx.z - f * p.nnb;
  const DenoiseJobTM &job = p.jobs[f];
  const int c = p.plane0 + (int)blockIdx.y;
  int8_t *mv = job.mv[c] + 2 * (k * p.blocks + (int)blockIdx.x);
  if (!job.t.nb[c][k]) {  // rule 5: the clip has no such frame (the same for the whole workgroup)
    if (threadIdx.x == 0) mv[0] = 0, mv[1] = 0;
    return;
  }
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
  MotionPlanes cur, ref;
#pragma unroll
  for (int a = 0; a < NA; ++a)
    cur.p[a] = job.t.f.in[c + a], cur.stride[a] = job.t.f.in_stride[c + a], ref.p[a] = job.t.nb[c + a][k], ref.stride[a] = job.t.nb_stride[c + a][k];
  dn_motion_tile<BPS, NA>((int)threadIdx.x, motion_geom(p.M, NA), dn_lds, cur, ref, p.W, p.H, tx, ty, [] { __syncthreads(); }, mv);
}

// a workgroup per (tile, plane of the class, frame)
template <Form F, int S, int BPS>
__global__ __launch_bounds__(kThreads) void kd_nlm(PlaneParams<JobOf<F>> p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dn_lds[];
  const JobOf<F> &job = p.jobs[blockIdx.z];
  const DenoiseJob &f = frame_of(job);
  const int c = p.plane0 + (int)blockIdx.y;
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
  const TileGeom g = tile_geom(p.A, S);
  if constexpr (F == Form::kPlain) {
    dn_tile<S, BPS>((int)threadIdx.x, g, dn_lds, p.table, p.q, f.in[c], f.in_stride[c], f.out[c], f.out_stride[c], p.W, p.H, tx * kTW, ty * kTH,
                    [] { __syncthreads(); });
  } else if constexpr (F == Form::kTemporal) {
    dn_tile_t<S, BPS>((int)threadIdx.x, g, dn_lds, p.table, p.q, f.in[c], f.in_stride[c], job.nb[c], job.nb_stride[c], p.nnb, f.out[c], f.out_stride[c], p.W,
                      p.H, tx * kTW, ty * kTH, [] { __syncthreads(); });
  } else {
    dn_tile_tm<S, BPS>((int)threadIdx.x, g, dn_lds, p.table, p.q, f.in[c], f.in_stride[c], job.t.nb[c], job.t.nb_stride[c], p.nnb,
                       job.mv[c] + 2 * (int)blockIdx.x, 2 * p.blocks, f.out[c], f.out_stride[c], p.W, p.H, tx * kTW, ty * kTH, [] { __syncthreads(); });
  }
}

// the joint chroma kernels (rules 8 - 11t): a workgroup per (chroma tile, frame) filters Cb and Cr with one weight.  Under a
// chroma gain (rules 21 - 24) the kernel takes a second argument: the same tiles in the gain's layout, the weight of a pair
// scaled by the gain at the guide under both of its ends.
struct GainArg {
  const uint16_t *table;  // m[256]
  int shift;              // B - 8
};

__device__ inline JointPlanes joint_planes(const DenoiseJob &f) { return JointPlanes{f.in[1], f.in[2], f.in[0], f.in_stride[1], f.in_stride[2], f.in_stride[0]}; }

template <class... G>
__device__ inline auto joint_layout(const TileGeom &g) {
  if constexpr (sizeof...(G) != 0) return joint_gain_geom(g);
  else return joint_geom(g);
}

template <Form F, int S, int BPS, class... G>  // G: nothing, or GainArg
__global__ __launch_bounds__(kThreads) void kd_nlm_j(JointParams<JobOf<F>> p, G... ga) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dn_lds[];
  const JobOf<F> &job = p.jobs[blockIdx.z];
  const DenoiseJob &f = frame_of(job);
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
  const TileGeom g = tile_geom(p.A, S);
  if constexpr (F == Form::kPlain) {
    dn_tile_j<S, BPS>((int)threadIdx.x, g, joint_layout<G...>(g), dn_lds, p.table, p.q, joint_planes(f), p.s, f.out[1], f.out_stride[1], f.out[2],
                      f.out_stride[2], tx * kTW, ty * kTH, [] { __syncthreads(); }, Gain{ga.table, ga.shift}...);
  } else {
    const DenoiseJobT &t = around_of(job);
    auto nb = [&t](int k) { return JointPlanes{t.nb[1][k], t.nb[2][k], t.nb[0][k], t.nb_stride[1][k], t.nb_stride[2][k], t.nb_stride[0][k]}; };
    if constexpr (F == Form::kTemporal) {
      dn_tile_jt<S, BPS>((int)threadIdx.x, g, joint_layout<G...>(g), dn_lds, p.table, p.q, joint_planes(f), nb, p.nnb, p.s, f.out[1], f.out_stride[1],
                         f.out[2], f.out_stride[2], tx * kTW, ty * kTH, [] { __syncthreads(); }, Gain{ga.table, ga.shift}...);
    } else {
      dn_tile_jtm<S, BPS>((int)threadIdx.x, g, joint_layout<G...>(g), dn_lds, p.table, p.q, joint_planes(f), nb, p.nnb, job.mv[1] + 2 * (int)blockIdx.x,
                          2 * p.blocks, p.s, f.out[1], f.out_stride[1], f.out[2], f.out_stride[2], tx * kTW, ty * kTH, [] { __syncthreads(); },
                          Gain{ga.table, ga.shift}...);
    }
  }
}

// the kernel families as the host launches them: the arguments each takes and its instantiation for (S, BPS)
template <Form F>
struct Planes {
  template <int S, int BPS> static void launch(dim3 grid, size_t lds, hipStream_t st, const PlaneParams<JobOf<F>> &p) {
    hipLaunchKernelGGL((kd_nlm<F, S, BPS>), grid, dim3(kThreads), lds, st, p);
  }
};
template <Form F, class... G>
struct Joint {
  template <int S, int BPS> static void launch(dim3 grid, size_t lds, hipStream_t st, const JointParams<JobOf<F>> &p, const G &...ga) {
    hipLaunchKernelGGL((kd_nlm_j<F, S, BPS, G...>), grid, dim3(kThreads), lds, st, p, ga...);
  }
};

// the family's kernel for patch radius S and `bps` bytes a sample; false: there is none
template <class Family, class... Args>
bool launch_family(uint32_t S, uint32_t bps, dim3 grid, size_t lds, hipStream_t st, const Args &...args) {
  switch (S * 2 + (bps - 1)) {
#define DN_CASE(s)                                                                   \
  case (s) * 2: Family::template launch<s, 1>(grid, lds, st, args...); return true; \
  case (s) * 2 + 1: Family::template launch<s, 2>(grid, lds, st, args...); return true;
    DN_CASE(1)
    DN_CASE(2)
    DN_CASE(3)
    DN_CASE(4)
#undef DN_CASE
  }
  return false;
}

// G1S_OP_TRY outside a member: the operation is `g`
#define G1S_OP_TRY_(g, expr)                                                                                       \
  do {                                                                                                             \
    hipError_t e_ = (expr);                                                                                        \
    if (e_ != hipSuccess) return (g)->fail(G1S_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
  } while (0)

// rule 3's bound on a strength and its text, and the strengths of level 0 as the opts give them (a zero field, or no opts: the
// default): the one place either is said -- make_table, rule 28's levels and the commands' early look at them ask here
constexpr const char *kStrengthBound = "strength must be greater than 0 and at most 1000";
inline bool strength_ok(double h) { return h > 0.0 && h <= 1000.0; }
struct Strengths {
  double h, hc;
};
inline Strengths strengths_of(const g1s_denoise_opts_t *opts) {
  const double h = opts && opts->strength != 0.0 ? opts->strength : 4.0;
  return {h, opts && opts->chroma_strength != 0.0 ? opts->chroma_strength : h};
}

// rule 3, for patches of `planes` planes (rule 10: 3).  "" when fine.
std::string make_table(uint32_t bit_depth, uint32_t S, double h, uint16_t T[kTable], uint32_t *q_out, uint32_t planes = 1) {
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return "denoise is defined for bit depths 8, 10 and 12";
  if (S < 1 || S > (uint32_t)kMaxS) return "patch_radius must be 1..4";
  if (!strength_ok(h)) return kStrengthBound;
  const double n = (double)(planes * (2 * S + 1) * (2 * S + 1)), den = n * h * h * std::pow(4.0, (double)bit_depth - 8.0);
  auto entry = [&](int i, uint32_t q) { return std::floor(4096.0 * std::exp(-(((double)i + 0.5) * std::ldexp(1.0, (int)q)) / den) + 0.5); };
  uint32_t q = 0;
  while (entry(kTable - 1, q) != 0.0) ++q;
  T[0] = 4096;
  for (int i = 1; i < kTable; ++i) T[i] = (uint16_t)std::min(entry(i, q), (double)T[i - 1]);
  *q_out = q;
  return "";
}

}  // namespace

// =============================================================== host engine =====
using namespace g1s_op;

// (the stream, the sticky error, the parameter sets' turn and the staging of host frames: BatchedOp, frame_op.h)
struct g1s_denoise : BatchedOp {
  uint32_t A = 3, S = 2, D = 0;
  uint32_t M = 0;  // the motion range on the search plane (rules 16 - 20); 0: no motion, the launches of rules 1 - 15
  bool joint = false;         // G1S_DENOISE_JOINT_CHROMA: frames of three planes get kd_nlm_j for their chroma
  bool gain = false;          // a chroma gain (rules 21 - 24): the joint launch is kd_nlm_j<.., GainArg>
  DevBuf<uint16_t> d_gain;    // m[256]
  uint32_t q[4] = {0, 0, 0, 0};  // luma, chroma, joint chroma, luma in the stabilised domain
  Event ev[3];
  // a frame handed over: its planes on the device (the caller's, or a slot of the input staging ring) and where its
  // output goes (out[c] is null for a host frame: a slot of the output staging buffer is chosen at the launch)
  struct Queued {
    const uint8_t *in[3];
    uint8_t *out[3];
    uint32_t in_stride[3], out_stride[3];
    bool host_out;
    HostPlanes host;
  };
  // frames [first_queued, frames_in): what is not launched yet and, in front of it, up to D launched frames of the same clip
  std::deque<Queued> queue;
  uint64_t frames_in = 0, first_queued = 0, next_launch = 0, clip_first = 0, frames_complete = 0;
  ParamSets<uint8_t> p_jobs;  // the form's jobs: JobOf<Form>
  DevBuf<uint16_t> d_tables;  // [4][1024]
  // a grain prior's curve (rules 12 - 15): luma goes forward into a ring of 12-bit u16 planes, one slot a frame of the
  // input ring, is filtered there into `batch` planes and comes back through the inverse
  bool curve = false;
  DevBuf<uint16_t> d_curve;  // fwd[1 << B], inv[4096]
  DevBuf<uint8_t> d_stab, d_filt;
  size_t stab_row = 0, stab_plane = 0;
  uint64_t next_stab = 0;  // the first frame whose luma is not in its slot yet
  double ms_kernel = 0, ms_motion = 0;
  uint64_t frames_timed = 0;
  // under motion: a set's vectors, a frame after the other: per plane [2 D][blocks of the plane] pairs of int8
  DevBuf<int8_t> d_mv[2];
  size_t mv_off[3] = {0, 0, 0}, mv_frame = 0;
  int blocks_of(const PlaneGeom &pg, int c) const { return (int)((pg.pw(c) + kTW - 1) / kTW * ((pg.ph(c) + kTH - 1) / kTH)); }
  // where plane c's vectors start in a frame's; under the joint flag the chroma planes share plane 1's.  Returns a frame's bytes.
  size_t mv_layout(const PlaneGeom &pg, uint32_t nnb, size_t off[3]) const {
    size_t at = 0;
    for (int c = 0; c < pg.nplanes; ++c) {
      if (c == 2 && joint) {
        off[2] = off[1];
        continue;
      }
      off[c] = at, at += align_up((size_t)2 * nnb * (size_t)blocks_of(pg, c), 16);
    }
    return at;
  }
  // coarse levels (rules 25 - 29): level K - 1 is a whole denoiser on the coarse frames, made by new_denoiser with the scaled
  // strengths and the halved motion range, on this denoiser's stream.  Its frames are device frames in three rings for the
  // geometry in hand: coarse inputs (a slot a frame of the input ring), coarse outputs and d (a slot a frame of a batch).
  uint32_t K = 0;
  g1s_denoise *inner = nullptr;
  bool borrowed_stream = false;  // an inner level's stream is its owner's
  PlaneGeom cgeom;               // the coarse frame (rule 25)
  Layout clay, dlay;             // a coarse frame; its d: the same planes as int16
  DevBuf<uint8_t> d_cin, d_cout, d_d;
  ParamSets<uint8_t> p_level;    // a set: the kd_down jobs (batch + D), then the merge's (batch)
  uint64_t next_coarse = 0;      // the first frame whose coarse frame is not made and handed to the inner level yet
  double ms_level = 0, ms_level_k = 0;  // of the timed batches: the three kernels and the inner level; the three kernels alone
  Event evl[5];
  size_t off_merge() const { return sizeof(g1s_lv::LevelJob) * (batch + D); }
  size_t level_bytes() const { return off_merge() + sizeof(g1s_lv::LevelJob) * batch; }
  int need_levels();
  int coarse_level(int set, uint32_t nframes, uint32_t ndown, uint64_t first_down);
  int merge(int set, uint32_t nframes);
  ~g1s_denoise() {
    delete inner;
    if (borrowed_stream) stream.p = nullptr;
  }
  int need_mv();
  int launch_motion(const DenoiseJobTM *jobs, const PlaneGeom &pg, uint32_t nframes, uint32_t nnb, int plane0, uint32_t bps_, hipStream_t st);

  // the form of this denoiser's filter kernels, as a tag: the one place the choice among them is made
  template <class Fn>
  auto with_form(Fn &&fn) const {
    if (D && M) return fn(std::integral_constant<Form, Form::kMotion>());
    if (D) return fn(std::integral_constant<Form, Form::kTemporal>());
    return fn(std::integral_constant<Form, Form::kPlain>());
  }
  size_t job_bytes() const { return with_form([](auto form) { return sizeof(JobOf<decltype(form)::value>); }); }
  // a parameter set: the batch's jobs and, with a curve, the luma launch's jobs in the stabilised planes, the forward
  // launch's (a first batch brings its D later neighbours along) and the inverse launch's
  size_t off_luma() const { return align_up(job_bytes() * batch, 16); }
  size_t off_fwd() const { return 2 * off_luma(); }
  size_t off_inv() const { return off_fwd() + align_up(sizeof(g1s_cv::CurveJob) * (batch + D), 16); }
  size_t set_bytes() const { return curve ? off_inv() + sizeof(g1s_cv::CurveJob) * batch : job_bytes() * batch; }
  uint8_t *stab_slot(uint64_t n) const { return d_stab + stab_plane * (size_t)(n % ring()); }
  int need_stab();
  // host and pinned inputs wait on the device in a ring: a slot is written again B + 2D frames later, and by then every
  // frame that reads it (up to D frames on) has been launched in front of that copy on the stream
  uint32_t ring() const { return batch + 2 * D; }
  const Queued &frame(uint64_t n) const { return queue[(size_t)(n - first_queued)]; }
  int launch(int set, uint32_t nframes, int plane0, int nplanes_in_class, bool stabilised = false);
  int launch_joint(int set, uint32_t nframes);
  int flush(uint32_t nframes);
  int launch_up_to(uint64_t limit);
  int end_clip();
};

// the planes of a class through kd_nlm; `stabilised`: luma as the forward curve left it -- 12-bit u16 planes,
// the jobs that point into them and rule 14's table
int g1s_denoise::launch(int set, uint32_t nframes, int plane0, int nplanes_in_class, bool stabilised) {
  const int W = (int)geom.pw(plane0), H = (int)geom.ph(plane0), tiles_x = (W + kTW - 1) / kTW;
  const int ti = stabilised ? 3 : plane0 ? 1 : 0;
  const uint32_t bps = stabilised ? 2u : this->bps;
  const dim3 grid((unsigned)(tiles_x * ((H + kTH - 1) / kTH)), (unsigned)nplanes_in_class, nframes);
  const TileGeom tg = tile_geom((int)A, (int)S);
  const bool found = with_form([&](auto form) {
    constexpr Form F = decltype(form)::value;
    PlaneParams<JobOf<F>> p{};
    p.jobs = reinterpret_cast<const JobOf<F> *>(p_jobs.d[set].p + (stabilised ? off_luma() : 0)), p.table = d_tables + ti * kTable, p.q = (int)q[ti], p.A = (int)A;
    p.W = W, p.H = H, p.tiles_x = tiles_x, p.plane0 = plane0, p.nnb = (int)(2 * D), p.blocks = (int)grid.x;
    return launch_family<Planes<F>>(S, bps, grid, (size_t)(F == Form::kPlain ? tg.bytes : tg.bytes_t), stream, p);
  });
  if (!found) return fail(G1S_ERR_INVALID, "no kernel for this patch radius");
  G1S_OP_TRY(hipGetLastError());
  return G1S_OK;
}

// both chroma planes of the batch's frames through the joint kernel: grid (tiles, 1, frames)
int g1s_denoise::launch_joint(int set, uint32_t nframes) {
  const int cw = (int)geom.pw(1), ch = (int)geom.ph(1), tiles_x = (cw + kTW - 1) / kTW;
  const dim3 grid((unsigned)(tiles_x * ((ch + kTH - 1) / kTH)), 1u, nframes);
  const TileGeom tg = tile_geom((int)A, (int)S);
  const JointGeom jg = gain ? joint_gain_geom(tg) : joint_geom(tg);  // (the gain's layout: the same fields, Mt between T and N)
  const GainArg ga{d_gain, (int)bit_depth - 8};
  const bool found = with_form([&](auto form) {
    constexpr Form F = decltype(form)::value;
    JointParams<JobOf<F>> p{};
    p.jobs = reinterpret_cast<const JobOf<F> *>(p_jobs.d[set].p), p.table = d_tables + 2 * kTable, p.q = (int)q[2], p.A = (int)A;
    p.s = JointShape{geom.W, geom.H, geom.subx, geom.suby, cw, ch}, p.tiles_x = tiles_x, p.nnb = (int)(2 * D), p.blocks = (int)grid.x;
    const size_t lds = (size_t)(F == Form::kPlain ? jg.bytes : jg.bytes_t);
    return gain ? launch_family<Joint<F, GainArg>>(S, bps, grid, lds, stream, p, ga) : launch_family<Joint<F>>(S, bps, grid, lds, stream, p);
  });
  if (!found) return fail(G1S_ERR_INVALID, "no kernel for this patch radius");
  G1S_OP_TRY(hipGetLastError());
  return G1S_OK;
}

// the ring of stabilised luma planes and the planes the luma launch writes, for the geometry in hand
int g1s_denoise::need_stab() {
  if (d_stab) return G1S_OK;
  stab_row = align_up((size_t)geom.W * 2, kStageRowAlign), stab_plane = align_up(stab_row * (size_t)geom.H, kStagePlaneAlign);
  if (hipMalloc((void **)&d_stab.p, stab_plane * ring()) != hipSuccess || hipMalloc((void **)&d_filt.p, stab_plane * batch) != hipSuccess)
    return fail(G1S_ERR_HIP, "hipMalloc of the stabilised luma planes failed");
  return G1S_OK;
}

// the two sets' vectors for the geometry in hand
int g1s_denoise::need_mv() {
  if (d_mv[0]) return G1S_OK;
  mv_frame = mv_layout(geom, 2 * D, mv_off);
  for (DevBuf<int8_t> &b : d_mv)
    if (hipMalloc((void **)&b.p, mv_frame * batch) != hipSuccess) return fail(G1S_ERR_HIP, "hipMalloc of the motion vectors failed");
  return G1S_OK;
}

// the three rings of a coarse level for the geometry in hand
int g1s_denoise::need_levels() {
  if (d_cin) return G1S_OK;
  cgeom = geom, cgeom.W = (geom.W + 1) >> 1, cgeom.H = (geom.H + 1) >> 1;  // (rule 25: its chroma planes are the chroma planes' boxes)
  PlaneGeom dg = cgeom;
  dg.bps = 2;
  clay = staging_layout(cgeom), dlay = staging_layout(dg);
  if (hipMalloc((void **)&d_cin.p, clay.frame * ring()) != hipSuccess || hipMalloc((void **)&d_cout.p, clay.frame * batch) != hipSuccess ||
      hipMalloc((void **)&d_d.p, dlay.frame * batch) != hipSuccess)
    return fail(G1S_ERR_HIP, "hipMalloc of the coarse level's planes failed");
  return G1S_OK;
}

// In front of a batch's fine launches: kd_down for the `ndown` frames from `first_down` on (the set's first jobs), those
// frames handed to the inner level as device frames, and the inner level's launches for the batch's frames.  Everything
// is ordered by the one stream.
int g1s_denoise::coarse_level(int set, uint32_t nframes, uint32_t ndown, uint64_t first_down) {
  G1S_OP_TRY(p_level.upload(set, level_bytes(), stream));
  if (timing) G1S_OP_TRY(hipEventRecord(evl[0], stream));
  const int W[3] = {(int)geom.pw(0), (int)geom.pw(1), (int)geom.pw(2)}, H[3] = {(int)geom.ph(0), (int)geom.ph(1), (int)geom.ph(2)};
  G1S_OP_TRY(g1s_lv::launch_down((int)bps, reinterpret_cast<const g1s_lv::LevelJob *>(p_level.d[set].p), ndown, geom.nplanes, W, H, stream));
  if (timing) G1S_OP_TRY(hipEventRecord(evl[4], stream));
  for (uint64_t m = first_down; m < first_down + ndown; ++m) {
    g1s_frame_t fi{}, fo{};
    fi.width = (uint32_t)cgeom.W, fi.height = (uint32_t)cgeom.H, fi.bytes_per_sample = (uint8_t)bps, fi.xdec = (uint8_t)cgeom.subx, fi.ydec = (uint8_t)cgeom.suby;
    fi.nplanes = (uint8_t)cgeom.nplanes, fi.on_device = 1;
    fo = fi;
    clay.point(fi, d_cin + clay.frame * (size_t)(m % ring()), cgeom.nplanes);
    clay.point(fo, d_cout + clay.frame * (size_t)(m % batch), cgeom.nplanes);
    if (g1s_denoise_frame(inner, &fi, &fo) != G1S_OK) return fail(inner->err_code, "coarse level: " + inner->err);
  }
  if (inner->launch_up_to(next_launch + nframes) != G1S_OK) return fail(inner->err_code, "coarse level: " + inner->err);
  if (timing) G1S_OP_TRY(hipEventRecord(evl[1], stream));
  return G1S_OK;
}

// Behind a batch's fine launches (rule 27): d = c - box(out), out += U(d) in place -- on the caller's plane or the staging slot
int g1s_denoise::merge(int set, uint32_t nframes) {
  const g1s_lv::LevelJob *jobs = reinterpret_cast<const g1s_lv::LevelJob *>(p_level.d[set].p + off_merge());
  const int W[3] = {(int)geom.pw(0), (int)geom.pw(1), (int)geom.pw(2)}, H[3] = {(int)geom.ph(0), (int)geom.ph(1), (int)geom.ph(2)};
  if (timing) G1S_OP_TRY(hipEventRecord(evl[2], stream));
  G1S_OP_TRY(g1s_lv::launch_lowres((int)bps, jobs, nframes, geom.nplanes, W, H, stream));
  G1S_OP_TRY(g1s_lv::launch_add((int)bps, (int)bit_depth, jobs, nframes, geom.nplanes, W, H, stream));
  if (timing) G1S_OP_TRY(hipEventRecord(evl[3], stream));
  return G1S_OK;
}

// kd_motion for the planes of a class (plane0 = 0: luma, in samples of bps_ bytes; 1: the chroma planes, or under the joint
// flag the pair) of `nframes` jobs with nnb neighbours each
int g1s_denoise::launch_motion(const DenoiseJobTM *jobs, const PlaneGeom &pg, uint32_t nframes, uint32_t nnb, int plane0, uint32_t bps_, hipStream_t st) {
  MotionParams p{};
  p.jobs = jobs, p.M = (int)M, p.W = (int)pg.pw(plane0), p.H = (int)pg.ph(plane0), p.tiles_x = (p.W + kTW - 1) / kTW, p.plane0 = plane0, p.nnb = (int)nnb;
  p.blocks = blocks_of(pg, plane0);
  const bool pair = plane0 && joint;
  const dim3 grid((unsigned)p.blocks, plane0 && !pair ? 2u : 1u, nframes * nnb);
  const size_t lds = (size_t)motion_geom((int)M, pair ? 2 : 1).bytes;
  if (pair) {
    if (bps_ == 2) hipLaunchKernelGGL((kd_motion<2, 2>), grid, dim3(kThreads), lds, st, p);
    else hipLaunchKernelGGL((kd_motion<1, 2>), grid, dim3(kThreads), lds, st, p);
  } else {
    if (bps_ == 2) hipLaunchKernelGGL((kd_motion<2, 1>), grid, dim3(kThreads), lds, st, p);
    else hipLaunchKernelGGL((kd_motion<1, 1>), grid, dim3(kThreads), lds, st, p);
  }
  G1S_OP_TRY(hipGetLastError());
  return G1S_OK;
}

// frames next_launch .. next_launch + nframes - 1 as one batch (nframes <= batch); their neighbours are in the queue
int g1s_denoise::flush(uint32_t nframes) {
  if (!nframes) return G1S_OK;
  int set, rc = next_set(&set);
  if (rc) return rc;
  bool host_outs = false;
  // with a curve: every frame this batch reads that is not in its slot yet goes forward -- the batch's own and the up to D
  // behind them.  A slot is written again batch + 2D frames later, by a batch that starts beyond every frame that read it.
  uint32_t nfwd = 0;
  if (curve) {
    g1s_cv::CurveJob *cf = reinterpret_cast<g1s_cv::CurveJob *>(p_jobs.h[set].p + off_fwd());
    for (const uint64_t upto = std::min<uint64_t>(frames_in, next_launch + nframes + D); next_stab < upto; ++next_stab)
      cf[nfwd++] = g1s_cv::CurveJob{frame(next_stab).in[0], stab_slot(next_stab), frame(next_stab).in_stride[0], (uint32_t)stab_row};
  }
  // with coarse levels: the same for the coarse frames -- kd_down's jobs
  uint32_t ndown = 0;
  const uint64_t first_down = next_coarse;
  if (K) {
    g1s_lv::LevelJob *dj = reinterpret_cast<g1s_lv::LevelJob *>(p_level.h[set].p);
    for (const uint64_t upto = std::min<uint64_t>(frames_in, next_launch + nframes + D); next_coarse < upto; ++next_coarse) {
      g1s_lv::LevelJob &j = dj[ndown++];
      j = g1s_lv::LevelJob{};
      for (int c = 0; c < geom.nplanes; ++c) {
        j.fine[c] = const_cast<uint8_t *>(frame(next_coarse).in[c]), j.fine_stride[c] = frame(next_coarse).in_stride[c];
        j.coarse[c] = d_cin + clay.frame * (size_t)(next_coarse % ring()) + clay.off[c], j.coarse_stride[c] = (uint32_t)clay.row[c];
      }
    }
  }
  for (uint32_t i = 0; i < nframes; ++i) {
    const uint64_t n = next_launch + i;
    const Queued &f = frame(n);
    // the widest job, and one more for the luma launch under a curve; slot i of the set takes the part this form's kernels index
    DenoiseJobTM tm{}, ltm{};
    DenoiseJob &job = tm.t.f, &lj = ltm.t.f;
    for (int c = 0; c < geom.nplanes; ++c) {
      job.in[c] = f.in[c], job.in_stride[c] = f.in_stride[c];
      job.out[c] = f.host_out ? stage_out(i, c) : f.out[c];
      job.out_stride[c] = f.host_out ? (uint32_t)stage.row[c] : f.out_stride[c];
    }
    host_outs = host_outs || f.host_out;
    if (K) {  // the merge's job: the coarse level's output of the frame, its d, and the planes the fine launch writes
      g1s_lv::LevelJob &j = reinterpret_cast<g1s_lv::LevelJob *>(p_level.h[set].p + off_merge())[i];
      j = g1s_lv::LevelJob{};
      for (int c = 0; c < geom.nplanes; ++c) {
        j.fine[c] = job.out[c], j.fine_stride[c] = job.out_stride[c];
        j.coarse[c] = d_cout + clay.frame * (size_t)(n % batch) + clay.off[c], j.coarse_stride[c] = (uint32_t)clay.row[c];
        j.d[c] = d_d + dlay.frame * (size_t)i + dlay.off[c], j.d_stride[c] = (uint32_t)dlay.row[c];
      }
    }
    // (rule 14) the luma launch's job: from the frame's slot into plane i of the filtered ones, which the inverse takes
    // to where the frame's luma goes
    if (curve) {
      lj.in[0] = stab_slot(n), lj.out[0] = d_filt + stab_plane * i, lj.in_stride[0] = lj.out_stride[0] = (uint32_t)stab_row;
      reinterpret_cast<g1s_cv::CurveJob *>(p_jobs.h[set].p + off_inv())[i] = g1s_cv::CurveJob{lj.out[0], job.out[0], (uint32_t)stab_row, job.out_stride[0]};
    }
    int k = 0;
    for (int64_t m = (int64_t)n - (int64_t)D; m <= (int64_t)(n + D); ++m) {
      if (m == (int64_t)n) continue;
      if (m >= (int64_t)clip_first && m < (int64_t)frames_in) {  // rule 5: the frames the clip has
        for (int c = 0; c < geom.nplanes; ++c) tm.t.nb[c][k] = frame((uint64_t)m).in[c], tm.t.nb_stride[c][k] = frame((uint64_t)m).in_stride[c];
        if (curve) ltm.t.nb[0][k] = stab_slot((uint64_t)m), ltm.t.nb_stride[0][k] = (uint32_t)stab_row;
      }
      ++k;
    }
    // (the stabilised luma's vectors are the luma's: one search, on the planes the filter filters -- rule 20)
    for (int c = 0; M && c < geom.nplanes; ++c) tm.mv[c] = d_mv[set] + mv_frame * i + mv_off[c];
    ltm.mv[0] = tm.mv[0];
    std::memcpy(p_jobs.h[set].p + job_bytes() * i, &tm, job_bytes());
    if (curve) std::memcpy(p_jobs.h[set].p + off_luma() + job_bytes() * i, &ltm, job_bytes());
  }
  G1S_OP_TRY(p_jobs.upload(set, curve ? set_bytes() : job_bytes() * nframes, stream));
  if (timing) G1S_OP_TRY(hipEventRecord(ev[0], stream));
  if (K && (rc = coarse_level(set, nframes, ndown, first_down)) != 0) return rc;
  if (curve)
    G1S_OP_TRY(g1s_cv::launch_curve((int)bps, 2, reinterpret_cast<const g1s_cv::CurveJob *>(p_jobs.d[set].p + off_fwd()), nfwd, d_curve, 1u << bit_depth,
                                    (uint32_t)geom.W, (uint32_t)geom.H, stream));
  if (D && M) {
    // the batch's vectors, in front of its filter launches: luma on what the luma launch filters, then chroma
    const uint8_t *dj = p_jobs.d[set].p;
    if (timing) G1S_OP_TRY(hipEventRecord(ev[2], stream));
    if ((rc = launch_motion(reinterpret_cast<const DenoiseJobTM *>(dj + (curve ? off_luma() : 0)), geom, nframes, 2 * D, 0, curve ? 2u : bps, stream)) != 0) return rc;
    if (geom.nplanes == 3 && (rc = launch_motion(reinterpret_cast<const DenoiseJobTM *>(dj), geom, nframes, 2 * D, 1, bps, stream)) != 0) return rc;
    if (timing) G1S_OP_TRY(hipEventRecord(ev[1], stream));
    if (timing) G1S_OP_TRY(hipStreamSynchronize(stream));
    float a = 0;
    if (timing) G1S_OP_TRY(hipEventElapsedTime(&a, ev[2], ev[1]));
    ms_motion += a;
  }
  if (curve) {
    const uint8_t *dj = p_jobs.d[set].p;
    if ((rc = launch(set, nframes, 0, 1, true)) != 0) return rc;
    G1S_OP_TRY(g1s_cv::launch_curve(2, (int)bps, reinterpret_cast<const g1s_cv::CurveJob *>(dj + off_inv()), nframes, d_curve + (1u << bit_depth),
                                    g1s_cv::kInvEntries, (uint32_t)geom.W, (uint32_t)geom.H, stream));
  } else if ((rc = launch(set, nframes, 0, 1)) != 0) {
    return rc;
  }
  if (geom.nplanes == 3 && (rc = joint ? launch_joint(set, nframes) : launch(set, nframes, 1, 2)) != 0) return rc;
  if (K && (rc = merge(set, nframes)) != 0) return rc;
  if (timing) G1S_OP_TRY(hipEventRecord(ev[1], stream));
  if ((rc = set_done(set)) != 0) return rc;
  for (uint32_t i = 0; host_outs && i < nframes; ++i)
    if (frame(next_launch + i).host_out && (rc = copy_back(i, frame(next_launch + i).host)) != 0) return rc;
  if (timing) {
    G1S_OP_TRY(hipStreamSynchronize(stream));
    float a = 0;
    G1S_OP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    ms_kernel += a, frames_timed += nframes;
    if (K) {
      // evl: 0 in front of kd_down, 4 behind it, 1 behind the inner level's launches; 2 in front of kd_lowres, 3 behind kd_add
      float front = 0, down = 0, merged = 0;
      G1S_OP_TRY(hipEventElapsedTime(&front, evl[0], evl[1]));
      G1S_OP_TRY(hipEventElapsedTime(&down, evl[0], evl[4]));
      G1S_OP_TRY(hipEventElapsedTime(&merged, evl[2], evl[3]));
      ms_level += front + merged, ms_level_k += down + merged;
    }
  }
  next_launch += nframes;
  // what stays in front of the frames to come: the D frames before the next one to launch
  while (first_queued + D < next_launch) queue.pop_front(), ++first_queued;
  return G1S_OK;
}

// every frame below `limit` that is not launched yet, a batch at a time
int g1s_denoise::launch_up_to(uint64_t limit) {
  while (next_launch < limit) {
    const int rc = flush((uint32_t)std::min<uint64_t>(batch, limit - next_launch));
    if (rc) return rc;
  }
  return G1S_OK;
}

// the clip ends here: what is queued goes out with the neighbours it has and is waited for
int g1s_denoise::end_clip() {
  int rc = launch_up_to(frames_in);
  if (rc || (rc = wait()) != 0) return rc;
  queue.clear();
  first_queued = clip_first = frames_complete = next_stab = next_coarse = frames_in;
  // (the coarse frames of a clip are a clip with the same ends)
  if (inner && inner->end_clip() != G1S_OK) return fail(inner->err_code, "coarse level: " + inner->err);
  return G1S_OK;
}

// what makes a denoiser beyond the opts; `curve`: with the pair (fwd, inv) of rules 12 - 15
struct DenoiserSpec {
  uint32_t temporal_radius = 0, flags = 0;
  bool curve = false;
  const uint16_t *fwd = nullptr, *inv = nullptr;
  uint32_t motion_range = 0;
  const uint16_t *chroma_gain = nullptr;
  uint32_t coarse_levels = 0;
  double coarse_ratio = 0.0;
  hipStream_t share = nullptr;  // (an inner level) the stream of the denoiser that owns this one
};

// rule 28: the refusals of K levels at ratio rho (0: 1.0) over the strengths h, hc of level 0, which passed rule 3's
// bounds.  Level l's strengths are rho times level l - 1's.  "" when fine.
static std::string levels_refusal(uint32_t K, double rho, double h, double hc) {
  if (K > (uint32_t)kMaxLevels) return "coarse_levels must be 0..2";
  if (rho != 0.0 && (!(rho >= 0.0625) || !(rho <= 4.0))) return "coarse_ratio must be 0.0625..4 (0 = 1)";
  if (rho != 0.0 && !K) return "coarse_ratio needs coarse_levels";
  const double r = rho != 0.0 ? rho : 1.0;
  for (uint32_t l = 1; l <= K; ++l) {
    h *= r, hc *= r;
    if (!strength_ok(h)) return "level " + std::to_string(l) + " " + kStrengthBound;
    if (!strength_ok(hc)) return "level " + std::to_string(l) + " chroma_" + kStrengthBound;
  }
  return "";
}

// what every g1s_denoise_new* call makes
static g1s_denoise *new_denoiser(uint32_t bit_depth, const g1s_denoise_opts_t *opts, const DenoiserSpec &spec) {
  if (!opts_fit(opts, "g1s_denoise_opts_t")) return nullptr;
  // the parameters first: a refusal needs no device
  const uint32_t A = opts && opts->search_radius ? opts->search_radius : 3u, S = opts && opts->patch_radius ? opts->patch_radius : 2u;
  const Strengths strengths = strengths_of(opts);
  const double h = strengths.h, hc = strengths.hc;
  if (A < 1 || A > (uint32_t)kMaxA) {
    g1s_set_global_error_("search_radius must be 1..7");
    return nullptr;
  }
  if (spec.temporal_radius > (uint32_t)kMaxD) {
    g1s_set_global_error_("temporal_radius must be 0..3");
    return nullptr;
  }
  if (spec.flags & ~G1S_DENOISE_JOINT_CHROMA) {
    g1s_set_global_error_("unknown denoise flags");
    return nullptr;
  }
  if ((spec.motion_range & 1) || spec.motion_range > 2u * (uint32_t)kMaxM) {
    g1s_set_global_error_("motion_range must be even and 0..64");
    return nullptr;
  }
  if (spec.motion_range && !spec.temporal_radius) {
    g1s_set_global_error_("motion_range needs a temporal radius");
    return nullptr;
  }
  if (spec.chroma_gain) {
    const std::string no = g1s_cv::check_gain(spec.chroma_gain);
    if (!no.empty() || !(spec.flags & G1S_DENOISE_JOINT_CHROMA)) {
      g1s_set_global_error_(no.empty() ? "a chroma gain needs joint chroma" : no.c_str());
      return nullptr;
    }
  }
  std::vector<uint16_t> tables(4 * kTable);
  uint32_t q[4] = {0, 0, 0, 0};
  std::string why = make_table(bit_depth, S, h, tables.data(), &q[0]);
  if (why.empty()) {
    why = make_table(bit_depth, S, hc, tables.data() + kTable, &q[1]);
    if (why.empty()) why = make_table(bit_depth, S, hc, tables.data() + 2 * kTable, &q[2], 3);
    if (!why.empty()) why = "chroma_" + why;
  }
  // the curve: luma is filtered as a 12-bit plane with the luma strength (rule 14)
  if (why.empty() && spec.curve) {
    why = g1s_cv::check(bit_depth, spec.fwd, spec.inv);
    if (why.empty()) why = make_table(g1s_cv::kStabBits, S, h, tables.data() + 3 * kTable, &q[3]);
  }
  if (why.empty()) why = levels_refusal(spec.coarse_levels, spec.coarse_ratio, h, hc);
  if (!why.empty()) {
    g1s_set_global_error_(why.c_str());
    return nullptr;
  }
  // (the device's own refusal, of the LDS a workgroup asks for, is the first thing the allocation does)
  return open_op<g1s_denoise>("denoise", opts, bit_depth, [&](g1s_denoise &g, std::string &refusal) {
    // the LDS a workgroup of the largest kernel these parameters select asks for, against what the device gives one
    const bool joint = (spec.flags & G1S_DENOISE_JOINT_CHROMA) != 0;
    {
      const TileGeom tg = tile_geom((int)A, (int)S);
      const JointGeom jg = spec.chroma_gain ? joint_gain_geom(tg) : joint_geom(tg);
      const int need = spec.temporal_radius ? (joint ? jg.bytes_t : tg.bytes_t) : (joint ? jg.bytes : tg.bytes);
      int limit = 0;
      if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, g.device) != hipSuccess || need > limit) {
        refusal = "these parameters need " + std::to_string(need) + " bytes of LDS a workgroup" + (joint ? " (joint chroma)" : "") +
                  "; the device allows " + std::to_string(limit);
        return false;
      }
    }
    g.A = A, g.S = S, g.D = spec.temporal_radius, g.joint = joint;
    g.curve = spec.curve, g.M = spec.motion_range / 2, g.gain = spec.chroma_gain != nullptr;
    for (int i = 0; i < 4; ++i) g.q[i] = q[i];
    g.K = spec.coarse_levels;
    if (spec.share) {  // an inner level runs on its owner's stream: one order for kd_down, its launches and the merge
      (void)hipStreamDestroy(g.stream.p);
      g.stream.p = spec.share, g.borrowed_stream = true;
    }
    bool ok = true;
    for (Event &e : g.ev) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    if (ok && g.K) {
      // rule 26: level K - 1 on the coarse frames -- the strengths times rho, Mr' = 2 ceil(Mr / 4), everything else the same
      const double rho = spec.coarse_ratio != 0.0 ? spec.coarse_ratio : 1.0;
      g1s_denoise_opts_t io{};
      io.struct_size = sizeof io, io.device = g.device, io.batch_frames = g.batch, io.search_radius = A, io.patch_radius = S;
      io.strength = rho * h, io.chroma_strength = rho * hc;
      for (Event &e : g.evl) ok = ok && hipEventCreate(&e.p) == hipSuccess;
      ok = ok && g.p_level.alloc(g.level_bytes());
      if (ok) {
        g.inner = new_denoiser(bit_depth, &io, {spec.temporal_radius, spec.flags, spec.curve, spec.fwd, spec.inv, 2 * ((spec.motion_range + 3) / 4),
                                                spec.chroma_gain, g.K - 1, g.K > 1 ? rho : 0.0, g.stream.p});
        if (!g.inner) {  // (the parameters were checked above: a refusal here is the device's, and its text is this call's)
          refusal = g1s_last_global_error();
          return false;
        }
      }
    }
    ok = ok && g.p_jobs.alloc(g.set_bytes()) && hipMalloc((void **)&g.d_tables.p, tables.size() * 2) == hipSuccess &&
         hipMemcpy(g.d_tables, tables.data(), tables.size() * 2, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && spec.curve) {
      const size_t nf = (size_t)1 << bit_depth;
      ok = hipMalloc((void **)&g.d_curve.p, (nf + g1s_cv::kInvEntries) * 2) == hipSuccess &&
           hipMemcpy(g.d_curve, spec.fwd, nf * 2, hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(g.d_curve + nf, spec.inv, g1s_cv::kInvEntries * 2, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok && spec.chroma_gain)
      ok = hipMalloc((void **)&g.d_gain.p, kGain * 2) == hipSuccess && hipMemcpy(g.d_gain, spec.chroma_gain, kGain * 2, hipMemcpyHostToDevice) == hipSuccess;
    return ok;
  });
}

extern "C" {

int g1s_denoise_weights(uint32_t bit_depth, uint32_t patch_radius, double strength, uint16_t T[1024], uint32_t *q) {
  return g1s_denoise_weights_ex(bit_depth, patch_radius, strength, 0, T, q);
}

int g1s_denoise_weights_ex(uint32_t bit_depth, uint32_t patch_radius, double strength, uint32_t flags, uint16_t T[1024], uint32_t *q) {
  if (!T || !q) return G1S_ERR_INVALID;
  const std::string why = flags & ~G1S_DENOISE_JOINT_CHROMA ? std::string("unknown denoise flags")
                                                            : make_table(bit_depth, patch_radius, strength, T, q, flags & G1S_DENOISE_JOINT_CHROMA ? 3 : 1);
  if (!why.empty()) {
    g1s_set_global_error_(why.c_str());
    return G1S_ERR_INVALID;
  }
  return G1S_OK;
}

g1s_denoise_t *g1s_denoise_new(uint32_t bit_depth, const g1s_denoise_opts_t *opts) { return new_denoiser(bit_depth, opts, {}); }

g1s_denoise_t *g1s_denoise_new_temporal(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius) {
  return new_denoiser(bit_depth, opts, {temporal_radius});
}

g1s_denoise_t *g1s_denoise_new_ex(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags) {
  return new_denoiser(bit_depth, opts, {temporal_radius, flags});
}

g1s_denoise_t *g1s_denoise_new_curve(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags, const uint16_t *fwd,
                                     const uint16_t *inv) {
  return new_denoiser(bit_depth, opts, {temporal_radius, flags, true, fwd, inv});
}

g1s_denoise_t *g1s_denoise_new_motion(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags, const uint16_t *fwd,
                                      const uint16_t *inv, uint32_t motion_range) {
  return new_denoiser(bit_depth, opts, {temporal_radius, flags, fwd || inv, fwd, inv, motion_range});
}

g1s_denoise_t *g1s_denoise_new_gain(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags, const uint16_t *fwd,
                                    const uint16_t *inv, uint32_t motion_range, const uint16_t *chroma_gain) {
  return new_denoiser(bit_depth, opts, {temporal_radius, flags, fwd || inv, fwd, inv, motion_range, chroma_gain});
}

g1s_denoise_t *g1s_denoise_new_levels(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags, const uint16_t *fwd,
                                      const uint16_t *inv, uint32_t motion_range, const uint16_t *chroma_gain, uint32_t coarse_levels, double coarse_ratio) {
  return new_denoiser(bit_depth, opts, {temporal_radius, flags, fwd || inv, fwd, inv, motion_range, chroma_gain, coarse_levels, coarse_ratio});
}

// (denoise_file.cpp) rule 28's refusals for a command that looks for its device before it makes the denoiser: the text into
// err, or "" -- with the strengths as the opts give them (0 = the default; an auto strength is checked when the denoiser is made)
void g1s_denoise_levels_refusal_(const g1s_denoise_opts_t *opts, uint32_t coarse_levels, double coarse_ratio, char *err, size_t cap) {
  // (opts of another size, or strengths rule 3 refuses: the constructor says so; the levels are then looked at over the defaults)
  Strengths s = strengths_of(opts && opts->struct_size == sizeof(g1s_denoise_opts_t) ? opts : nullptr);
  if (!strength_ok(s.h) || !strength_ok(s.hc)) s = strengths_of(nullptr);
  const std::string why = levels_refusal(coarse_levels, coarse_ratio, s.h, s.hc);
  if (err && cap) snprintf(err, cap, "%s", why.c_str());
}

// (denoise_file.cpp) what the file commands size their rings by
uint32_t g1s_denoise_batch_(const g1s_denoise_t *g) { return g->batch; }
uint32_t g1s_denoise_temporal_radius_(const g1s_denoise_t *g) { return g->D; }

// stage 1 alone: both frames on the device (a host frame in an allocation of this call), luma through the forward curve
// where there is one, one job with `ref` as its only neighbour, kd_motion, the vectors back
int g1s_denoise_motion_search(g1s_denoise_t *g, const g1s_frame_t *cur, const g1s_frame_t *ref, int16_t *mv[3], size_t cap_pairs[3]) {
  if (!g || !cur || !ref || !mv || !cap_pairs) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  if (!g->M) return g->fail(G1S_ERR_INVALID, "g1s_denoise_motion_search needs a denoiser with a motion range");
  (void)hipSetDevice(g->device);
  const Refusal no = check_frame_pair(*cur, *ref, g->bps, 65536u, "g1s_denoise_new_motion",
                                      "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)", "the two");
  if (no.code) return g->fail(no.code, no.text);
  const PlaneGeom pg(*cur, g->bps);
  size_t off[3] = {0, 0, 0};
  const size_t bytes = g->mv_layout(pg, 1, off);
  bool fits = true;
  for (int c = 0; c < pg.nplanes; ++c) {
    const size_t need = (size_t)g->blocks_of(pg, c);
    fits = fits && mv[c] && cap_pairs[c] >= need;
    cap_pairs[c] = need;
  }
  if (!fits) return G1S_ERR_CAPACITY;
  // the planes kd_motion reads: the caller's device planes, or copies; luma with a curve: its stabilised form
  const Layout lay = staging_layout(pg);
  const size_t stab_row = align_up((size_t)pg.W * 2, kStageRowAlign), stab_plane = align_up(stab_row * (size_t)pg.H, kStagePlaneAlign);
  DevBuf<uint8_t> copy[2], stab;
  DevBuf<uint8_t> d_job;
  DevBuf<int8_t> d_v;
  DenoiseJobTM job{};
  g1s_cv::CurveJob cj[2];
  const g1s_frame_t *fr[2] = {cur, ref};
  if (hipMalloc((void **)&d_job.p, sizeof job + sizeof cj) != hipSuccess || hipMalloc((void **)&d_v.p, bytes) != hipSuccess ||
      (g->curve && hipMalloc((void **)&stab.p, 2 * stab_plane) != hipSuccess))
    return g->fail(G1S_ERR_HIP, "hipMalloc for the motion search failed");
  for (int i = 0; i < 2; ++i) {
    const uint8_t *pl[3] = {nullptr, nullptr, nullptr};
    uint32_t st[3] = {0, 0, 0};
    if (fr[i]->on_device != 1 && hipMalloc((void **)&copy[i].p, lay.frame) != hipSuccess) return g->fail(G1S_ERR_HIP, "hipMalloc for the motion search failed");
    for (int c = 0; c < pg.nplanes; ++c) {
      if (fr[i]->on_device == 1) {
        pl[c] = static_cast<const uint8_t *>(fr[i]->data[c]), st[c] = (uint32_t)fr[i]->stride_bytes[c];
        continue;
      }
      uint8_t *dst = copy[i] + lay.off[c];
      G1S_OP_TRY_(g, hipMemcpy2DAsync(dst, lay.row[c], fr[i]->data[c], fr[i]->stride_bytes[c], pg.row_bytes(c), pg.ph(c), hipMemcpyHostToDevice, g->stream));
      pl[c] = dst, st[c] = (uint32_t)lay.row[c];
    }
    if (g->curve) {
      cj[i] = g1s_cv::CurveJob{pl[0], stab + stab_plane * (size_t)i, st[0], (uint32_t)stab_row};
      pl[0] = stab + stab_plane * (size_t)i, st[0] = (uint32_t)stab_row;
    }
    for (int c = 0; c < pg.nplanes; ++c) {
      if (i == 0) job.t.f.in[c] = pl[c], job.t.f.in_stride[c] = st[c], job.mv[c] = d_v + off[c];
      else job.t.nb[c][0] = pl[c], job.t.nb_stride[c][0] = st[c];
    }
  }
  G1S_OP_TRY_(g, hipMemcpyAsync(d_job, &job, sizeof job, hipMemcpyHostToDevice, g->stream));
  if (g->curve) {
    G1S_OP_TRY_(g, hipMemcpyAsync(d_job + sizeof job, cj, sizeof cj, hipMemcpyHostToDevice, g->stream));
    G1S_OP_TRY_(g, g1s_cv::launch_curve((int)g->bps, 2, reinterpret_cast<const g1s_cv::CurveJob *>(d_job + sizeof job), 2, g->d_curve, 1u << g->bit_depth,
                                        (uint32_t)pg.W, (uint32_t)pg.H, g->stream));
  }
  int rc = g->launch_motion(reinterpret_cast<const DenoiseJobTM *>(d_job.p), pg, 1, 1, 0, g->curve ? 2u : g->bps, g->stream);
  if (!rc && pg.nplanes == 3) rc = g->launch_motion(reinterpret_cast<const DenoiseJobTM *>(d_job.p), pg, 1, 1, 1, g->bps, g->stream);
  if (rc) return rc;
  std::vector<int8_t> v(bytes);
  G1S_OP_TRY_(g, hipMemcpyAsync(v.data(), d_v, bytes, hipMemcpyDeviceToHost, g->stream));
  if ((rc = g->wait()) != 0) return rc;  // (the job, the copies and the pageable copies above are this call's: through before it returns)
  for (int c = 0; c < pg.nplanes; ++c)
    for (size_t i = 0; i < 2 * cap_pairs[c]; ++i) mv[c][i] = v[off[c] + i];
  return G1S_OK;
}

int g1s_denoise_motion_time(g1s_denoise_t *g, double *ms_motion) {
  if (!g || !ms_motion) return G1S_ERR_INVALID;
  *ms_motion = g->ms_motion;
  return G1S_OK;
}

int g1s_denoise_level_time(g1s_denoise_t *g, double *ms_level) {
  if (!g || !ms_level) return G1S_ERR_INVALID;
  *ms_level = g->ms_level;
  return G1S_OK;
}

int g1s_denoise_level_kernel_time(g1s_denoise_t *g, double *ms_kernels) {
  if (!g || !ms_kernels) return G1S_ERR_INVALID;
  *ms_kernels = 0;
  for (const g1s_denoise *l = g; l; l = l->inner) *ms_kernels += l->ms_level_k;
  return G1S_OK;
}

int g1s_denoise_frame(g1s_denoise_t *g, const g1s_frame_t *in, g1s_frame_t *out) {
  if (!g || !in || !out) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  const Refusal no = check_frame_pair(*in, *out, g->bps, 65536u, "g1s_denoise_new",
                                      "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)");
  if (no.code) return g->fail(no.code, no.text);
  int rc;
  if (g->have_geom && !g->geom.same_shape(*in)) {
    // a new geometry: the clip ends, what is queued goes out and finishes first, the staging buffers are sized again
    if ((rc = g->end_clip()) != 0) return rc;
    g->have_geom = false;
  }
  if (!g->have_geom) {
    g->set_frame_geometry(*in), g->d_stab = DevBuf<uint8_t>(), g->d_filt = DevBuf<uint8_t>(), g->d_mv[0] = DevBuf<int8_t>(), g->d_mv[1] = DevBuf<int8_t>();
    g->d_cin = DevBuf<uint8_t>(), g->d_cout = DevBuf<uint8_t>(), g->d_d = DevBuf<uint8_t>();
  }
  if (g->K && (rc = g->need_levels()) != 0) return rc;
  if (g->curve && (rc = g->need_stab()) != 0) return rc;
  if (g->M && (rc = g->need_mv()) != 0) return rc;
  const PlaneGeom &gm = g->geom;
  g1s_denoise::Queued f{};
  // the input ring's slot: a launched frame stays a neighbour.  The output buffer is `batch` slots, chosen at the launch
  if ((rc = g->stage_in(*in, (uint32_t)(g->frames_in % g->ring()), g->ring(), f.in, f.in_stride)) != 0) return rc;
  f.host_out = out->on_device != 1;
  if (f.host_out && (rc = g->need_stage_out(g->batch)) != 0) return rc;
  if (f.host_out) f.host = host_planes(*out);
  for (int c = 0; !f.host_out && c < gm.nplanes; ++c)
    f.out[c] = static_cast<uint8_t *>(const_cast<void *>(out->data[c])), f.out_stride[c] = (uint32_t)out->stride_bytes[c];
  // in != out: no device plane of the output may overlap a plane of the input -- nor, with a temporal radius, a plane the
  // queue still reads, and no plane of the input may be one that a frame of the queue is going to write
  if (!f.host_out) {
    for (int c = 0; c < gm.nplanes; ++c)
      for (int d = 0; d < gm.nplanes; ++d) {
        bool bad = planes_overlap(gm, f.out[c], f.out_stride[c], c, f.in[d], f.in_stride[d], d);
        if (g->D)
          for (const g1s_denoise::Queued &o : g->queue) bad = bad || planes_overlap(gm, f.out[c], f.out_stride[c], c, o.in[d], o.in_stride[d], d);
        if (bad) return g->fail(G1S_ERR_INVALID, "input and output planes overlap: g1s_denoise_frame needs distinct buffers");
      }
  }
  for (uint64_t n = g->next_launch; g->D && n < g->frames_in; ++n) {
    const g1s_denoise::Queued &o = g->frame(n);
    if (o.host_out) continue;
    for (int c = 0; c < gm.nplanes; ++c)
      for (int d = 0; d < gm.nplanes; ++d)
        if (planes_overlap(gm, o.out[c], o.out_stride[c], c, f.in[d], f.in_stride[d], d))
          return g->fail(G1S_ERR_INVALID, "input and output planes overlap: g1s_denoise_frame needs distinct buffers");
  }
  if ((rc = g->wait_host_input(*in)) != 0) return rc;
  g->queue.push_back(f);
  ++g->frames_in;
  // a full batch of frames whose D later neighbours are all there goes out; the last D frames wait for theirs
  if (g->frames_in >= g->next_launch + g->D + g->batch) return g->flush(g->batch);
  return G1S_OK;
}

int g1s_denoise_drain(g1s_denoise_t *g, uint64_t *frames_complete) {
  if (!g) return G1S_ERR_INVALID;
  if (frames_complete) *frames_complete = g->frames_complete;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  const uint64_t limit = g->frames_in >= g->clip_first + g->D ? g->frames_in - g->D : g->clip_first;
  int rc = g->launch_up_to(limit);
  if (rc || (rc = g->wait()) != 0) return rc;
  g->frames_complete = g->next_launch;
  if (frames_complete) *frames_complete = g->frames_complete;
  return G1S_OK;
}

int g1s_denoise_sync(g1s_denoise_t *g) {
  if (!g) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  return g->end_clip();
}

int g1s_denoise_set_timing(g1s_denoise_t *g, int enable, double *ms_kernel, uint64_t *frames) {
  if (!g) return G1S_ERR_INVALID;
  for (g1s_denoise *l = g; l; l = l->inner) l->timing = enable != 0;  // (a timed inner level gives the three kernels' own time)
  if (ms_kernel) *ms_kernel = g->ms_kernel;
  if (frames) *frames = g->frames_timed;
  return G1S_OK;
}

const char *g1s_denoise_last_error(const g1s_denoise_t *g) { return g ? g->err.c_str() : ""; }

void g1s_denoise_free(g1s_denoise_t *g) { free_op(g); }

}  // extern "C"
