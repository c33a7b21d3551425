// denoise.hip -- `denoise`: the project's integer-exact non-local-means filter on the device.
//
// The filter is defined in include/g1s_diff.h ("denoise", rules 1 - 4); tests/denoise_ref.py restates it in numpy.  It is
// this project's own definition of non-local means: ffmpeg's nlmeans and KNLMeansCL have the same structure, not the
// same bits.  Two kernels, a workgroup per (tile, plane of the class, frame), the phases of denoise_tile.hip.h:
// kd_nlm<S, BPS> for one frame on its own (temporal radius 0, rules 1 - 4) and kd_nlm_t<S, BPS>, which goes on over the
// frames around it (rules 5 - 7).  A batch of frames goes out as one launch per plane class (luma; the two chroma planes)
// on the denoiser's own stream.  Planes are independent, but `out` must not overlap `in`: a tile reads the halo its
// neighbours write.
//
// The engine numbers the frames handed over since the denoiser was made.  With temporal radius D a frame is launched once
// the D frames after it are there (or the clip ends), so the queue holds the frames not yet launched and, in front of
// them, the last D that were: their planes are the neighbours of what comes next.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "denoise_tile.hip.h"

extern "C" void g1s_set_global_error_(const char *);  // (engine.hip)
extern "C" void g1s_diff_set_error_text_(g1s_diff_t *, const char *);
extern "C" int32_t g1s_diff_device_(const g1s_diff_t *);
extern "C" uint32_t g1s_diff_frames_in_flight_max_(const g1s_diff_t *);

namespace {

using namespace g1s_dn;

struct DenoiseJob {
  const uint8_t *in[3];
  uint8_t *out[3];
  uint32_t in_stride[3], out_stride[3];  // bytes
};

struct DenoiseParams {
  const DenoiseJob *jobs;
  const uint16_t *table;  // the class's 1024 weights
  int q, A;
  int W, H, tiles_x;  // the class's plane size
  int plane0;         // first plane of the class: 0 luma, 1 chroma
};

// the temporal kernel's job: the frame and, per plane, the 2 D frames around it (null: the clip has no such frame)
struct DenoiseJobT {
  DenoiseJob f;
  const uint8_t *nb[3][2 * kMaxD];
  uint32_t nb_stride[3][2 * kMaxD];
};

struct DenoiseParamsT {
  const DenoiseJobT *jobs;
  const uint16_t *table;
  int q, A;
  int W, H, tiles_x;
  int plane0;
  int nnb;  // 2 D
};

template <int S, int BPS>
__global__ __launch_bounds__(kThreads) void kd_nlm_t(DenoiseParamsT p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dn_lds[];
  const DenoiseJobT &job = p.jobs[blockIdx.z];
  const int c = p.plane0 + (int)blockIdx.y;
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
  const TileGeom g = tile_geom(p.A, S);
  dn_tile_t<S, BPS>((int)threadIdx.x, g, dn_lds, p.table, p.q, job.f.in[c], job.f.in_stride[c], job.nb[c], job.nb_stride[c], p.nnb, job.f.out[c],
                    job.f.out_stride[c], p.W, p.H, tx * kTW, ty * kTH, [] { __syncthreads(); });
}

template <int S, int BPS>
__global__ __launch_bounds__(kThreads) void kd_nlm(DenoiseParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dn_lds[];
  const DenoiseJob &job = p.jobs[blockIdx.z];
  const int c = p.plane0 + (int)blockIdx.y;
  const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
  const TileGeom g = tile_geom(p.A, S);
  dn_tile<S, BPS>((int)threadIdx.x, g, dn_lds, p.table, p.q, job.in[c], job.in_stride[c], job.out[c], job.out_stride[c], p.W, p.H, tx * kTW,
                  ty * kTH, [] { __syncthreads(); });
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// rule 3.  "" when fine.
std::string make_table(uint32_t bit_depth, uint32_t S, double h, uint16_t T[kTable], uint32_t *q_out) {
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return "denoise is defined for bit depths 8, 10 and 12";
  if (S < 1 || S > (uint32_t)kMaxS) return "patch_radius must be 1..4";
  if (!(h > 0.0) || !(h <= 1000.0)) return "strength must be greater than 0 and at most 1000";
  const double n = (double)((2 * S + 1) * (2 * S + 1)), den = n * h * h * std::pow(4.0, (double)bit_depth - 8.0);
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
struct g1s_denoise {
  int device = 0;
  uint32_t bit_depth = 8, bps = 1, batch = 32;
  uint32_t A = 3, S = 2, D = 0;
  uint32_t q[2] = {0, 0};  // luma, chroma
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool have_geom = false;
  int W = 0, H = 0, subx = 0, suby = 0, nplanes = 0;
  size_t plane_row[3] = {0, 0, 0}, plane_off[3] = {0, 0, 0}, stage_frame = 0;  // staging layout of a host frame on the device
  // a frame handed over: its planes on the device (the caller's, or a slot of the input staging ring) and where its
  // output goes (out[c] is null for a host frame: a slot of the output staging buffer is chosen at the launch)
  struct Queued {
    const uint8_t *in[3];
    uint8_t *out[3];
    uint32_t in_stride[3], out_stride[3];
    bool host_out;
    void *host_data[3];
    size_t host_stride[3];
  };
  // frames [first_queued, frames_in): what is not launched yet and, in front of it, up to D launched frames of the same clip
  std::deque<Queued> queue;
  uint64_t frames_in = 0, first_queued = 0, next_launch = 0, clip_first = 0, frames_complete = 0;
  // the jobs of a batch, two sets in turn: pinned on the host, uploaded on the stream, free again when the event behind
  // the batch's kernels has passed -- the next batch is filled while this one runs
  uint8_t *d_jobs[2] = {nullptr, nullptr}, *h_jobs[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  uint64_t batches = 0;
  uint16_t *d_tables = nullptr;  // [2][1024]
  uint8_t *d_stage_in = nullptr, *d_stage_out = nullptr;
  int err_code = 0;
  std::string err;
  bool timing = false;
  double ms_kernel = 0;
  uint64_t frames_timed = 0;

  int fail(int code, const std::string &m) {
    if (!err_code) err_code = code, err = m;  // sticky: the first failure is the one reported from then on
    return err_code;
  }
  size_t pw(int c) const { return c ? (size_t)((W + subx) >> subx) : (size_t)W; }
  size_t ph(int c) const { return c ? (size_t)((H + suby) >> suby) : (size_t)H; }
  size_t job_bytes() const { return D ? sizeof(DenoiseJobT) : sizeof(DenoiseJob); }
  // host and pinned inputs wait on the device in a ring: a slot is written again B + 2D frames later, and by then every
  // frame that reads it (up to D frames on) has been launched in front of that copy on the stream
  uint32_t ring() const { return batch + 2 * D; }
  const Queued &frame(uint64_t n) const { return queue[(size_t)(n - first_queued)]; }
  void set_geometry(const g1s_frame_t &f);
  int launch(int set, uint32_t nframes, int plane0, int nplanes_in_class);
  int flush(uint32_t nframes);
  int launch_up_to(uint64_t limit);
  int end_clip();
};

#define DN_TRY(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return fail(G1S_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
  } while (0)

void g1s_denoise::set_geometry(const g1s_frame_t &f) {
  W = (int)f.width, H = (int)f.height, subx = f.xdec, suby = f.ydec, nplanes = f.nplanes;
  size_t off = 0;
  for (int c = 0; c < nplanes; ++c) {
    plane_row[c] = align_up(pw(c) * bps, 16);
    plane_off[c] = off;
    off += align_up(plane_row[c] * ph(c), 256);
  }
  stage_frame = off;
  have_geom = true;
}

int g1s_denoise::launch(int set, uint32_t nframes, int plane0, int nplanes_in_class) {
  DenoiseParams p{};
  p.jobs = reinterpret_cast<const DenoiseJob *>(d_jobs[set]), p.table = d_tables + (plane0 ? kTable : 0), p.q = (int)q[plane0 ? 1 : 0], p.A = (int)A;
  p.W = (int)pw(plane0), p.H = (int)ph(plane0), p.tiles_x = (p.W + kTW - 1) / kTW, p.plane0 = plane0;
  const dim3 grid((unsigned)(p.tiles_x * ((p.H + kTH - 1) / kTH)), (unsigned)nplanes_in_class, nframes);
  const TileGeom geom = tile_geom((int)A, (int)S);
  if (D) {
    DenoiseParamsT t{};
    t.jobs = reinterpret_cast<const DenoiseJobT *>(d_jobs[set]), t.table = p.table, t.q = p.q, t.A = p.A, t.W = p.W, t.H = p.H, t.tiles_x = p.tiles_x,
    t.plane0 = plane0, t.nnb = (int)(2 * D);
    const size_t lds = (size_t)geom.bytes_t;
    switch (S * 2 + (bps - 1)) {
#define DN_CASE(s)                                                                                  \
  case (s) * 2: hipLaunchKernelGGL((kd_nlm_t<s, 1>), grid, dim3(kThreads), lds, stream, t); break; \
  case (s) * 2 + 1: hipLaunchKernelGGL((kd_nlm_t<s, 2>), grid, dim3(kThreads), lds, stream, t); break;
      DN_CASE(1)
      DN_CASE(2)
      DN_CASE(3)
      DN_CASE(4)
#undef DN_CASE
      default: return fail(G1S_ERR_INVALID, "no kernel for this patch radius");
    }
    DN_TRY(hipGetLastError());
    return G1S_OK;
  }
  const size_t lds = (size_t)geom.bytes;
  switch (S * 2 + (bps - 1)) {
#define DN_CASE(s)                                                                          \
  case (s) * 2: hipLaunchKernelGGL((kd_nlm<s, 1>), grid, dim3(kThreads), lds, stream, p); break; \
  case (s) * 2 + 1: hipLaunchKernelGGL((kd_nlm<s, 2>), grid, dim3(kThreads), lds, stream, p); break;
    DN_CASE(1)
    DN_CASE(2)
    DN_CASE(3)
    DN_CASE(4)
#undef DN_CASE
    default: return fail(G1S_ERR_INVALID, "no kernel for this patch radius");
  }
  DN_TRY(hipGetLastError());
  return G1S_OK;
}

// frames next_launch .. next_launch + nframes - 1 as one batch (nframes <= batch); their neighbours are in the queue
int g1s_denoise::flush(uint32_t nframes) {
  if (!nframes) return G1S_OK;
  const int set = (int)(batches & 1);
  if (batches >= 2) DN_TRY(hipEventSynchronize(done[set]));
  ++batches;
  bool host_outs = false;
  for (uint32_t i = 0; i < nframes; ++i) {
    const uint64_t n = next_launch + i;
    const Queued &f = frame(n);
    DenoiseJob job{};
    for (int c = 0; c < nplanes; ++c) {
      job.in[c] = f.in[c], job.in_stride[c] = f.in_stride[c];
      job.out[c] = f.host_out ? d_stage_out + stage_frame * i + plane_off[c] : f.out[c];
      job.out_stride[c] = f.host_out ? (uint32_t)plane_row[c] : f.out_stride[c];
    }
    host_outs = host_outs || f.host_out;
    if (!D) {
      reinterpret_cast<DenoiseJob *>(h_jobs[set])[i] = job;
      continue;
    }
    DenoiseJobT t{};
    t.f = job;
    int k = 0;
    for (int64_t m = (int64_t)n - (int64_t)D; m <= (int64_t)(n + D); ++m) {
      if (m == (int64_t)n) continue;
      if (m >= (int64_t)clip_first && m < (int64_t)frames_in)  // rule 5: the frames the clip has
        for (int c = 0; c < nplanes; ++c) t.nb[c][k] = frame((uint64_t)m).in[c], t.nb_stride[c][k] = frame((uint64_t)m).in_stride[c];
      ++k;
    }
    reinterpret_cast<DenoiseJobT *>(h_jobs[set])[i] = t;
  }
  DN_TRY(hipMemcpyAsync(d_jobs[set], h_jobs[set], job_bytes() * nframes, hipMemcpyHostToDevice, stream));
  if (timing) DN_TRY(hipEventRecord(ev[0], stream));
  int rc = launch(set, nframes, 0, 1);
  if (rc) return rc;
  if (nplanes == 3 && (rc = launch(set, nframes, 1, 2)) != 0) return rc;
  if (timing) DN_TRY(hipEventRecord(ev[1], stream));
  DN_TRY(hipEventRecord(done[set], stream));
  if (host_outs)
    for (uint32_t i = 0; i < nframes; ++i) {
      const Queued &f = frame(next_launch + i);
      if (!f.host_out) continue;
      for (int c = 0; c < nplanes; ++c)
        DN_TRY(hipMemcpy2DAsync(f.host_data[c], f.host_stride[c], d_stage_out + stage_frame * i + plane_off[c], plane_row[c], pw(c) * bps, ph(c),
                                hipMemcpyDeviceToHost, stream));
    }
  if (timing) {
    DN_TRY(hipStreamSynchronize(stream));
    float a = 0;
    DN_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    ms_kernel += a, frames_timed += nframes;
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
  const int rc = launch_up_to(frames_in);
  if (rc) return rc;
  if (hipStreamSynchronize(stream) != hipSuccess) return fail(G1S_ERR_HIP, std::string("hipStreamSynchronize failed: ") + hipGetErrorString(hipGetLastError()));
  queue.clear();
  first_queued = clip_first = frames_complete = frames_in;
  return G1S_OK;
}

namespace {

// the bytes of plane c of a frame of the denoiser's geometry at `base`
bool planes_overlap(const g1s_denoise &g, const uint8_t *a, uint32_t a_stride, int ca, const uint8_t *b, uint32_t b_stride, int cb) {
  const uint8_t *ae = a + (size_t)a_stride * (g.ph(ca) - 1) + g.pw(ca) * g.bps, *be = b + (size_t)b_stride * (g.ph(cb) - 1) + g.pw(cb) * g.bps;
  return a < be && b < ae;
}

}  // namespace

extern "C" {

int g1s_denoise_weights(uint32_t bit_depth, uint32_t patch_radius, double strength, uint16_t T[1024], uint32_t *q) {
  if (!T || !q) return G1S_ERR_INVALID;
  const std::string why = make_table(bit_depth, patch_radius, strength, T, q);
  if (!why.empty()) {
    g1s_set_global_error_(why.c_str());
    return G1S_ERR_INVALID;
  }
  return G1S_OK;
}

g1s_denoise_t *g1s_denoise_new(uint32_t bit_depth, const g1s_denoise_opts_t *opts) { return g1s_denoise_new_temporal(bit_depth, opts, 0); }

g1s_denoise_t *g1s_denoise_new_temporal(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius) {
  g1s_set_global_error_("");
  if (opts && opts->struct_size != sizeof(g1s_denoise_opts_t)) {
    g1s_set_global_error_("g1s_denoise_opts_t.struct_size mismatch");
    return nullptr;
  }
  // the parameters first: a refusal needs no device
  const uint32_t A = opts && opts->search_radius ? opts->search_radius : 3u, S = opts && opts->patch_radius ? opts->patch_radius : 2u;
  const double h = opts && opts->strength != 0.0 ? opts->strength : 4.0, hc = opts && opts->chroma_strength != 0.0 ? opts->chroma_strength : h;
  if (A < 1 || A > (uint32_t)kMaxA) {
    g1s_set_global_error_("search_radius must be 1..7");
    return nullptr;
  }
  if (temporal_radius > (uint32_t)kMaxD) {
    g1s_set_global_error_("temporal_radius must be 0..3");
    return nullptr;
  }
  std::vector<uint16_t> tables(2 * kTable);
  uint32_t q[2];
  std::string why = make_table(bit_depth, S, h, tables.data(), &q[0]);
  if (why.empty()) {
    why = make_table(bit_depth, S, hc, tables.data() + kTable, &q[1]);
    if (!why.empty()) why = "chroma_" + why;
  }
  if (!why.empty()) {
    g1s_set_global_error_(why.c_str());
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g1s_set_global_error_("no HIP device available: denoise has no CPU fallback");
    return nullptr;
  }
  int device = opts ? opts->device : -1;
  if (device < 0 && hipGetDevice(&device) != hipSuccess) {
    g1s_set_global_error_("hipGetDevice failed");
    return nullptr;
  }
  g1s_denoise *g = new g1s_denoise;
  g->device = device;
  g->bit_depth = bit_depth;
  g->bps = bit_depth > 8 ? 2 : 1;
  g->batch = opts && opts->batch_frames ? std::min(opts->batch_frames, 256u) : 32u;
  g->A = A, g->S = S, g->D = temporal_radius, g->q[0] = q[0], g->q[1] = q[1];
  const size_t jobs_bytes = g->job_bytes() * g->batch;
  bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess;
  for (auto &e : g->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  for (int k = 0; k < 2; ++k)
    ok = ok && hipEventCreateWithFlags(&g->done[k], hipEventDisableTiming) == hipSuccess &&
         hipMalloc((void **)&g->d_jobs[k], jobs_bytes) == hipSuccess &&
         hipHostMalloc((void **)&g->h_jobs[k], jobs_bytes, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipMalloc((void **)&g->d_tables, tables.size() * 2) == hipSuccess &&
       hipMemcpy(g->d_tables, tables.data(), tables.size() * 2, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    g1s_set_global_error_((std::string("HIP initialisation failed: ") + hipGetErrorString(hipGetLastError())).c_str());
    g1s_denoise_free(g);
    return nullptr;
  }
  return g;
}

int g1s_denoise_frame(g1s_denoise_t *g, const g1s_frame_t *in, g1s_frame_t *out) {
  if (!g || !in || !out) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  if (in->bytes_per_sample != g->bps || out->bytes_per_sample != g->bps)
    return g->fail(G1S_ERR_INVALID, "bytes_per_sample does not match the bit depth given to g1s_denoise_new");
  if (in->width < 1 || in->height < 1 || in->width > 65536u || in->height > 65536u || (in->nplanes != 1 && in->nplanes != 3) || in->xdec > 1 ||
      in->ydec > in->xdec)
    return g->fail(G1S_ERR_INVALID, "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)");
  if (out->width != in->width || out->height != in->height || out->nplanes != in->nplanes || out->xdec != in->xdec || out->ydec != in->ydec)
    return g->fail(G1S_ERR_DIM_MISMATCH, "input and output frame geometry differ");
  if (!g->have_geom) {
    g->set_geometry(*in);
  } else if (g->W != (int)in->width || g->H != (int)in->height || g->nplanes != in->nplanes || g->subx != in->xdec || g->suby != in->ydec) {
    // a new geometry: the clip ends, what is queued goes out and finishes first, the staging buffers are sized again
    const int rc = g->end_clip();
    if (rc) return rc;
    if (g->d_stage_in) (void)hipFree(g->d_stage_in), g->d_stage_in = nullptr;
    if (g->d_stage_out) (void)hipFree(g->d_stage_out), g->d_stage_out = nullptr;
    g->set_geometry(*in);
  }
  g1s_denoise::Queued f{};
  const uint32_t slot = (uint32_t)(g->frames_in % g->ring());
  f.host_out = out->on_device != 1;
  for (int c = 0; c < g->nplanes; ++c) {
    const size_t pw = g->pw(c), ph = g->ph(c);
    if (!in->data[c] || !out->data[c] || in->stride_bytes[c] < pw * g->bps || out->stride_bytes[c] < pw * g->bps ||
        in->stride_bytes[c] > 0xffffffffu || out->stride_bytes[c] > 0xffffffffu || (g->bps == 2 && ((in->stride_bytes[c] | out->stride_bytes[c]) & 1)))
      return g->fail(G1S_ERR_INVALID, "bad plane pointer or row stride");
    if (in->on_device == 1) {
      f.in[c] = static_cast<const uint8_t *>(in->data[c]);
      f.in_stride[c] = (uint32_t)in->stride_bytes[c];
    } else {
      if (!g->d_stage_in && hipMalloc((void **)&g->d_stage_in, g->stage_frame * g->ring()) != hipSuccess)
        return g->fail(G1S_ERR_HIP, "hipMalloc of the input staging buffer failed");
      uint8_t *dst = g->d_stage_in + g->stage_frame * slot + g->plane_off[c];
      // host planes are read before the call returns (the stream copy is waited for below); pinned planes are queued
      if (hipMemcpy2DAsync(dst, g->plane_row[c], in->data[c], in->stride_bytes[c], pw * g->bps, ph, hipMemcpyHostToDevice, g->stream) != hipSuccess)
        return g->fail(G1S_ERR_HIP, "copy of an input plane to the device failed");
      f.in[c] = dst;
      f.in_stride[c] = (uint32_t)g->plane_row[c];
    }
    if (f.host_out) {
      if (!g->d_stage_out && hipMalloc((void **)&g->d_stage_out, g->stage_frame * g->batch) != hipSuccess)
        return g->fail(G1S_ERR_HIP, "hipMalloc of the output staging buffer failed");
      f.host_data[c] = const_cast<void *>(out->data[c]), f.host_stride[c] = out->stride_bytes[c];
    } else {
      f.out[c] = static_cast<uint8_t *>(const_cast<void *>(out->data[c]));
      f.out_stride[c] = (uint32_t)out->stride_bytes[c];
    }
  }
  // in != out: no device plane of the output may overlap a plane of the input -- nor, with a temporal radius, a plane the
  // queue still reads, and no plane of the input may be one that a frame of the queue is going to write
  if (!f.host_out) {
    for (int c = 0; c < g->nplanes; ++c)
      for (int d = 0; d < g->nplanes; ++d) {
        bool bad = planes_overlap(*g, f.out[c], f.out_stride[c], c, f.in[d], f.in_stride[d], d);
        if (g->D)
          for (const g1s_denoise::Queued &o : g->queue) bad = bad || planes_overlap(*g, f.out[c], f.out_stride[c], c, o.in[d], o.in_stride[d], d);
        if (bad) return g->fail(G1S_ERR_INVALID, "input and output planes overlap: g1s_denoise_frame needs distinct buffers");
      }
  }
  for (uint64_t n = g->next_launch; g->D && n < g->frames_in; ++n) {
    const g1s_denoise::Queued &o = g->frame(n);
    if (o.host_out) continue;
    for (int c = 0; c < g->nplanes; ++c)
      for (int d = 0; d < g->nplanes; ++d)
        if (planes_overlap(*g, o.out[c], o.out_stride[c], c, f.in[d], f.in_stride[d], d))
          return g->fail(G1S_ERR_INVALID, "input and output planes overlap: g1s_denoise_frame needs distinct buffers");
  }
  if (in->on_device == 0 && hipStreamSynchronize(g->stream) != hipSuccess) return g->fail(G1S_ERR_HIP, "copy of a host frame to the device failed");
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
  const int rc = g->launch_up_to(limit);
  if (rc) return rc;
  if (hipStreamSynchronize(g->stream) != hipSuccess) return g->fail(G1S_ERR_HIP, std::string("hipStreamSynchronize failed: ") + hipGetErrorString(hipGetLastError()));
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
  g->timing = enable != 0;
  if (ms_kernel) *ms_kernel = g->ms_kernel;
  if (frames) *frames = g->frames_timed;
  return G1S_OK;
}

const char *g1s_denoise_last_error(const g1s_denoise_t *g) { return g ? g->err.c_str() : ""; }

void g1s_denoise_free(g1s_denoise_t *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  void *bufs[] = {g->d_jobs[0], g->d_jobs[1], g->d_tables, g->d_stage_in, g->d_stage_out};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  for (int k = 0; k < 2; ++k) {
    if (g->h_jobs[k]) (void)hipHostFree(g->h_jobs[k]);
    if (g->done[k]) (void)hipEventDestroy(g->done[k]);
  }
  for (auto &e : g->ev)
    if (e) (void)hipEventDestroy(e);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  delete g;
}

}  // extern "C"

namespace {

// the first line of a .y4m file: goes out as it came in
std::string y4m_header_line(const char *path) {
  std::string header;
  if (FILE *f = std::fopen(path, "rb")) {
    char line[1024];
    if (std::fgets(line, sizeof line, f)) header = line;
    std::fclose(f);
  }
  return header;
}

struct PlaneLayout {
  size_t prow[3] = {0, 0, 0}, pbytes[3] = {0, 0, 0}, ph[3] = {0, 0, 0}, fbytes = 0;
  explicit PlaneLayout(const g1s_y4m_info_t &info) {
    const size_t bps = info.bit_depth > 8 ? 2 : 1;
    for (uint32_t c = 0; c < info.nplanes; ++c) {
      const size_t pw = c ? (info.width + (1u << info.xdec) - 1) >> info.xdec : info.width;
      ph[c] = c ? (info.height + (1u << info.ydec) - 1) >> info.ydec : info.height;
      prow[c] = pw * bps, pbytes[c] = pw * ph[c] * bps, fbytes += pbytes[c];
    }
  }
  // the planes of a frame stored without padding from `base`
  void point(g1s_frame_t &f, uint8_t *base, const g1s_y4m_info_t &info) const {
    size_t off = 0;
    for (uint32_t c = 0; c < info.nplanes; ++c) f.data[c] = base + off, f.stride_bytes[c] = prow[c], off += pbytes[c];
  }
};

}  // namespace

extern "C" {

int64_t g1s_denoise_y4m_file(const char *in, const char *out, const g1s_denoise_opts_t *opts, char *err, size_t cap) {
  return g1s_denoise_y4m_file_temporal(in, out, opts, 0, err, cap);
}

int64_t g1s_denoise_y4m_file_temporal(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, char *err,
                                      size_t cap) {
  auto refuse = [&](int code, const std::string &m) -> int64_t {
    if (err && cap) snprintf(err, cap, "%s", m.c_str());
    return code;
  };
  if (!in || !out) return refuse(G1S_ERR_INVALID, "null path");
  const std::string header = y4m_header_line(in);
  g1s_y4m_t *y = g1s_y4m_open(in, err, cap);
  if (!y) return G1S_ERR_INVALID;
  g1s_y4m_info_t info;
  g1s_y4m_get_info(y, &info);
  g1s_denoise_t *g = g1s_denoise_new_temporal(info.bit_depth, opts, temporal_radius);
  if (!g) {
    g1s_y4m_close(y);
    return refuse(G1S_ERR_INVALID, g1s_last_global_error());
  }
  FILE *fo = std::fopen(out, "wb");
  if (!fo) {
    g1s_denoise_free(g);
    g1s_y4m_close(y);
    return refuse(G1S_ERR_INVALID, std::string("cannot create ") + out);
  }
  const PlaneLayout lay(info);
  // a ring of output frames in pinned memory: denoised, waited for, written.  The file is one clip: between two drains a
  // batch is handed over, and the denoiser holds the last D frames back, so batch + D frames can be unwritten
  const uint32_t batch = g->batch, ring = batch + g->D;
  uint8_t *obuf = nullptr;
  int64_t frames = 0, written = 0;
  int rc = G1S_OK;
  std::string why;
  bool ok = std::fwrite(header.data(), 1, header.size(), fo) == header.size();
  if (!ok) rc = G1S_ERR_INVALID, why = std::string("cannot write ") + out;
  if (ok && hipHostMalloc((void **)&obuf, lay.fbytes * ring, hipHostMallocDefault) != hipSuccess)
    ok = false, rc = G1S_ERR_HIP, why = "hipHostMalloc of the output frames failed";
  auto drain = [&](bool end) {
    uint64_t complete = (uint64_t)frames;
    rc = end ? g1s_denoise_sync(g) : g1s_denoise_drain(g, &complete);
    if (rc) {
      why = g1s_denoise_last_error(g);
      return false;
    }
    for (; written < (int64_t)complete; ++written)
      if (std::fwrite("FRAME\n", 1, 6, fo) != 6 || std::fwrite(obuf + lay.fbytes * (size_t)(written % ring), 1, lay.fbytes, fo) != lay.fbytes) {
        rc = G1S_ERR_INVALID, why = std::string("cannot write ") + out;
        return false;
      }
    return true;
  };
  while (ok) {
    g1s_frame_t fin;
    const int got = g1s_y4m_next(y, &fin);
    if (got < 0) {
      ok = false, rc = got, why = g1s_y4m_last_error(y);
      break;
    }
    if (got == 0) break;
    g1s_frame_t fout = fin;
    lay.point(fout, obuf + lay.fbytes * (size_t)(frames % ring), info);
    fin.on_device = 0;  // (the reader lends the frame until its next call: copied before g1s_denoise_frame returns)
    fout.on_device = 2;
    rc = g1s_denoise_frame(g, &fin, &fout);
    if (rc) {
      ok = false, why = "frame " + std::to_string(frames) + ": " + g1s_denoise_last_error(g);
      break;
    }
    ++frames;
    if (frames % batch == 0) ok = drain(false);
  }
  if (ok) ok = drain(true);
  if (std::fclose(fo) != 0 && ok) ok = false, rc = G1S_ERR_INVALID, why = std::string("cannot write ") + out;
  g1s_denoise_free(g);
  if (obuf) (void)hipHostFree(obuf);
  g1s_y4m_close(y);
  if (!ok) return refuse(rc ? rc : G1S_ERR_INVALID, why);
  return frames;
}

// `diff SOURCE --denoise -o TABLE`: the source is read once and copied to the device once; the denoiser writes its
// output beside it and the generator takes the pair as device frames.  A pair's two buffers belong to the generator
// until g1s_diff_frames_released() covers the frame, and its source buffer is a neighbour of the D frames after it until the
// denoiser is past those; then they are used again.  The file is one clip: the denoiser is drained once a group, not
// synchronised, and only the frames it has completed go on to the generator.
int g1s_diff_y4m_file_denoised(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                               const g1s_denoise_opts_t *dopts, uint64_t *frames_out, char *err, size_t cap) {
  return g1s_diff_y4m_file_denoised_temporal(source, out_tbl, keep_denoised, opts, dopts, 0, frames_out, err, cap);
}

int g1s_diff_y4m_file_denoised_temporal(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                        const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint64_t *frames_out, char *err, size_t cap) {
  auto refuse = [&](int code, const std::string &m) {
    if (err && cap) snprintf(err, cap, "%s", m.c_str());
    return code;
  };
  if (frames_out) *frames_out = 0;
  if (!source || !out_tbl) return refuse(G1S_ERR_INVALID, "null path");
  const std::string header = y4m_header_line(source);
  g1s_y4m_t *y = g1s_y4m_open(source, err, cap);
  if (!y) return G1S_ERR_INVALID;
  g1s_y4m_info_t info;
  g1s_y4m_get_info(y, &info);
  const PlaneLayout lay(info);
  g1s_diff_t *g = nullptr;
  g1s_denoise_t *dn = nullptr;
  FILE *fk = nullptr;
  uint8_t *kbuf = nullptr;
  struct Pair {
    uint8_t *src = nullptr, *den = nullptr;
  };
  std::vector<Pair> pairs;                          // every pair of buffers allocated so far
  std::deque<std::pair<uint64_t, size_t>> lent;     // (frame index, pair) handed to the generator, oldest first
  std::deque<size_t> held;                          // pairs of the frames the denoiser has not completed, oldest first
  std::vector<size_t> spare;
  size_t pair_cap = 0;
  uint64_t frames = 0, taken = 0, complete = 0;     // frames handed to the generator; to the denoiser; completed by it
  uint32_t D = 0;
  int rc = G1S_OK;
  std::string why;
  std::vector<g1s_segment_t> segs(64);
  size_t nseg = 0;

  g = g1s_diff_new(info.fps_num, info.fps_den, info.bit_depth, info.bit_depth, opts);
  if (!g) {
    rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
    goto done;
  }
  {
    g1s_denoise_opts_t d{};
    if (dopts) d = *dopts;
    d.struct_size = sizeof d;
    d.device = g1s_diff_device_(g);  // one device: the pair never leaves it
    dn = g1s_denoise_new_temporal(info.bit_depth, &d, temporal_radius);
  }
  if (!dn) {
    rc = G1S_ERR_INVALID, why = g1s_last_global_error();
    goto done;
  }
  (void)hipSetDevice(g1s_diff_device_(g));
  if (keep_denoised) {
    fk = std::fopen(keep_denoised, "wb");
    if (!fk || std::fwrite(header.data(), 1, header.size(), fk) != header.size() ||
        hipHostMalloc((void **)&kbuf, lay.fbytes, hipHostMallocDefault) != hipSuccess) {
      rc = G1S_ERR_INVALID, why = std::string("cannot write ") + keep_denoised;
      goto done;
    }
  }
  // buffers for two groups until the generator has said how many frames it can hold (after the first hand-over), and for
  // the window: the D frames the denoiser holds back and the D before them that are still their neighbours
  D = dn->D;
  pair_cap = 2 * (size_t)dn->batch + 2 * D;
  for (bool eof = false; !eof && !rc;) {
    // ---- one group: up to batch_frames frames to the device and to the denoiser
    for (uint32_t in_group = 0; in_group < dn->batch; ++in_group) {
      g1s_frame_t fin;
      const int got = g1s_y4m_next(y, &fin);
      if (got < 0) {
        rc = got, why = "frame " + std::to_string(taken) + ": source reader failed (" + g1s_y4m_last_error(y) + ")";
        break;
      }
      if (got == 0) {
        eof = true;
        break;
      }
      // a pair of buffers: one that the generator has released and the denoiser is past (frame t + D complete), a new one,
      // or -- the ring is full -- wait for the generator
      size_t k;
      uint64_t released = g1s_diff_frames_released(g);
      auto reclaim = [&] {
        while (!lent.empty() && lent.front().first < released && lent.front().first + D < complete) spare.push_back(lent.front().second), lent.pop_front();
      };
      reclaim();
      if (spare.empty() && pairs.size() >= pair_cap) {
        rc = g1s_diff_sync(g);
        if (rc) {
          why = std::string("diff_frame: ") + g1s_diff_last_error(g);
          break;
        }
        released = frames;
        reclaim();
      }
      if (!spare.empty()) {
        k = spare.back(), spare.pop_back();
      } else {
        Pair p;
        if (hipMalloc((void **)&p.src, lay.fbytes) != hipSuccess || hipMalloc((void **)&p.den, lay.fbytes) != hipSuccess) {
          if (p.src) (void)hipFree(p.src);
          rc = G1S_ERR_HIP, why = "hipMalloc of a frame pair failed";
          break;
        }
        pairs.push_back(p), k = pairs.size() - 1;
      }
      // the reader lends the frame until its next call: on the device before that
      size_t off = 0;
      bool copied = true;
      for (uint32_t c = 0; c < info.nplanes; ++c) {
        copied = copied && hipMemcpy2D(pairs[k].src + off, lay.prow[c], fin.data[c], fin.stride_bytes[c], lay.prow[c], lay.ph[c], hipMemcpyHostToDevice) == hipSuccess;
        off += lay.pbytes[c];
      }
      if (!copied) {
        rc = G1S_ERR_HIP, why = "copy of a source frame to the device failed";
        break;
      }
      g1s_frame_t s = fin, d = fin;
      lay.point(s, pairs[k].src, info), lay.point(d, pairs[k].den, info);
      s.on_device = d.on_device = 1;
      rc = g1s_denoise_frame(dn, &s, &d);
      if (rc) {
        why = "frame " + std::to_string(taken) + ": denoise: " + g1s_denoise_last_error(dn);
        break;
      }
      held.push_back(k), ++taken;
    }
    if (rc) break;
    // the end of the file is the end of the clip; before it the last D frames stay with the denoiser
    rc = eof ? g1s_denoise_sync(dn) : g1s_denoise_drain(dn, &complete);
    if (rc) {
      why = std::string("denoise: ") + g1s_denoise_last_error(dn);
      break;
    }
    if (eof) complete = taken;
    // ---- the completed frames' pairs to the generator, the denoised frames to the kept file
    while (frames < complete) {
      const size_t k = held.front();
      held.pop_front();
      g1s_frame_t s{}, d{};
      s.width = info.width, s.height = info.height, s.bytes_per_sample = info.bit_depth > 8 ? 2 : 1, s.xdec = (uint8_t)info.xdec, s.ydec = (uint8_t)info.ydec,
      s.nplanes = (uint8_t)info.nplanes, s.on_device = 1;
      d = s;
      lay.point(s, pairs[k].src, info), lay.point(d, pairs[k].den, info);
      rc = g1s_diff_frame(g, &s, &d);
      if (rc) {
        why = "frame " + std::to_string(frames) + ": diff_frame: " + g1s_diff_last_error(g);
        break;
      }
      lent.emplace_back(frames, k);
      if (fk && (hipMemcpy(kbuf, pairs[k].den, lay.fbytes, hipMemcpyDeviceToHost) != hipSuccess || std::fwrite("FRAME\n", 1, 6, fk) != 6 ||
                 std::fwrite(kbuf, 1, lay.fbytes, fk) != lay.fbytes)) {
        rc = G1S_ERR_INVALID, why = std::string("cannot write ") + keep_denoised;
        break;
      }
      ++frames;
    }
    if (rc) break;
    if (const uint32_t inside = g1s_diff_frames_in_flight_max_(g)) pair_cap = std::max(pair_cap, (size_t)dn->batch + inside + inside / 4 + 2 * D);
  }
  if (rc) goto done;
  rc = g1s_diff_finish(g, segs.data(), segs.size(), &nseg);
  if (rc == G1S_ERR_CAPACITY) {
    segs.resize(nseg);
    rc = g1s_diff_finish(g, segs.data(), segs.size(), &nseg);
  }
  if (rc) {
    why = g1s_diff_last_error(g);
    goto done;
  }
  rc = g1s_write_tbl(out_tbl, segs.data(), nseg);
  if (rc) why = std::string("cannot write ") + out_tbl;
done:
  if (fk && std::fclose(fk) != 0 && !rc) rc = G1S_ERR_INVALID, why = std::string("cannot write ") + keep_denoised;
  if (dn) g1s_denoise_free(dn);
  if (g) g1s_diff_free(g);  // (waits for the kernels that read the pairs)
  for (Pair &p : pairs) (void)hipFree(p.src), (void)hipFree(p.den);
  if (kbuf) (void)hipHostFree(kbuf);
  g1s_y4m_close(y);
  if (frames_out) *frames_out = frames;
  if (rc) return refuse(rc, why);
  return G1S_OK;
}

}  // extern "C"
