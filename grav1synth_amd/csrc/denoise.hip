// denoise.hip -- `denoise`: the project's integer-exact non-local-means filter on the device.
//
// The filter is defined in include/g1s_diff.h ("denoise", rules 1 - 4); tests/denoise_ref.py restates it in numpy.  It is
// this project's own definition of non-local means: ffmpeg's nlmeans and KNLMeansCL have the same structure, not the
// same bits.  One kernel, kd_nlm<S, BPS>: a workgroup per (tile, plane of the class, frame), the phases of
// denoise_tile.hip.h.  A batch of frames goes out as one launch per plane class (luma; the two chroma planes) on the
// denoiser's own stream.  Planes are independent, but `out` must not overlap `in`: a tile reads the halo its neighbours
// write.
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
  uint32_t A = 3, S = 2;
  uint32_t q[2] = {0, 0};  // luma, chroma
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool have_geom = false;
  int W = 0, H = 0, subx = 0, suby = 0, nplanes = 0;
  size_t plane_row[3] = {0, 0, 0}, plane_off[3] = {0, 0, 0}, stage_frame = 0;  // staging layout of a host frame on the device
  std::vector<DenoiseJob> jobs;  // the batch being filled
  struct HostOut {
    uint32_t slot;
    void *data[3];
    size_t stride[3];
  };
  std::vector<HostOut> host_outs;  // frames whose out planes are host memory: copied back behind the kernels
  // the jobs of a batch, two sets in turn: pinned on the host, uploaded on the stream, free again when the event behind
  // the batch's kernels has passed -- the next batch is filled while this one runs
  DenoiseJob *d_jobs[2] = {nullptr, nullptr}, *h_jobs[2] = {nullptr, nullptr};
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
  void set_geometry(const g1s_frame_t &f);
  int launch(int set, uint32_t nframes, int plane0, int nplanes_in_class);
  int flush();
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
  p.jobs = d_jobs[set], p.table = d_tables + (plane0 ? kTable : 0), p.q = (int)q[plane0 ? 1 : 0], p.A = (int)A;
  p.W = (int)pw(plane0), p.H = (int)ph(plane0), p.tiles_x = (p.W + kTW - 1) / kTW, p.plane0 = plane0;
  const dim3 grid((unsigned)(p.tiles_x * ((p.H + kTH - 1) / kTH)), (unsigned)nplanes_in_class, nframes);
  const size_t lds = (size_t)tile_geom((int)A, (int)S).bytes;
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

int g1s_denoise::flush() {
  const uint32_t B = (uint32_t)jobs.size();
  if (!B) return G1S_OK;
  const int set = (int)(batches & 1);
  if (batches >= 2) DN_TRY(hipEventSynchronize(done[set]));
  ++batches;
  std::memcpy(h_jobs[set], jobs.data(), sizeof(DenoiseJob) * B);
  DN_TRY(hipMemcpyAsync(d_jobs[set], h_jobs[set], sizeof(DenoiseJob) * B, hipMemcpyHostToDevice, stream));
  if (timing) DN_TRY(hipEventRecord(ev[0], stream));
  int rc = launch(set, B, 0, 1);
  if (rc) return rc;
  if (nplanes == 3 && (rc = launch(set, B, 1, 2)) != 0) return rc;
  if (timing) DN_TRY(hipEventRecord(ev[1], stream));
  DN_TRY(hipEventRecord(done[set], stream));
  for (const HostOut &h : host_outs)
    for (int c = 0; c < nplanes; ++c)
      DN_TRY(hipMemcpy2DAsync(h.data[c], h.stride[c], d_stage_out + stage_frame * h.slot + plane_off[c], plane_row[c], pw(c) * bps, ph(c),
                              hipMemcpyDeviceToHost, stream));
  if (timing) {
    DN_TRY(hipStreamSynchronize(stream));
    float a = 0;
    DN_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    ms_kernel += a, frames_timed += B;
  }
  jobs.clear();
  host_outs.clear();
  return G1S_OK;
}

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

g1s_denoise_t *g1s_denoise_new(uint32_t bit_depth, const g1s_denoise_opts_t *opts) {
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
  g->A = A, g->S = S, g->q[0] = q[0], g->q[1] = q[1];
  const uint32_t B = g->batch;
  bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess;
  for (auto &e : g->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  for (int k = 0; k < 2; ++k)
    ok = ok && hipEventCreateWithFlags(&g->done[k], hipEventDisableTiming) == hipSuccess &&
         hipMalloc((void **)&g->d_jobs[k], sizeof(DenoiseJob) * B) == hipSuccess &&
         hipHostMalloc((void **)&g->h_jobs[k], sizeof(DenoiseJob) * B, hipHostMallocDefault) == hipSuccess;
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
    // a new geometry: what is queued goes out and finishes first, the staging buffers are sized again
    const int rc = g->flush();
    if (rc) return rc;
    if (hipStreamSynchronize(g->stream) != hipSuccess) return g->fail(G1S_ERR_HIP, "hipStreamSynchronize failed");
    if (g->d_stage_in) (void)hipFree(g->d_stage_in), g->d_stage_in = nullptr;
    if (g->d_stage_out) (void)hipFree(g->d_stage_out), g->d_stage_out = nullptr;
    g->set_geometry(*in);
  }
  DenoiseJob job{};
  const uint32_t slot = (uint32_t)g->jobs.size();
  for (int c = 0; c < g->nplanes; ++c) {
    const size_t pw = g->pw(c), ph = g->ph(c);
    if (!in->data[c] || !out->data[c] || in->stride_bytes[c] < pw * g->bps || out->stride_bytes[c] < pw * g->bps ||
        in->stride_bytes[c] > 0xffffffffu || out->stride_bytes[c] > 0xffffffffu || (g->bps == 2 && ((in->stride_bytes[c] | out->stride_bytes[c]) & 1)))
      return g->fail(G1S_ERR_INVALID, "bad plane pointer or row stride");
    if (in->on_device == 1) {
      job.in[c] = static_cast<const uint8_t *>(in->data[c]);
      job.in_stride[c] = (uint32_t)in->stride_bytes[c];
    } else {
      if (!g->d_stage_in && hipMalloc((void **)&g->d_stage_in, g->stage_frame * g->batch) != hipSuccess)
        return g->fail(G1S_ERR_HIP, "hipMalloc of the input staging buffer failed");
      uint8_t *dst = g->d_stage_in + g->stage_frame * slot + g->plane_off[c];
      // host planes are read before the call returns (the stream copy is waited for below); pinned planes are queued
      if (hipMemcpy2DAsync(dst, g->plane_row[c], in->data[c], in->stride_bytes[c], pw * g->bps, ph, hipMemcpyHostToDevice, g->stream) != hipSuccess)
        return g->fail(G1S_ERR_HIP, "copy of an input plane to the device failed");
      job.in[c] = dst;
      job.in_stride[c] = (uint32_t)g->plane_row[c];
    }
    if (out->on_device == 1) {
      job.out[c] = static_cast<uint8_t *>(const_cast<void *>(out->data[c]));
      job.out_stride[c] = (uint32_t)out->stride_bytes[c];
    } else {
      if (!g->d_stage_out && hipMalloc((void **)&g->d_stage_out, g->stage_frame * g->batch) != hipSuccess)
        return g->fail(G1S_ERR_HIP, "hipMalloc of the output staging buffer failed");
      job.out[c] = g->d_stage_out + g->stage_frame * slot + g->plane_off[c];
      job.out_stride[c] = (uint32_t)g->plane_row[c];
    }
  }
  // in != out: no plane of the output may overlap a plane of the input
  for (int c = 0; c < g->nplanes; ++c) {
    const uint8_t *ob = job.out[c], *oe = ob + (size_t)job.out_stride[c] * (g->ph(c) - 1) + g->pw(c) * g->bps;
    for (int d = 0; d < g->nplanes; ++d) {
      const uint8_t *ib = job.in[d], *ie = ib + (size_t)job.in_stride[d] * (g->ph(d) - 1) + g->pw(d) * g->bps;
      if (ob < ie && ib < oe) return g->fail(G1S_ERR_INVALID, "input and output planes overlap: g1s_denoise_frame needs distinct buffers");
    }
  }
  if (in->on_device == 0 && hipStreamSynchronize(g->stream) != hipSuccess) return g->fail(G1S_ERR_HIP, "copy of a host frame to the device failed");
  if (out->on_device != 1) {
    g1s_denoise::HostOut h{};
    h.slot = slot;
    for (int c = 0; c < g->nplanes; ++c) h.data[c] = const_cast<void *>(out->data[c]), h.stride[c] = out->stride_bytes[c];
    g->host_outs.push_back(h);
  }
  g->jobs.push_back(job);
  return g->jobs.size() >= g->batch ? g->flush() : G1S_OK;
}

int g1s_denoise_sync(g1s_denoise_t *g) {
  if (!g) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  const int rc = g->flush();
  if (rc) return rc;
  if (hipStreamSynchronize(g->stream) != hipSuccess) return g->fail(G1S_ERR_HIP, std::string("hipStreamSynchronize failed: ") + hipGetErrorString(hipGetLastError()));
  return G1S_OK;
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
  g1s_denoise_t *g = g1s_denoise_new(info.bit_depth, opts);
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
  // a batch of output frames in pinned memory: denoised, waited for, written
  const uint32_t batch = g->batch;
  uint8_t *obuf = nullptr;
  int64_t frames = 0;
  int rc = G1S_OK;
  std::string why;
  bool ok = std::fwrite(header.data(), 1, header.size(), fo) == header.size();
  if (!ok) rc = G1S_ERR_INVALID, why = std::string("cannot write ") + out;
  if (ok && hipHostMalloc((void **)&obuf, lay.fbytes * batch, hipHostMallocDefault) != hipSuccess)
    ok = false, rc = G1S_ERR_HIP, why = "hipHostMalloc of the output frames failed";
  uint32_t pending = 0;
  auto drain = [&]() {
    rc = g1s_denoise_sync(g);
    if (rc) {
      why = g1s_denoise_last_error(g);
      return false;
    }
    for (uint32_t k = 0; k < pending; ++k)
      if (std::fwrite("FRAME\n", 1, 6, fo) != 6 || std::fwrite(obuf + lay.fbytes * k, 1, lay.fbytes, fo) != lay.fbytes) {
        rc = G1S_ERR_INVALID, why = std::string("cannot write ") + out;
        return false;
      }
    pending = 0;
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
    lay.point(fout, obuf + lay.fbytes * pending, info);
    fin.on_device = 0;  // (the reader lends the frame until its next call: copied before g1s_denoise_frame returns)
    fout.on_device = 2;
    rc = g1s_denoise_frame(g, &fin, &fout);
    if (rc) {
      ok = false, why = "frame " + std::to_string(frames) + ": " + g1s_denoise_last_error(g);
      break;
    }
    ++frames, ++pending;
    if (pending == batch) ok = drain();
  }
  if (ok) ok = drain();
  if (std::fclose(fo) != 0 && ok) ok = false, rc = G1S_ERR_INVALID, why = std::string("cannot write ") + out;
  g1s_denoise_free(g);
  if (obuf) (void)hipHostFree(obuf);
  g1s_y4m_close(y);
  if (!ok) return refuse(rc ? rc : G1S_ERR_INVALID, why);
  return frames;
}

// `diff SOURCE --denoise -o TABLE`: the source is read once and copied to the device once; the denoiser writes its
// output beside it and the generator takes the pair as device frames.  A pair's two buffers belong to the generator
// until g1s_diff_frames_released() covers the frame; then they are used again.
int g1s_diff_y4m_file_denoised(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                               const g1s_denoise_opts_t *dopts, uint64_t *frames_out, char *err, size_t cap) {
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
  std::vector<size_t> group;                        // pairs of the frames the denoiser holds
  std::vector<size_t> spare;
  size_t pair_cap = 0;
  uint64_t frames = 0;
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
    dn = g1s_denoise_new(info.bit_depth, &d);
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
  // buffers for two groups until the generator has said how many frames it can hold (after the first hand-over)
  pair_cap = 2 * (size_t)dn->batch;
  for (bool eof = false; !eof && !rc;) {
    // ---- one group: up to batch_frames frames to the device and through the denoiser
    group.clear();
    while (group.size() < dn->batch) {
      g1s_frame_t fin;
      const int got = g1s_y4m_next(y, &fin);
      if (got < 0) {
        rc = got, why = "frame " + std::to_string(frames + group.size()) + ": source reader failed (" + g1s_y4m_last_error(y) + ")";
        break;
      }
      if (got == 0) {
        eof = true;
        break;
      }
      // a pair of buffers: one the generator has released, a new one, or -- the ring is full -- wait for the generator
      size_t k;
      const uint64_t released = g1s_diff_frames_released(g);
      while (!lent.empty() && lent.front().first < released) spare.push_back(lent.front().second), lent.pop_front();
      if (spare.empty() && pairs.size() >= pair_cap) {
        rc = g1s_diff_sync(g);
        if (rc) {
          why = std::string("diff_frame: ") + g1s_diff_last_error(g);
          break;
        }
        while (!lent.empty()) spare.push_back(lent.front().second), lent.pop_front();
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
        why = "frame " + std::to_string(frames + group.size()) + ": denoise: " + g1s_denoise_last_error(dn);
        break;
      }
      group.push_back(k);
    }
    if (rc) break;
    rc = g1s_denoise_sync(dn);
    if (rc) {
      why = std::string("denoise: ") + g1s_denoise_last_error(dn);
      break;
    }
    // ---- the group's pairs to the generator, the denoised frames to the kept file
    for (size_t k : group) {
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
    if (const uint32_t inside = g1s_diff_frames_in_flight_max_(g)) pair_cap = std::max(pair_cap, (size_t)dn->batch + inside + inside / 4);
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
