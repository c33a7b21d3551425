// surface.hip -- decoder surfaces to frames and back: NV12, P010 / P012 / P016, MSB-aligned planes <-> g1s_frame_t.
//
// The layouts and the six rules are in include/g1s_diff.h ("decoder surfaces"); tests/surface_ref.py restates them in
// numpy.  A permutation and a shift of integers, bound by HBM and nothing else.  Two kernels, one launch a batch:
//
//   ks_unpack<BPS>  surface -> frame      ks_pack<BPS>  frame -> surface
//
// A workgroup takes kStripRows consecutive rows of the frame's row list -- the luma rows, then the rows of the interleaved
// plane (each gives a Cb and a Cr row), or the Cb rows and then the Cr rows of a planar surface -- a wave a row at a time,
// its lanes along the row.  Per row the wave picks its path (uniform: base and pitch decide):
//   fast    every address of the row on either side is 16-byte aligned: a lane moves 16 bytes a plane and step as dwordx4
//           (the interleaved plane: 32 bytes against 16 + 16), de-interleaved with v_perm_b32 (bytes at 8 bits, halves at
//           16), two samples shifted by one 32-bit shift and a mask; the ragged end of the row sample by sample.
//   slow    anything else: sample by sample, consecutive lanes on consecutive samples.
// No LDS, no byte written outside the rows' samples.  Row times stride is formed in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "frame_op.h"

// (a build switch for the measurement of DESIGN 4.12, `make variant NAME=nt DEFS=-DG1S_SURFACE_NT=1`: non-temporal loads and stores)
#ifndef G1S_SURFACE_NT
#define G1S_SURFACE_NT 0
#endif

namespace {

constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kStripRows = 16;  // rows a workgroup: 4 a wave
constexpr int kAhead = 4;       // 16-byte loads a lane has in flight before its first store

enum : uint32_t { kNoChroma = 0, kInterleaved = 1, kPlanar = 2 };

// one frame of a batch.  s: the surface's planes (1, 2 or 3), f: the frame's (1 or 3); which is read says the kernel
struct SurfJob {
  uint8_t *s[3], *f[3];
  uint32_t s_stride[3], f_stride[3];  // bytes
};

struct SurfParams {
  const SurfJob *jobs;
  uint32_t W, H, cw, ch;  // luma and chroma size in samples
  uint32_t sh;            // rule 2
  uint32_t chroma;        // kNoChroma, kInterleaved, kPlanar
};

// the planes are HBM: global, not flat, addresses
#define G1S_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef G1S_GLOBAL u32x4 *gptr_u4;
typedef G1S_GLOBAL uint8_t *gptr_u8;
typedef G1S_GLOBAL uint16_t *gptr_u16;

__device__ __forceinline__ u32x4 load16(const uint8_t *p) {
  gptr_u4 g = (gptr_u4)(uintptr_t)p;
  return G1S_SURFACE_NT ? __builtin_nontemporal_load(g) : *g;
}
__device__ __forceinline__ void store16(uint8_t *p, u32x4 v) {
  gptr_u4 g = (gptr_u4)(uintptr_t)p;
  if (G1S_SURFACE_NT) __builtin_nontemporal_store(v, g);
  else *g = v;
}
template <int BPS>
__device__ __forceinline__ uint32_t load1(const uint8_t *row, uint32_t x) {
  return BPS == 2 ? (uint32_t)((gptr_u16)(uintptr_t)row)[x] : (uint32_t)((gptr_u8)(uintptr_t)row)[x];
}
template <int BPS>
__device__ __forceinline__ void store1(uint8_t *row, uint32_t x, uint32_t v) {
  if (BPS == 2) ((gptr_u16)(uintptr_t)row)[x] = (uint16_t)v;
  else ((gptr_u8)(uintptr_t)row)[x] = (uint8_t)v;
}

// Rules 3 and 4 on one sample and on the two samples of a 32-bit word (sh == 0: the word as it is).  One-byte samples have no shift.
template <int BPS, bool UNPACK>
__device__ __forceinline__ uint32_t shift1(uint32_t v, uint32_t sh) {
  if (BPS == 1) return v;
  return UNPACK ? v >> sh : (v << sh) & 0xffffu;
}
template <int BPS, bool UNPACK>
__device__ __forceinline__ uint32_t shift2(uint32_t w, uint32_t sh) {
  if (BPS == 1) return w;
  return UNPACK ? (w >> sh) & ((0xffffu >> sh) * 0x10001u) : (w << sh) & (((0xffffu << sh) & 0xffffu) * 0x10001u);
}
template <int BPS, bool UNPACK>
__device__ __forceinline__ u32x4 shift8(u32x4 v, uint32_t sh) {
  if (BPS == 1) return v;
  u32x4 r;
  r.x = shift2<BPS, UNPACK>(v.x, sh), r.y = shift2<BPS, UNPACK>(v.y, sh), r.z = shift2<BPS, UNPACK>(v.z, sh), r.w = shift2<BPS, UNPACK>(v.w, sh);
  return r;
}

// v_perm_b32 of the eight bytes {hi, lo}: selector bytes 0 .. 3 take lo's, 4 .. 7 hi's.
//   apart:    the even (first) / odd (second) samples of two words of pairs
//   together: the pairs made of the low / high halves of two words of samples
template <int BPS> struct Sel;
template <> struct Sel<1> { static constexpr uint32_t first = 0x06040200u, second = 0x07050301u, low = 0x05010400u, high = 0x07030602u; };
template <> struct Sel<2> { static constexpr uint32_t first = 0x05040100u, second = 0x07060302u, low = 0x05040100u, high = 0x07060302u; };

// A row of n samples, plane to plane.
template <int BPS, bool UNPACK>
__device__ __forceinline__ void copy_row(const uint8_t *src, uint8_t *dst, uint32_t n, uint32_t sh, uint32_t lane) {
  uint32_t done = 0;
  if (((((uintptr_t)src | (uintptr_t)dst)) & 15) == 0) {
    const uint32_t nvec = (n * BPS) >> 4;
    uint32_t i = lane;
    for (; i + 64 * (kAhead - 1) < nvec; i += 64 * kAhead) {
      u32x4 v[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) v[k] = load16(src + (size_t)(i + 64 * k) * 16);
#pragma unroll
      for (int k = 0; k < kAhead; ++k) store16(dst + (size_t)(i + 64 * k) * 16, shift8<BPS, UNPACK>(v[k], sh));
    }
    for (; i < nvec; i += 64) store16(dst + (size_t)i * 16, shift8<BPS, UNPACK>(load16(src + (size_t)i * 16), sh));
    done = nvec * (16 / BPS);
  }
  for (uint32_t x = done + lane; x < n; x += 64) store1<BPS>(dst, x, shift1<BPS, UNPACK>(load1<BPS>(src, x), sh));
}

// A row of n Cb, Cr pairs apart: 32 bytes of pairs into 16 of Cb and 16 of Cr a lane and step.
template <int BPS>
__device__ __forceinline__ void split_row(const uint8_t *src, uint8_t *cb, uint8_t *cr, uint32_t n, uint32_t sh, uint32_t lane) {
  uint32_t done = 0;
  if (((((uintptr_t)src | (uintptr_t)cb | (uintptr_t)cr)) & 15) == 0) {
    const uint32_t nvec = (n * BPS) >> 4;
    for (uint32_t i = lane; i < nvec; i += 64 * 2) {
      const bool two = i + 64 < nvec;
      u32x4 a[2], b[2];
      a[0] = load16(src + (size_t)i * 32), b[0] = load16(src + (size_t)i * 32 + 16);
      if (two) a[1] = load16(src + (size_t)(i + 64) * 32), b[1] = load16(src + (size_t)(i + 64) * 32 + 16);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (k && !two) break;
        u32x4 u, v;
        u.x = __builtin_amdgcn_perm(a[k].y, a[k].x, Sel<BPS>::first), v.x = __builtin_amdgcn_perm(a[k].y, a[k].x, Sel<BPS>::second);
        u.y = __builtin_amdgcn_perm(a[k].w, a[k].z, Sel<BPS>::first), v.y = __builtin_amdgcn_perm(a[k].w, a[k].z, Sel<BPS>::second);
        u.z = __builtin_amdgcn_perm(b[k].y, b[k].x, Sel<BPS>::first), v.z = __builtin_amdgcn_perm(b[k].y, b[k].x, Sel<BPS>::second);
        u.w = __builtin_amdgcn_perm(b[k].w, b[k].z, Sel<BPS>::first), v.w = __builtin_amdgcn_perm(b[k].w, b[k].z, Sel<BPS>::second);
        store16(cb + (size_t)(i + 64 * k) * 16, shift8<BPS, true>(u, sh));
        store16(cr + (size_t)(i + 64 * k) * 16, shift8<BPS, true>(v, sh));
      }
    }
    done = nvec * (16 / BPS);
  }
  for (uint32_t x = done + lane; x < n; x += 64) {
    store1<BPS>(cb, x, shift1<BPS, true>(load1<BPS>(src, 2 * x), sh));
    store1<BPS>(cr, x, shift1<BPS, true>(load1<BPS>(src, 2 * x + 1), sh));
  }
}

// A row of n Cb and n Cr samples together: the reverse.
template <int BPS>
__device__ __forceinline__ void join_row(const uint8_t *cb, const uint8_t *cr, uint8_t *dst, uint32_t n, uint32_t sh, uint32_t lane) {
  uint32_t done = 0;
  if (((((uintptr_t)dst | (uintptr_t)cb | (uintptr_t)cr)) & 15) == 0) {
    const uint32_t nvec = (n * BPS) >> 4;
    for (uint32_t i = lane; i < nvec; i += 64 * 2) {
      const bool two = i + 64 < nvec;
      u32x4 u[2], v[2];
      u[0] = load16(cb + (size_t)i * 16), v[0] = load16(cr + (size_t)i * 16);
      if (two) u[1] = load16(cb + (size_t)(i + 64) * 16), v[1] = load16(cr + (size_t)(i + 64) * 16);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (k && !two) break;
        const u32x4 c = shift8<BPS, false>(u[k], sh), r = shift8<BPS, false>(v[k], sh);
        u32x4 a, b;
        a.x = __builtin_amdgcn_perm(r.x, c.x, Sel<BPS>::low), a.y = __builtin_amdgcn_perm(r.x, c.x, Sel<BPS>::high);
        a.z = __builtin_amdgcn_perm(r.y, c.y, Sel<BPS>::low), a.w = __builtin_amdgcn_perm(r.y, c.y, Sel<BPS>::high);
        b.x = __builtin_amdgcn_perm(r.z, c.z, Sel<BPS>::low), b.y = __builtin_amdgcn_perm(r.z, c.z, Sel<BPS>::high);
        b.z = __builtin_amdgcn_perm(r.w, c.w, Sel<BPS>::low), b.w = __builtin_amdgcn_perm(r.w, c.w, Sel<BPS>::high);
        store16(dst + (size_t)(i + 64 * k) * 32, a);
        store16(dst + (size_t)(i + 64 * k) * 32 + 16, b);
      }
    }
    done = nvec * (16 / BPS);
  }
  for (uint32_t x = done + lane; x < n; x += 64) {
    store1<BPS>(dst, 2 * x, shift1<BPS, false>(load1<BPS>(cb, x), sh));
    store1<BPS>(dst, 2 * x + 1, shift1<BPS, false>(load1<BPS>(cr, x), sh));
  }
}

// rows of the frame's row list: H luma rows, then ch rows of pairs or 2 ch planar chroma rows
__host__ __device__ inline uint32_t row_count(uint32_t H, uint32_t ch, uint32_t chroma) { return H + (chroma == kInterleaved ? ch : chroma == kPlanar ? 2 * ch : 0u); }

template <int BPS, bool UNPACK>
__device__ __forceinline__ void convert(const SurfParams &p) {
  const SurfJob &job = p.jobs[blockIdx.y];
  const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t rows = row_count(p.H, p.ch, p.chroma);
  constexpr uint32_t kRowsPerWave = kStripRows / kWaves;
  for (uint32_t k = 0; k < kRowsPerWave; ++k) {
    const uint32_t t = blockIdx.x * kStripRows + k * kWaves + wave;  // (uniform over the wave)
    if (t >= rows) break;
    if (t < p.H) {
      uint8_t *s = job.s[0] + (size_t)t * job.s_stride[0], *f = job.f[0] + (size_t)t * job.f_stride[0];
      copy_row<BPS, UNPACK>(UNPACK ? s : f, UNPACK ? f : s, p.W, p.sh, lane);
    } else if (p.chroma == kPlanar) {
      const uint32_t c = t - p.H < p.ch ? 1 : 2, y = t - p.H - (c - 1) * p.ch;
      uint8_t *s = job.s[c] + (size_t)y * job.s_stride[c], *f = job.f[c] + (size_t)y * job.f_stride[c];
      copy_row<BPS, UNPACK>(UNPACK ? s : f, UNPACK ? f : s, p.cw, p.sh, lane);
    } else {
      const uint32_t y = t - p.H;
      uint8_t *s = job.s[1] + (size_t)y * job.s_stride[1];
      uint8_t *cb = job.f[1] + (size_t)y * job.f_stride[1], *cr = job.f[2] + (size_t)y * job.f_stride[2];
      if (UNPACK) split_row<BPS>(s, cb, cr, p.cw, p.sh, lane);
      else join_row<BPS>(cb, cr, s, p.cw, p.sh, lane);
    }
  }
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void ks_unpack(SurfParams p) { convert<BPS, true>(p); }
template <int BPS>
__global__ __launch_bounds__(kThreads) void ks_pack(SurfParams p) { convert<BPS, false>(p); }

}  // namespace

// =============================================================== host engine =====
using namespace g1s_op;

struct g1s_surface_conv : BatchedOp {
  Event ev[2];
  // what the queued frames have in common: a call that differs in any of it drains the queue first
  bool unpack = true;
  uint32_t surface_planes = 0, msb_aligned = 0;
  std::vector<SurfJob> jobs;  // the batch being filled
  ParamSets<SurfJob> p_jobs;
  struct HostOut {
    uint32_t slot;
    HostPlanes planes;
  };
  std::vector<HostOut> host_outs;  // frames whose out planes are host memory: copied back behind the kernel
  double ms_kernel = 0;
  uint64_t frames_timed = 0;

  int flush();
  int convert(const g1s_surface_t &s, const g1s_frame_t &f, bool unpack_);
};

// the queued frames as one launch, the host outputs copied back behind it
int g1s_surface_conv::flush() {
  const uint32_t B = (uint32_t)jobs.size();
  if (!B) return G1S_OK;
  int set, rc = next_set(&set);
  if (rc) return rc;
  std::memcpy(p_jobs.h[set], jobs.data(), sizeof(SurfJob) * B);
  G1S_OP_TRY(p_jobs.upload(set, B, stream));
  SurfParams sp{};
  sp.jobs = p_jobs.d[set];
  sp.W = (uint32_t)geom.W, sp.H = (uint32_t)geom.H, sp.cw = (uint32_t)geom.pw(1), sp.ch = (uint32_t)geom.ph(1);
  sp.sh = msb_aligned ? 16u - bit_depth : 0u;
  sp.chroma = surface_planes == 1 ? kNoChroma : surface_planes == 2 ? kInterleaved : kPlanar;
  const dim3 grid((row_count(sp.H, sp.ch, sp.chroma) + kStripRows - 1) / kStripRows, B);
  if (timing) G1S_OP_TRY(hipEventRecord(ev[0], stream));
  if (unpack) {
    if (bps == 2) hipLaunchKernelGGL(ks_unpack<2>, grid, dim3(kThreads), 0, stream, sp);
    else hipLaunchKernelGGL(ks_unpack<1>, grid, dim3(kThreads), 0, stream, sp);
  } else {
    if (bps == 2) hipLaunchKernelGGL(ks_pack<2>, grid, dim3(kThreads), 0, stream, sp);
    else hipLaunchKernelGGL(ks_pack<1>, grid, dim3(kThreads), 0, stream, sp);
  }
  G1S_OP_TRY(hipGetLastError());
  if (timing) G1S_OP_TRY(hipEventRecord(ev[1], stream));
  if ((rc = set_done(set)) != 0) return rc;
  for (const HostOut &h : host_outs)
    if ((rc = unpack ? copy_back(h.slot, h.planes) : copy_back_surface(h.slot, h.planes)) != 0) return rc;
  if (timing) {
    G1S_OP_TRY(hipStreamSynchronize(stream));
    float ms = 0;
    G1S_OP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    ms_kernel += ms, frames_timed += B;
  }
  jobs.clear();
  host_outs.clear();
  return G1S_OK;
}

int g1s_surface_conv::convert(const g1s_surface_t &s, const g1s_frame_t &f, bool unpack_) {
  if (err_code) return err_code;
  (void)hipSetDevice(device);
  const Refusal no = check_surface_pair(s, f, bit_depth, unpack_);
  if (no.code) return fail(no.code, no.text);
  int rc;
  if (have_geom && (!geom.same_shape(f) || unpack != unpack_ || surface_planes != s.nplanes || msb_aligned != (s.msb_aligned ? 1u : 0u))) {
    // a new direction, geometry or layout: what is queued goes out and finishes first, the staging buffers are sized again
    if ((rc = flush()) != 0 || (rc = wait()) != 0) return rc;
    have_geom = false;
  }
  if (!have_geom) {
    set_frame_geometry(f);
    set_surface_geometry(s);
    unpack = unpack_, surface_planes = s.nplanes, msb_aligned = s.msb_aligned ? 1 : 0;
  }
  // input and output staging are `batch` slots each; a frame's slot is its place in the batch being filled
  SurfJob job{};
  const uint32_t slot = (uint32_t)jobs.size();
  const uint8_t *in_plane[3] = {nullptr, nullptr, nullptr};
  uint32_t in_stride[3] = {0, 0, 0};
  if ((rc = unpack ? stage_in(s, slot, batch, in_plane, in_stride) : stage_in(f, slot, batch, in_plane, in_stride)) != 0) return rc;
  const int out_kind = unpack ? f.on_device : s.on_device;
  const bool host_out = out_kind != 1;
  if (host_out && (rc = unpack ? need_stage_out(batch) : need_surface_stage_out(batch)) != 0) return rc;
  for (int c = 0; c < sgeom.nplanes; ++c) {
    if (unpack) job.s[c] = const_cast<uint8_t *>(in_plane[c]), job.s_stride[c] = in_stride[c];
    else if (host_out) job.s[c] = surface_stage_out(slot, c), job.s_stride[c] = (uint32_t)sstage.row[c];
    else job.s[c] = static_cast<uint8_t *>(const_cast<void *>(s.data[c])), job.s_stride[c] = (uint32_t)s.stride_bytes[c];
  }
  for (int c = 0; c < geom.nplanes; ++c) {
    if (!unpack) job.f[c] = const_cast<uint8_t *>(in_plane[c]), job.f_stride[c] = in_stride[c];
    else if (host_out) job.f[c] = stage_out(slot, c), job.f_stride[c] = (uint32_t)stage.row[c];
    else job.f[c] = static_cast<uint8_t *>(const_cast<void *>(f.data[c])), job.f_stride[c] = (uint32_t)f.stride_bytes[c];
  }
  if ((rc = unpack ? wait_host_input(s) : wait_host_input(f)) != 0) return rc;
  if (host_out) host_outs.push_back({slot, unpack ? host_planes(f) : host_planes(s)});
  jobs.push_back(job);
  return jobs.size() >= batch ? flush() : G1S_OK;
}

extern "C" {

g1s_surface_conv_t *g1s_surface_new(uint32_t bit_depth, const g1s_surface_opts_t *opts) {
  if (bit_depth < 8 || bit_depth > 16) return refuse_new("a surface converter takes bit depths 8 to 16");
  return new_op<g1s_surface_conv>("the surface converter", opts, "g1s_surface_opts_t", bit_depth, [](g1s_surface_conv &g, std::string &) {
    bool ok = true;
    for (Event &e : g.ev) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    return ok && g.p_jobs.alloc(g.batch);
  });
}

int g1s_surface_unpack(g1s_surface_conv_t *g, const g1s_surface_t *in, g1s_frame_t *out) {
  if (!g || !in || !out) return G1S_ERR_INVALID;
  return g->convert(*in, *out, true);
}

int g1s_surface_pack(g1s_surface_conv_t *g, const g1s_frame_t *in, g1s_surface_t *out) {
  if (!g || !in || !out) return G1S_ERR_INVALID;
  return g->convert(*out, *in, false);
}

int g1s_surface_sync(g1s_surface_conv_t *g) {
  if (!g) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  const int rc = g->flush();
  return rc ? rc : g->wait();
}

int g1s_surface_set_timing(g1s_surface_conv_t *g, int enable, double *ms, uint64_t *frames) {
  if (!g) return G1S_ERR_INVALID;
  g->timing = enable != 0;
  if (ms) *ms = g->ms_kernel;
  if (frames) *frames = g->frames_timed;
  return G1S_OK;
}

const char *g1s_surface_last_error(const g1s_surface_conv_t *g) { return g ? g->err.c_str() : ""; }

void g1s_surface_free(g1s_surface_conv_t *g) { free_op(g); }

}  // extern "C"
