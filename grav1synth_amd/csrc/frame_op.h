// frame_op.h -- the host scaffold the frame operations share.  Who uses what: render (grain.hip), denoise (denoise.hip),
// measure (measure.hip), the noise levels (nlf.hip) and the surface converter (surface.hip) are BatchedOp's made by
// new_op; the two meters among them take take_shape and, on top of this file, meter_op.h (their record lanes, their
// summing launch, a temporal meter's frame before); the estimator (estimate.hip: its copies are synchronous) takes the
// owners, pick_device, open_stream and batch_of, the generator (engine.hip) the owners and the addressing predicate; of
// the file commands grain_file.cpp's and denoise_file.cpp's go through rewrite_y4m, measure_file.cpp and denoise_file.cpp
// take device_frame and upload_frame, nlf_file.cpp batch_of alone (what the file commands share among themselves is
// clip_file.h).  Host code only.  The first part -- the batch clamp, plane geometry, the two layouts of a frame, the
// checks of a frame pair, the overlap of two planes -- calls nothing of HIP and builds with a host compiler alone
// (measure_report.cpp, which needs a chroma plane's size and nothing else of this, has it as a local helper and does not
// include this file); the second part, under __HIPCC__, is the owners of HIP objects, the TRY macro, the base of a
// batched operation with its parameter sets and its staging buffers, the steps of a *_new call (opts_fit, open_op,
// new_op), a driver's device frames and the .y4m rewrite loop.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/g1s_diff.h"
#include "clip_file.h"

// (host_abi.cpp) the text g1s_last_global_error() returns on this thread: what a *_new call that returns NULL sets
extern "C" void g1s_set_global_error_(const char *);

namespace g1s_op {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the frames a batched operation launches at once, from the batch_frames its caller gave: 0 = 32, at most 256
inline uint32_t batch_of(uint32_t batch_frames) { return batch_frames ? (batch_frames < 256u ? batch_frames : 256u) : 32u; }

// the planes of a frame: luma W x H, chroma decimated by (subx, suby) <= 1, `bps` bytes a sample
struct PlaneGeom {
  int W = 0, H = 0, subx = 0, suby = 0, nplanes = 0;
  uint32_t bps = 1;
  PlaneGeom() = default;
  PlaneGeom(const g1s_frame_t &f, uint32_t bps_) : W((int)f.width), H((int)f.height), subx(f.xdec), suby(f.ydec), nplanes(f.nplanes), bps(bps_) {}
  explicit PlaneGeom(const g1s_y4m_info_t &i)
      : W((int)i.width), H((int)i.height), subx((int)i.xdec), suby((int)i.ydec), nplanes((int)i.nplanes), bps(i.bit_depth > 8 ? 2 : 1) {}
  size_t pw(int c) const { return c ? (size_t)((W + subx) >> subx) : (size_t)W; }
  size_t ph(int c) const { return c ? (size_t)((H + suby) >> suby) : (size_t)H; }
  size_t row_bytes(int c) const { return pw(c) * bps; }
  bool same_shape(const g1s_frame_t &f) const {
    return W == (int)f.width && H == (int)f.height && nplanes == f.nplanes && subx == f.xdec && suby == f.ydec;
  }
};

// a frame's planes one after the other in one buffer: rows of plane c are row[c] bytes apart, the plane starts at off[c]
struct Layout {
  size_t row[3] = {0, 0, 0}, off[3] = {0, 0, 0}, frame = 0;
  Layout() = default;
  template <class Geom>  // (PlaneGeom, or SurfaceGeom below: nplanes, row_bytes(c), ph(c))
  Layout(const Geom &g, size_t row_align, size_t plane_align) {
    for (int c = 0; c < g.nplanes; ++c) {
      row[c] = align_up(g.row_bytes(c), row_align);
      off[c] = frame;
      frame += align_up(row[c] * g.ph(c), plane_align);
    }
  }
  // the planes of a frame stored from `base`
  void point(g1s_frame_t &f, uint8_t *base, int nplanes) const {
    for (int c = 0; c < nplanes; ++c) f.data[c] = base + off[c], f.stride_bytes[c] = row[c];
  }
};
constexpr size_t kStageRowAlign = 16, kStagePlaneAlign = 256;
// a host frame's copy on the device: rows to 16 bytes, planes to 256
template <class Geom>
inline Layout staging_layout(const Geom &g) { return Layout(g, kStageRowAlign, kStagePlaneAlign); }
// a frame of a .y4m file: no padding anywhere
inline Layout packed_layout(const PlaneGeom &g) { return Layout(g, 1, 1); }

struct Refusal {
  int code = G1S_OK;
  std::string text;
};

// The checks of a frame pair handed to an operation made by `new_name` for `bps` bytes a sample: sample size, a geometry
// the operation takes (`geometry_text` says which), two frames of one shape, and per plane a pointer and a row stride
// that holds a row, fits 32 bits and, for 16-bit samples, is even.  code G1S_OK: fine.  `pair_names`: what the two
// frames are to the operation, for the text of a geometry mismatch (an operation with two inputs names them).
inline Refusal check_frame_pair(const g1s_frame_t &in, const g1s_frame_t &out, uint32_t bps, uint32_t max_width, const char *new_name,
                                const char *geometry_text, const char *pair_names = "input and output") {
  if (in.bytes_per_sample != bps || out.bytes_per_sample != bps)
    return {G1S_ERR_INVALID, std::string("bytes_per_sample does not match the bit depth given to ") + new_name};
  if (in.width < 1 || in.height < 1 || in.width > max_width || in.height > 65536u || (in.nplanes != 1 && in.nplanes != 3) || in.xdec > 1 ||
      in.ydec > in.xdec)
    return {G1S_ERR_INVALID, geometry_text};
  if (out.width != in.width || out.height != in.height || out.nplanes != in.nplanes || out.xdec != in.xdec || out.ydec != in.ydec)
    return {G1S_ERR_DIM_MISMATCH, std::string(pair_names) + " frame geometry differ"};
  const PlaneGeom g(in, bps);
  for (int c = 0; c < g.nplanes; ++c)
    if (!in.data[c] || !out.data[c] || in.stride_bytes[c] < g.row_bytes(c) || out.stride_bytes[c] < g.row_bytes(c) ||
        in.stride_bytes[c] > 0xffffffffu || out.stride_bytes[c] > 0xffffffffu || (bps == 2 && ((in.stride_bytes[c] | out.stride_bytes[c]) & 1)))
      return {G1S_ERR_INVALID, "bad plane pointer or row stride"};
  return {};
}

// The planes of a decoder surface (g1s_surface_t, rule 1): luma W x H; with two planes, plane 1 is rows of 2 cw interleaved
// Cb, Cr samples; with three, the planes of a frame.
struct SurfaceGeom {
  PlaneGeom frame;  // the frame the surface unpacks to (nplanes 1 or 3)
  int nplanes = 0;  // the surface's own: 1, 2 or 3
  SurfaceGeom() = default;
  SurfaceGeom(const g1s_surface_t &s, uint32_t bps) : nplanes(s.nplanes) {
    frame.W = (int)s.width, frame.H = (int)s.height, frame.subx = s.xdec, frame.suby = s.ydec, frame.nplanes = s.nplanes == 1 ? 1 : 3, frame.bps = bps;
  }
  bool interleaved() const { return nplanes == 2; }
  size_t ph(int c) const { return frame.ph(c); }
  size_t row_bytes(int c) const { return c && interleaved() ? 2 * frame.row_bytes(1) : frame.row_bytes(c); }
};

inline bool spans_overlap(const uint8_t *a, size_t a_stride, size_t a_rows, size_t a_row, const uint8_t *b, size_t b_stride, size_t b_rows, size_t b_row) {
  const uint8_t *ae = a + a_stride * (a_rows - 1) + a_row, *be = b + b_stride * (b_rows - 1) + b_row;
  return a < be && b < ae;
}

// The checks of a surface and a frame handed to a converter made by g1s_surface_new for `bit_depth`; `unpack`: the surface
// is the input.  Sample size and depth, msb_aligned, the plane counts of the two sides, the geometry of the input, the two
// geometries against each other, per plane a pointer and a row stride that holds the row (2 cw samples for the interleaved
// plane), fits 32 bits and, for 16-bit samples, is even -- and no byte of one side inside the extent of a plane of the other.
inline Refusal check_surface_pair(const g1s_surface_t &s, const g1s_frame_t &f, uint32_t bit_depth, bool unpack) {
  const uint32_t bps = bit_depth > 8 ? 2 : 1;
  if (s.bytes_per_sample != bps || f.bytes_per_sample != bps)
    return {G1S_ERR_INVALID, "bytes_per_sample does not match the bit depth given to g1s_surface_new"};
  if (s.bit_depth != bit_depth) return {G1S_ERR_INVALID, "the surface's bit_depth is not the one given to g1s_surface_new"};
  if (s.msb_aligned && bps == 1) return {G1S_ERR_INVALID, "msb_aligned needs two-byte samples"};
  if (f.nplanes != 1 && f.nplanes != 3) return {G1S_ERR_INVALID, "a frame has 1 or 3 planes: two planes are a surface's layout"};
  if (s.nplanes < 1 || s.nplanes > 3) return {G1S_ERR_INVALID, "a surface has 1, 2 or 3 planes"};
  const uint32_t iw = unpack ? s.width : f.width, ih = unpack ? s.height : f.height, ix = unpack ? s.xdec : f.xdec, iy = unpack ? s.ydec : f.ydec;
  if (iw < 1 || ih < 1 || iw > 65536u || ih > 65536u || ix > 1 || iy > ix)
    return {G1S_ERR_INVALID, "unsupported surface geometry (4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)"};
  if ((s.nplanes == 1) != (f.nplanes == 1))
    return {G1S_ERR_DIM_MISMATCH, "surface and frame planes do not correspond (1 and 1; 2 or 3 on the surface and 3 on the frame)"};
  if (s.width != f.width || s.height != f.height || s.xdec != f.xdec || s.ydec != f.ydec) return {G1S_ERR_DIM_MISMATCH, "surface and frame geometry differ"};
  const SurfaceGeom g(s, bps);
  for (int c = 0; c < g.nplanes; ++c)
    if (!s.data[c] || s.stride_bytes[c] < g.row_bytes(c) || s.stride_bytes[c] > 0xffffffffu || (bps == 2 && (s.stride_bytes[c] & 1)))
      return {G1S_ERR_INVALID, "bad surface plane pointer or row stride"};
  for (int c = 0; c < g.frame.nplanes; ++c)
    if (!f.data[c] || f.stride_bytes[c] < g.frame.row_bytes(c) || f.stride_bytes[c] > 0xffffffffu || (bps == 2 && (f.stride_bytes[c] & 1)))
      return {G1S_ERR_INVALID, "bad frame plane pointer or row stride"};
  for (int a = 0; a < g.nplanes; ++a)
    for (int b = 0; b < g.frame.nplanes; ++b)
      if (spans_overlap(static_cast<const uint8_t *>(s.data[a]), s.stride_bytes[a], g.ph(a), g.row_bytes(a), static_cast<const uint8_t *>(f.data[b]),
                        f.stride_bytes[b], g.frame.ph(b), g.frame.row_bytes(b)))
        return {G1S_ERR_INVALID, "surface and frame planes overlap: a converter needs distinct buffers"};
  return {};
}

// What `diff` can address: the one predicate g1s_diff::append (refusals) and g1s_diff::batch_far (the chain of a batch) in
// engine.hip ask, per plane.
//   side:   the unit lists pack a unit's column and block row into bit fields (k3m_units: 12 + 12 bits of 64-sample chunks and
//           32-row block rows; k2w_select_units: 10 + 12 bits, which wide_ok keeps to fewer blocks still), so a frame is at
//           most kDiffMaxSide samples wide and high: 4 096 blocks a side.
//   stride: both accumulation kernels form (row of a tile) * stride in 32 bits, for the up to kDiffTileRows rows of a block's tile
//           with its halo, also for rows below the plane that are then not loaded: kDiffTileRows * stride must fit 32 bits.
//   extent: the bytes from a plane's first sample to its last, stride * (rows - 1) + row bytes in 64 bits.  The wide chain
//           reads a plane through a buffer descriptor of 2^31 - 1 bytes (a load beyond it returns zero), the stream chain
//           forms (first row of a tile) * stride in 32 bits: up to kDiffWideMaxExtent either chain, up to kDiffMaxExtent the
//           stream chain, beyond that the plane is refused.
// A chroma plane is (width >> xdec) x (height >> ydec), as everywhere in `diff`.
constexpr uint32_t kDiffMaxSide = 131072u, kDiffTileRows = 36u;
constexpr uint64_t kDiffWideMaxExtent = 0x7fffffffull, kDiffMaxExtent = 0xffffffffull, kDiffMaxStride = 0xffffffffull / kDiffTileRows;

inline uint64_t plane_extent(uint64_t stride_bytes, uint64_t rows, uint64_t row_bytes) { return rows ? stride_bytes * (rows - 1) + row_bytes : 0; }

inline bool diff_size_ok(uint32_t width, uint32_t height) { return width >= 1 && height >= 1 && width <= kDiffMaxSide && height <= kDiffMaxSide; }

enum class DiffReach { kAnyChain, kStreamChain, kRefusedExtent, kRefusedStride };
inline bool diff_refused(DiffReach r) { return r == DiffReach::kRefusedExtent || r == DiffReach::kRefusedStride; }
// a plane of `rows` rows of `row_bytes` bytes, `stride_bytes` apart (a stride that holds a row)
inline DiffReach diff_plane_reach(uint64_t stride_bytes, uint64_t rows, uint64_t row_bytes) {
  if (stride_bytes > kDiffMaxStride) return DiffReach::kRefusedStride;
  const uint64_t extent = plane_extent(stride_bytes, rows, row_bytes);
  return extent <= kDiffWideMaxExtent ? DiffReach::kAnyChain : extent <= kDiffMaxExtent ? DiffReach::kStreamChain : DiffReach::kRefusedExtent;
}
inline const char *diff_refusal_text(DiffReach r) {
  return r == DiffReach::kRefusedStride ? "a row stride above 119304647 bytes (36 rows of it leave 32 bits)"
                                        : "the plane's extent (row stride x (rows - 1) + a row) is 4 GiB or more";
}
static_assert(kDiffMaxStride == 119304647ull, "diff_refusal_text names the bound");

// plane c of a frame handed to `diff`: its extent and its reach
inline uint64_t diff_plane_rows(const g1s_frame_t &f, int c) { return c ? f.height >> f.ydec : f.height; }
inline uint64_t diff_plane_row_bytes(const g1s_frame_t &f, int c) { return (uint64_t)(c ? f.width >> f.xdec : f.width) * f.bytes_per_sample; }
inline uint64_t diff_plane_extent(const g1s_frame_t &f, int c) { return plane_extent(f.stride_bytes[c], diff_plane_rows(f, c), diff_plane_row_bytes(f, c)); }
inline DiffReach diff_plane_reach(const g1s_frame_t &f, int c) { return diff_plane_reach(f.stride_bytes[c], diff_plane_rows(f, c), diff_plane_row_bytes(f, c)); }
// the planes 0 .. nplanes - 1 of a frame together: the furthest any of them reaches
inline DiffReach diff_frame_reach(const g1s_frame_t &f, int nplanes) {
  DiffReach r = DiffReach::kAnyChain;
  for (int c = 0; c < nplanes; ++c) {
    const DiffReach p = diff_plane_reach(f, c);
    if ((int)p > (int)r) r = p;
  }
  return r;
}

// What a scales meter can sum (rule 21 of `measure`): s2 of the 32 x 32 boxes is at most 4^5 (2^B - 1)^2 pw ph, which leaves 64
// bits only for a 12-bit plane of more than 2^30 samples.  Luma is a frame's largest plane.
constexpr uint64_t kScalesMaxSamples12 = 1ull << 30;
inline bool scales_size_ok(uint32_t bit_depth, uint32_t width, uint32_t height) {
  return bit_depth < 12 || (uint64_t)width * height <= kScalesMaxSamples12;
}
inline const char *scales_refusal_text() { return "a scales meter takes 12-bit planes of at most 2^30 samples"; }

// do the bytes of plane ca at `a` and of plane cb at `b` (frames of geometry g) share an address?
inline bool planes_overlap(const PlaneGeom &g, const uint8_t *a, size_t a_stride, int ca, const uint8_t *b, size_t b_stride, int cb) {
  const uint8_t *ae = a + a_stride * (g.ph(ca) - 1) + g.row_bytes(ca), *be = b + b_stride * (g.ph(cb) - 1) + g.row_bytes(cb);
  return a < be && b < ae;
}

// the first line of a .y4m file: goes out as it came in ("" when the file cannot be read: the reader says why)
inline std::string y4m_header_line(const char *path) {
  std::string header;
  if (FILE *f = std::fopen(path, "rb")) {
    char line[1024];
    if (std::fgets(line, sizeof line, f)) header = line;
    std::fclose(f);
  }
  return header;
}

}  // namespace g1s_op

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace g1s_op {

// What a slot or an operation owns: a HIP allocation, event or stream, released when its holder goes.  Move-only; reads as
// the raw pointer it holds.
template <class T, auto FREE>
struct Owned {
  T *p = nullptr;
  Owned() = default;
  Owned(Owned &&o) noexcept : p(o.p) { o.p = nullptr; }
  Owned &operator=(Owned &&o) noexcept { return std::swap(p, o.p), *this; }  // (what this one held goes with `o`)
  ~Owned() { if (p) (void)FREE(p); }
  operator T *() const { return p; }
};
template <class T> using DevBuf = Owned<T, hipFree>;
template <class T> using PinnedBuf = Owned<T, hipHostFree>;
using Event = Owned<std::remove_pointer<hipEvent_t>::type, hipEventDestroy>;
using Stream = Owned<std::remove_pointer<hipStream_t>::type, hipStreamDestroy>;

// inside a member of something with fail(code, text): a HIP call that must succeed
#define G1S_OP_TRY(expr)                                                                                     \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return fail(G1S_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
  } while (0)

// the device an operation runs on: `want`, or the current one when `want` is negative.  "" when there is one, else why not
inline std::string pick_device(int want, const char *operation, int *device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return std::string("no HIP device available: ") + operation + " has no CPU fallback";
  if (want < 0 && hipGetDevice(&want) != hipSuccess) return "hipGetDevice failed";
  *device = want;
  return "";
}

// the operation's own stream on `device`, which becomes the thread's current device
inline bool open_stream(int device, Stream &s) { return hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&s.p, hipStreamNonBlocking) == hipSuccess; }

// one array of a batch's parameters, two sets in turn: pinned on the host, uploaded on the stream
template <class T>
struct ParamSets {
  PinnedBuf<T> h[2];
  DevBuf<T> d[2];
  bool alloc(size_t n) {
    bool ok = true;
    for (int k = 0; k < 2; ++k)
      ok = ok && hipMalloc((void **)&d[k].p, sizeof(T) * n) == hipSuccess && hipHostMalloc((void **)&h[k].p, sizeof(T) * n, hipHostMallocDefault) == hipSuccess;
    return ok;
  }
  hipError_t upload(int set, size_t n, hipStream_t s) { return hipMemcpyAsync(d[set], h[set], sizeof(T) * n, hipMemcpyHostToDevice, s); }
};

// where the output of a frame with host planes goes once its kernels are through
struct HostPlanes {
  void *data[3];
  size_t stride[3];
};
inline HostPlanes host_planes(const g1s_frame_t &f) {
  HostPlanes h{};
  for (int c = 0; c < 3; ++c) h.data[c] = const_cast<void *>(f.data[c]), h.stride[c] = f.stride_bytes[c];
  return h;
}
inline HostPlanes host_planes(const g1s_surface_t &f) {
  HostPlanes h{};
  for (int c = 0; c < f.nplanes; ++c) h.data[c] = const_cast<void *>(f.data[c]), h.stride[c] = f.stride_bytes[c];
  return h;
}

// The device copies of host frames (Geom = PlaneGeom) or host surfaces (SurfaceGeom, whose interleaved plane has rows of
// 2 cw samples) of one geometry: two input rings (the second for an operation that takes two frames a call) and an output
// buffer, each a number of slots of the staging layout, made when the first host frame needs them.
template <class Geom>
struct Staging {
  Geom geom;
  Layout lay;
  DevBuf<uint8_t> in[2], out;  // (after set(): sized again when they are next needed)
  void set(const Geom &g) { geom = g, lay = staging_layout(g), in[0] = DevBuf<uint8_t>(), in[1] = DevBuf<uint8_t>(), out = DevBuf<uint8_t>(); }
  // Where the kernels read `src` (a frame or a surface): the caller's device planes, or slot `slot` of input ring `ring` of
  // `slots` slots, the copies queued on the stream.  Null when fine, else what failed.
  template <class Src>
  const char *stage_in(const Src &src, uint32_t slot, uint32_t slots, int ring, hipStream_t stream, const uint8_t *plane[3], uint32_t stride[3]) {
    const bool theirs = src.on_device == 1;
    if (!theirs && !in[ring] && hipMalloc((void **)&in[ring].p, lay.frame * slots) != hipSuccess) return "hipMalloc of the input staging buffer failed";
    for (int c = 0; c < geom.nplanes; ++c) {
      uint8_t *dst = theirs ? nullptr : in[ring] + lay.frame * slot + lay.off[c];
      if (!theirs && hipMemcpy2DAsync(dst, lay.row[c], src.data[c], src.stride_bytes[c], geom.row_bytes(c), geom.ph(c), hipMemcpyHostToDevice, stream) != hipSuccess)
        return "copy of an input plane to the device failed";
      plane[c] = theirs ? static_cast<const uint8_t *>(src.data[c]) : dst, stride[c] = (uint32_t)(theirs ? src.stride_bytes[c] : lay.row[c]);
    }
    return nullptr;
  }
  const char *need_out(uint32_t slots) {
    return !out && hipMalloc((void **)&out.p, lay.frame * slots) != hipSuccess ? "hipMalloc of the output staging buffer failed" : nullptr;
  }
  uint8_t *out_plane(uint32_t slot, int c) const { return out + lay.frame * slot + lay.off[c]; }
  // slot `slot` of the output buffer back to the host planes, behind what the stream holds
  hipError_t copy_back(uint32_t slot, const HostPlanes &h, hipStream_t stream) const {
    hipError_t e = hipSuccess;
    for (int c = 0; c < geom.nplanes && e == hipSuccess; ++c)
      e = hipMemcpy2DAsync(h.data[c], h.stride[c], out_plane(slot, c), lay.row[c], geom.row_bytes(c), geom.ph(c), hipMemcpyDeviceToHost, stream);
    return e;
  }
};

// The base of an operation that takes frames one at a time and launches them a batch at a time on a stream of its own.
// (The stream comes first: it goes last, after the wait in *_free and after everything that was used on it.)
struct BatchedOp {
  Stream stream;
  int device = 0;
  uint32_t bit_depth = 8, bps = 1, batch = 32;
  int err_code = 0;
  std::string err;
  bool timing = false;
  // the parameters of a batch, two sets in turn (ParamSets): a set is free again when the event behind the kernels of the
  // batch that read it has passed -- the next batch is filled while this one runs
  Event done[2];
  uint64_t batches = 0;
  // the geometry of the frames so far and the device copies of host frames, made when the first such frame comes; beside
  // them the surface side of a converter (surface.hip), set after the frame's.  `geom`, `stage`, `sgeom` and `sstage` are
  // the names the operations know the two geometries and staging layouts by
  bool have_geom = false;
  Staging<PlaneGeom> frames;
  Staging<SurfaceGeom> surfaces;
  PlaneGeom &geom = frames.geom;
  Layout &stage = frames.lay;
  SurfaceGeom &sgeom = surfaces.geom;
  Layout &sstage = surfaces.lay;
  int fail(int code, const std::string &m) {
    if (!err_code) err_code = code, err = m;  // sticky: the first failure is the one reported from then on
    return err_code;
  }
  bool open(int device_, uint32_t bit_depth_, uint32_t batch_frames) {
    device = device_, bit_depth = bit_depth_, bps = bit_depth_ > 8 ? 2 : 1, batch = batch_of(batch_frames);
    bool ok = open_stream(device, stream);
    for (Event &e : done) ok = ok && hipEventCreateWithFlags(&e.p, hipEventDisableTiming) == hipSuccess;
    return ok;
  }
  // the set to fill next; waits for the launch two batches back, which read it
  int next_set(int *set) {
    *set = (int)(batches & 1);
    if (batches >= 2) G1S_OP_TRY(hipEventSynchronize(done[*set]));
    ++batches;
    return G1S_OK;
  }
  int set_done(int set) {
    G1S_OP_TRY(hipEventRecord(done[set], stream));
    return G1S_OK;
  }
  // (a new geometry: nothing may be in flight; the surface's comes after the frame's it corresponds to)
  void set_frame_geometry(const g1s_frame_t &f) { frames.set(PlaneGeom(f, bps)), have_geom = true; }
  void set_surface_geometry(const g1s_surface_t &s) { surfaces.set(SurfaceGeom(s, bps)); }
  // Staging's five, for a frame and for a surface: a host frame takes input ring `ring`, a host surface ring 0
  int staged(const char *no) { return no ? fail(G1S_ERR_HIP, no) : G1S_OK; }
  int stage_in(const g1s_frame_t &in, uint32_t slot, uint32_t slots, const uint8_t *plane[3], uint32_t stride[3], int ring = 0) {
    return staged(frames.stage_in(in, slot, slots, ring, stream, plane, stride));
  }
  int stage_in(const g1s_surface_t &in, uint32_t slot, uint32_t slots, const uint8_t *plane[3], uint32_t stride[3]) {
    return staged(surfaces.stage_in(in, slot, slots, 0, stream, plane, stride));
  }
  // host planes are read before the call that brought them returns; pinned planes stay queued
  int wait_host_input(int on_device, const char *text) { return on_device == 0 && hipStreamSynchronize(stream) != hipSuccess ? fail(G1S_ERR_HIP, text) : G1S_OK; }
  int wait_host_input(const g1s_frame_t &in) { return wait_host_input(in.on_device, "copy of a host frame to the device failed"); }
  int wait_host_input(const g1s_surface_t &in) { return wait_host_input(in.on_device, "copy of a host surface to the device failed"); }
  int need_stage_out(uint32_t slots) { return staged(frames.need_out(slots)); }
  int need_surface_stage_out(uint32_t slots) { return staged(surfaces.need_out(slots)); }
  uint8_t *stage_out(uint32_t slot, int c) const { return frames.out_plane(slot, c); }
  uint8_t *surface_stage_out(uint32_t slot, int c) const { return surfaces.out_plane(slot, c); }
  int copied_back(hipError_t e) { return e == hipSuccess ? G1S_OK : fail(G1S_ERR_HIP, std::string("hipMemcpy2DAsync of an output plane to the host failed: ") + hipGetErrorString(e)); }
  int copy_back(uint32_t slot, const HostPlanes &h) { return copied_back(frames.copy_back(slot, h, stream)); }
  int copy_back_surface(uint32_t slot, const HostPlanes &h) { return copied_back(surfaces.copy_back(slot, h, stream)); }
  int wait() {
    if (hipStreamSynchronize(stream) != hipSuccess) return fail(G1S_ERR_HIP, std::string("hipStreamSynchronize failed: ") + hipGetErrorString(hipGetLastError()));
    return G1S_OK;
  }
};

// *_free of anything with a device and a stream that owns the rest through the owners above
template <class Op>
void free_op(Op *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  delete g;
}

// The geometry step in front of a frame, for an operation whose flush() also waits: a frame of a new shape sends out what is
// queued and lets it finish, then op.set_geometry(f) sizes the buffers again, as it does for the first frame.  (The meters'
// step: render, denoise and the converter end more than a batch there and spell their own.)
template <class Op>
int take_shape(Op &op, const g1s_frame_t &f) {
  if (op.have_geom && !op.geom.same_shape(f)) {
    const int rc = op.flush();
    if (rc) return rc;
    op.have_geom = false;
  }
  return op.have_geom ? G1S_OK : op.set_geometry(f);
}

// A *_new call refuses: the text for g1s_last_global_error(), NULL for the caller
inline std::nullptr_t refuse_new(const std::string &text) { return g1s_set_global_error_(text.c_str()), nullptr; }

// the first steps of a *_new call: the global error cleared, an options struct of another size (`opts_name` names it) refused
template <class Opts>
bool opts_fit(const Opts *opts, const char *opts_name) {
  g1s_set_global_error_("");
  if (opts && opts->struct_size != sizeof(Opts)) return refuse_new(std::string(opts_name) + ".struct_size mismatch"), false;
  return true;
}

// What the *_new calls of the BatchedOp's do once their own parameters have passed.  open_op, behind opts_fit: the device
// (`operation` names the operation where there is none), the operation opened for `bit_depth` and opts->batch_frames, then
// `alloc(*op, refusal)`, the operation's own allocations (false: failed).  A failure is "HIP initialisation failed: ..."
// unless alloc put a text of its own into `refusal`; the operation is freed and the call returns NULL.  new_op is the two
// together, for an operation that reads nothing of its opts before it has a device.
template <class Op, class Opts, class Alloc>
Op *open_op(const char *operation, const Opts *opts, uint32_t bit_depth, Alloc &&alloc) {
  int device = 0;
  const std::string no_device = pick_device(opts ? opts->device : -1, operation, &device);
  if (!no_device.empty()) return refuse_new(no_device);
  Op *op = new Op;
  std::string refusal;
  if (op->open(device, bit_depth, opts ? opts->batch_frames : 0) && alloc(*op, refusal)) return op;
  refuse_new(refusal.empty() ? std::string("HIP initialisation failed: ") + hipGetErrorString(hipGetLastError()) : refusal);
  free_op(op);
  return nullptr;
}
template <class Op, class Opts, class Alloc>
Op *new_op(const char *operation, const Opts *opts, const char *opts_name, uint32_t bit_depth, Alloc &&alloc) {
  return opts_fit(opts, opts_name) ? open_op<Op>(operation, opts, bit_depth, alloc) : nullptr;
}

// A file driver's own device frames: a frame of geometry g whose planes lie from `base` on in layout `lay` ...
inline g1s_frame_t device_frame(const PlaneGeom &g, const Layout &lay, uint8_t *base) {
  g1s_frame_t f{};
  f.width = (uint32_t)g.W, f.height = (uint32_t)g.H, f.bytes_per_sample = (uint8_t)g.bps, f.xdec = (uint8_t)g.subx, f.ydec = (uint8_t)g.suby;
  f.nplanes = (uint8_t)g.nplanes, f.on_device = 1;
  lay.point(f, base, g.nplanes);
  return f;
}
// ... and a host frame of its shape (a reader lends one until its next call) copied into it before the call returns
inline bool upload_frame(const g1s_frame_t &host, const g1s_frame_t &dev) {
  const PlaneGeom g(dev, dev.bytes_per_sample);
  bool ok = true;
  for (int c = 0; c < g.nplanes; ++c)
    ok = ok && hipMemcpy2D(const_cast<void *>(dev.data[c]), dev.stride_bytes[c], host.data[c], host.stride_bytes[c], g.row_bytes(c), g.ph(c), hipMemcpyHostToDevice) == hipSuccess;
  return ok;
}

// A .y4m file through an operation into another .y4m file: the header line as it came, every frame handed over as a host
// frame with a slot of a pinned ring of packed frames as its output, and after every `batch` frames and at the end the
// completed frames written out.  `Driver` says what differs:
//   bool open(const g1s_y4m_info_t &)   makes the operation (false: refused with new_failed and the global error text)
//   uint32_t batch(), ring()            frames between two drains; frames that can be unwritten at once
//   int frame(int64_t n, const g1s_frame_t *in, g1s_frame_t *out)
//   int drain(bool end, uint64_t *complete)   waits; *complete (preset to the frames handed over) = frames that can be written
//   const char *last_error(); void close()
// Returns the number of frames, or the code of what went wrong with its text in err.
template <class Driver>
int64_t rewrite_y4m(const char *in, const char *out, char *err, size_t cap, Driver &&op) {
  using g1s_clip::refuse;
  if (!in || !out) return refuse(err, cap, G1S_ERR_INVALID, "null path");
  const std::string header = y4m_header_line(in);
  g1s_y4m_t *y = g1s_y4m_open(in, err, cap);
  if (!y) return G1S_ERR_INVALID;
  g1s_y4m_info_t info;
  g1s_y4m_get_info(y, &info);
  if (!op.open(info)) {
    g1s_y4m_close(y);
    return refuse(err, cap, op.new_failed, g1s_last_global_error());
  }
  FILE *fo = std::fopen(out, "wb");
  if (!fo) {
    op.close();
    g1s_y4m_close(y);
    return refuse(err, cap, G1S_ERR_INVALID, std::string("cannot create ") + out);
  }
  const Layout lay = packed_layout(PlaneGeom(info));
  const uint32_t batch = op.batch(), ring = op.ring();
  PinnedBuf<uint8_t> obuf;
  int64_t frames = 0, written = 0;
  int rc = G1S_OK;
  std::string why;
  bool ok = std::fwrite(header.data(), 1, header.size(), fo) == header.size();
  if (!ok) rc = G1S_ERR_INVALID, why = std::string("cannot write ") + out;
  if (ok && hipHostMalloc((void **)&obuf.p, lay.frame * ring, hipHostMallocDefault) != hipSuccess)
    ok = false, rc = G1S_ERR_HIP, why = "hipHostMalloc of the output frames failed";
  auto drain = [&](bool end) {
    uint64_t complete = (uint64_t)frames;
    rc = op.drain(end, &complete);
    if (rc) {
      why = op.last_error();
      return false;
    }
    for (; written < (int64_t)complete; ++written)
      if (std::fwrite("FRAME\n", 1, 6, fo) != 6 || std::fwrite(obuf + lay.frame * (size_t)(written % ring), 1, lay.frame, fo) != lay.frame) {
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
    lay.point(fout, obuf + lay.frame * (size_t)(frames % ring), (int)info.nplanes);
    fin.on_device = 0;  // (the reader lends the frame until its next call: copied before the operation's call returns)
    fout.on_device = 2;
    rc = op.frame(frames, &fin, &fout);
    if (rc) {
      ok = false, why = "frame " + std::to_string(frames) + ": " + op.last_error();
      break;
    }
    ++frames;
    if (frames % batch == 0) ok = drain(false);
  }
  if (ok) ok = drain(true);
  if (std::fclose(fo) != 0 && ok) ok = false, rc = G1S_ERR_INVALID, why = std::string("cannot write ") + out;
  op.close();
  g1s_y4m_close(y);
  if (!ok) return refuse(err, cap, rc ? rc : G1S_ERR_INVALID, why);
  return frames;
}

}  // namespace g1s_op
#endif  // __HIPCC__
