// levels_row.hip.h -- what a lane of the three coarse-level kernels (levels.hip) does: include/g1s_diff.h, rules 25 - 27.
//   box_lane<false>  kd_down:   8 samples of the coarse plane u' (rule 25) from two rows of 16 fine ones
//   box_lane<true>   kd_lowres: the same walk over the fine output v, d = c - box(v) as int16 (rule 27)
//   add_lane         kd_add:    v = Clip3(0, 2^B - 1, v + U(d)) on the 16 x 2 fine samples over those 8 coarse ones, in place
// A fine plane is the caller's: any base, any pitch, so a row of 16 goes through 16-byte loads and stores where its address
// allows and sample by sample where it does not or where the row ends; no byte outside a row's samples is read or written.
// The coarse planes and d are the denoiser's own (rows on 16-byte addresses, padded to 16 bytes), so a lane's 8 samples
// there are one aligned access and may touch the row's padding.  Rows are addressed with 64-bit offsets.  It is plain C++
// -- no built-in of the device, no address space -- so that tests/levels_host.cpp runs it lane by lane under the address and
// undefined-behaviour sanitizers as it stands.
#pragma once
#include <stdint.h>
#include <string.h>

#include "curve_row.hip.h"  // Vec16, load16, store16, load1, store1

namespace g1s_lv {

using g1s_cv::load1;
using g1s_cv::load16;
using g1s_cv::store1;
using g1s_cv::store16;
using g1s_cv::Vec16;

constexpr int kLaneCoarse = 8;                   // coarse samples a lane
constexpr int kLaneFine = 2 * kLaneCoarse;       // fine samples of a row over them
constexpr int kTileLanes = 32, kTileRows = 8;    // a workgroup: 256 x 8 coarse samples
constexpr int kThreads = kTileLanes * kTileRows;
constexpr int kTileW = kTileLanes * kLaneCoarse;

// one plane of a frame for the three kernels.  kd_down: fine = the input (read), coarse = the coarse input (written).
// kd_lowres: fine = the output (read), coarse = the coarse level's output (read), d written.  kd_add: d read, fine = the
// output, read and written.
struct LevelJob {
  uint8_t *fine[3], *coarse[3], *d[3];
  uint32_t fine_stride[3], coarse_stride[3], d_stride[3];  // bytes
};

G1S_CV_HD int imin(int a, int b) { return a < b ? a : b; }
G1S_CV_HD int imax(int a, int b) { return a > b ? a : b; }

// samples x0 .. x0 + 15 of a fine row of W samples, those beyond the row as its last one (the clamp of rule 16)
template <int BPS>
G1S_CV_HD void load_fine16(const uint8_t *row, int x0, int W, uint32_t s[kLaneFine]) {
  const uint8_t *p = row + (size_t)x0 * BPS;
  if (x0 + kLaneFine <= W && ((uintptr_t)p & 15) == 0) {
    if (BPS == 1) {
      const Vec16 a = load16(p);
      for (int k = 0; k < 16; ++k) s[k] = (a.w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    } else {
      const Vec16 a = load16(p), b = load16(p + 16);
      for (int k = 0; k < 8; ++k) s[k] = (a.w[k >> 1] >> (16 * (k & 1))) & 0xffffu, s[8 + k] = (b.w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
    }
  } else {
    for (int k = 0; k < kLaneFine; ++k) s[k] = load1<BPS>(row, (uint32_t)imin(x0 + k, W - 1));
  }
}

// the first n of 16 samples to x0 .. of a fine row: whole where n = 16 and the address allows
template <int BPS>
G1S_CV_HD void store_fine16(uint8_t *row, int x0, int n, const uint32_t s[kLaneFine]) {
  uint8_t *p = row + (size_t)x0 * BPS;
  if (n == kLaneFine && ((uintptr_t)p & 15) == 0) {
    if (BPS == 1) {
      Vec16 o;
      for (int k = 0; k < 4; ++k) o.w[k] = (s[4 * k] & 0xffu) | (s[4 * k + 1] & 0xffu) << 8 | (s[4 * k + 2] & 0xffu) << 16 | (s[4 * k + 3] & 0xffu) << 24;
      store16(p, o);
    } else {
      Vec16 o, q;
      for (int k = 0; k < 4; ++k) o.w[k] = s[2 * k] | s[2 * k + 1] << 16, q.w[k] = s[8 + 2 * k] | s[8 + 2 * k + 1] << 16;
      store16(p, o);
      store16(p + 16, q);
    }
  } else {
    for (int k = 0; k < kLaneFine; ++k)
      if (k < n) store1<BPS>(row, (uint32_t)(x0 + k), s[k]);
  }
}

// 8 samples of one of the denoiser's own planes (a row on a 16-byte address, padded to 16 bytes), x0 a multiple of 8
template <int BPS>
G1S_CV_HD void load_own8(const uint8_t *row, int x0, uint32_t s[kLaneCoarse]) {
  if (BPS == 1) {
    uint32_t w[2];
    memcpy(w, __builtin_assume_aligned(row + x0, 8), 8);
    for (int k = 0; k < 8; ++k) s[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
  } else {
    const Vec16 a = load16(row + (size_t)x0 * 2);
    for (int k = 0; k < 8; ++k) s[k] = (a.w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
  }
}
template <int BPS>
G1S_CV_HD void store_own8(uint8_t *row, int x0, const uint32_t s[kLaneCoarse]) {
  if (BPS == 1) {
    uint32_t w[2];
    for (int k = 0; k < 2; ++k) w[k] = (s[4 * k] & 0xffu) | (s[4 * k + 1] & 0xffu) << 8 | (s[4 * k + 2] & 0xffu) << 16 | (s[4 * k + 3] & 0xffu) << 24;
    memcpy(__builtin_assume_aligned(row + x0, 8), w, 8);
  } else {
    Vec16 o;
    for (int k = 0; k < 4; ++k) o.w[k] = (s[2 * k] & 0xffffu) | (s[2 * k + 1] & 0xffffu) << 16;
    store16(row + (size_t)x0 * 2, o);
  }
}

// Coarse samples cx0 .. cx0 + 7 of coarse row cy (inside the coarse plane) of a fine W x H plane: the box of rule 16.
// LOWRES: d = c - box as int16 into `dst`; else the box itself, BPS bytes a sample, into `dst`.  Samples beyond the coarse
// row's end land in its padding.
template <bool LOWRES, int BPS>
G1S_CV_HD void box_lane(const uint8_t *fine, size_t fine_stride, int W, int H, const uint8_t *c, size_t c_stride, uint8_t *dst, size_t dst_stride, int cx0,
                        int cy) {
  uint32_t a[kLaneFine], b[kLaneFine], o[kLaneCoarse];
  load_fine16<BPS>(fine + (size_t)(2 * cy) * fine_stride, 2 * cx0, W, a);
  load_fine16<BPS>(fine + (size_t)imin(2 * cy + 1, H - 1) * fine_stride, 2 * cx0, W, b);
  for (int k = 0; k < kLaneCoarse; ++k) o[k] = (a[2 * k] + a[2 * k + 1] + b[2 * k] + b[2 * k + 1] + 2) >> 2;
  if (LOWRES) {
    uint32_t cs[kLaneCoarse];
    load_own8<BPS>(c + (size_t)cy * c_stride, cx0, cs);
    for (int k = 0; k < kLaneCoarse; ++k) o[k] = (uint32_t)((int)cs[k] - (int)o[k]);
    store_own8<2>(dst + (size_t)cy * dst_stride, cx0, o);
  } else {
    store_own8<BPS>(dst + (size_t)cy * dst_stride, cx0, o);
  }
}

// d at coarse columns cx0 - 1 .. cx0 + 8 of a row, clamped to the coarse row's ends (rule 27's xb)
G1S_CV_HD void load_d10(const uint8_t *row, int cx0, int CW, int e[kLaneCoarse + 2]) {
  if (cx0 > 0 && cx0 + kLaneCoarse < CW) {
    uint32_t s[kLaneCoarse];
    load_own8<2>(row, cx0, s);
    for (int k = 0; k < kLaneCoarse; ++k) e[1 + k] = (int16_t)s[k];
    e[0] = (int16_t)load1<2>(row, (uint32_t)(cx0 - 1)), e[kLaneCoarse + 1] = (int16_t)load1<2>(row, (uint32_t)(cx0 + kLaneCoarse));
  } else {
    for (int k = 0; k < kLaneCoarse + 2; ++k) e[k] = (int16_t)load1<2>(row, (uint32_t)imin(imax(cx0 - 1 + k, 0), CW - 1));
  }
}

// Rule 27 on the fine samples over coarse samples cx0 .. cx0 + 7 of coarse row cy: rows 2 cy and 2 cy + 1 of the W x H plane
// `fine`, in place.  A sample's new value depends on its own old value and on d only.
template <int BPS>
G1S_CV_HD void add_lane(uint8_t *fine, size_t fine_stride, int W, int H, const uint8_t *d, size_t d_stride, int cx0, int cy, int maxv) {
  const int CW = (W + 1) >> 1, CH = (H + 1) >> 1;
  int ea[kLaneCoarse + 2], eb[kLaneCoarse + 2];
  load_d10(d + (size_t)cy * d_stride, cx0, CW, ea);
  const int x0 = 2 * cx0, n = imin(kLaneFine, W - x0);
  for (int r = 0; r < 2; ++r) {
    const int y = 2 * cy + r;
    if (y >= H) break;
    load_d10(d + (size_t)imin(imax(cy + (r ? 1 : -1), 0), CH - 1) * d_stride, cx0, CW, eb);
    uint8_t *row = fine + (size_t)y * fine_stride;
    uint32_t v[kLaneFine];
    load_fine16<BPS>(row, x0, W, v);
    for (int k = 0; k < kLaneFine; ++k) {
      const int ia = 1 + (k >> 1), ib = ia + ((k & 1) ? 1 : -1);
      const int U = (9 * ea[ia] + 3 * ea[ib] + 3 * eb[ia] + eb[ib] + 8) >> 4;  // (an arithmetic shift: floor)
      v[k] = (uint32_t)imin(imax((int)v[k] + U, 0), maxv);
    }
    store_fine16<BPS>(row, x0, n, v);
  }
}

}  // namespace g1s_lv

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace g1s_lv {
// (levels.hip) the three launches for `nframes` jobs of frames with `nplanes` planes of fine size W[c] x H[c], bps bytes a
// sample, grid (tiles, planes, frames); jobs is device memory
hipError_t launch_down(int bps, const LevelJob *jobs, uint32_t nframes, int nplanes, const int W[3], const int H[3], hipStream_t st);
hipError_t launch_lowres(int bps, const LevelJob *jobs, uint32_t nframes, int nplanes, const int W[3], const int H[3], hipStream_t st);
hipError_t launch_add(int bps, int bit_depth, const LevelJob *jobs, uint32_t nframes, int nplanes, const int W[3], const int H[3], hipStream_t st);
}  // namespace g1s_lv
#endif
