// curve_row.hip.h -- what a lane of kd_curve (curve.hip) does with a row: out(x) = lut[min(in(x), last)] for the n samples of
// the row (include/g1s_diff.h, rule 14), 16 samples a lane and step through 16-byte loads and stores where both rows start
// on a 16-byte address, sample by sample otherwise and for the ragged end.  It is plain C++ -- no built-in of the device, no
// address space -- so that tests/curve_host.cpp runs it lane by lane under the address and undefined-behaviour sanitizers
// as it stands.  Behind it, under hipcc, the launch that curve.hip defines and denoise.hip calls.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define G1S_CV_HD __host__ __device__ inline
#else
#define G1S_CV_HD inline
#endif

namespace g1s_cv {

constexpr uint32_t kMaxEntries = 4096;  // the largest table: the inverse curve, one entry a 12-bit value
constexpr uint32_t kLanes = 64;
constexpr uint32_t kStep = 16;  // samples a lane and step on the fast path: 16 or 32 bytes either side

struct alignas(16) Vec16 {
  uint32_t w[4];
};
G1S_CV_HD Vec16 load16(const uint8_t *p) {
  Vec16 v;
  memcpy(&v, __builtin_assume_aligned(p, 16), 16);
  return v;
}
G1S_CV_HD void store16(uint8_t *p, const Vec16 &v) { memcpy(__builtin_assume_aligned(p, 16), &v, 16); }

template <int BYTES>
G1S_CV_HD uint32_t load1(const uint8_t *row, uint32_t x) {
  if (BYTES == 1) return row[x];
  uint16_t v;
  memcpy(&v, row + (size_t)x * 2, 2);
  return v;
}
template <int BYTES>
G1S_CV_HD void store1(uint8_t *row, uint32_t x, uint32_t v) {
  if (BYTES == 1) {
    row[x] = (uint8_t)v;
  } else {
    const uint16_t h = (uint16_t)v;
    memcpy(row + (size_t)x * 2, &h, 2);
  }
}

G1S_CV_HD uint32_t look(const uint16_t *lut, uint32_t last, uint32_t v) { return lut[v < last ? v : last]; }

// 16 samples starting at sample x0 of rows whose addresses are 16-byte aligned (x0 a multiple of 16)
template <int BYTES_IN, int BYTES_OUT>
G1S_CV_HD void curve_step(const uint16_t *lut, uint32_t last, const uint8_t *src, uint8_t *dst, uint32_t x0) {
  uint32_t s[kStep];
  if (BYTES_IN == 1) {
    const Vec16 a = load16(src + x0);
    for (int k = 0; k < 16; ++k) s[k] = (a.w[k >> 2] >> (8 * (k & 3))) & 0xffu;
  } else {
    const Vec16 a = load16(src + (size_t)x0 * 2), b = load16(src + (size_t)x0 * 2 + 16);
    for (int k = 0; k < 8; ++k) s[k] = (a.w[k >> 1] >> (16 * (k & 1))) & 0xffffu, s[8 + k] = (b.w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
  }
  for (int k = 0; k < 16; ++k) s[k] = look(lut, last, s[k]);
  if (BYTES_OUT == 1) {
    Vec16 o;
    for (int k = 0; k < 4; ++k) o.w[k] = (s[4 * k] & 0xffu) | (s[4 * k + 1] & 0xffu) << 8 | (s[4 * k + 2] & 0xffu) << 16 | (s[4 * k + 3] & 0xffu) << 24;
    store16(dst + x0, o);
  } else {
    Vec16 o, q;
    for (int k = 0; k < 4; ++k) o.w[k] = s[2 * k] | s[2 * k + 1] << 16, q.w[k] = s[8 + 2 * k] | s[8 + 2 * k + 1] << 16;
    store16(dst + (size_t)x0 * 2, o);
    store16(dst + (size_t)x0 * 2 + 16, q);
  }
}

// what lane `lane` of the 64 does with a row of n samples: no byte outside the row's samples is read or written
template <int BYTES_IN, int BYTES_OUT>
G1S_CV_HD void curve_row(const uint16_t *lut, uint32_t last, const uint8_t *src, uint8_t *dst, uint32_t n, uint32_t lane) {
  uint32_t done = 0;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const uint32_t nstep = n / kStep;
    for (uint32_t i = lane; i < nstep; i += kLanes) curve_step<BYTES_IN, BYTES_OUT>(lut, last, src, dst, i * kStep);
    done = nstep * kStep;
  }
  for (uint32_t x = done + lane; x < n; x += kLanes) store1<BYTES_OUT>(dst, x, look(lut, last, load1<BYTES_IN>(src, x)));
}

// one plane of a batch's launch: rows src_stride / dst_stride bytes apart
struct CurveJob {
  const uint8_t *src;
  uint8_t *dst;
  uint32_t src_stride, dst_stride;
};

}  // namespace g1s_cv

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace g1s_cv {
// (curve.hip) W x H samples of `nframes` planes through the `entries` (256, 1024 or 4096) entries of `lut`, `bytes_in` to
// `bytes_out` bytes a sample (1 -> 2, 2 -> 2, 2 -> 1); jobs and lut are device memory
hipError_t launch_curve(int bytes_in, int bytes_out, const CurveJob *jobs, uint32_t nframes, const uint16_t *lut, uint32_t entries, uint32_t W, uint32_t H,
                        hipStream_t st);
}  // namespace g1s_cv
#endif
