// curve.h -- the variance-stabilising curve of `denoise` from the segments of a grain table (include/g1s_diff.h, rules 12
// and 13), and the checks of a pair (f, g) that a caller hands to g1s_denoise_new_curve.  Host code only: it calls nothing
// of HIP and builds with a host compiler alone.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/g1s_diff.h"

namespace g1s_cv {

constexpr uint32_t kStabBits = 12, kStabTop = (1u << kStabBits) - 1, kInvEntries = 1u << kStabBits;  // the stabilised domain

// 7.18.3.4 for the luma points of a segment: 256 entries through the points, flat outside them, zero without points
inline void scaling_lut_points(const uint8_t (*p)[2], int n, int lut[256]) {
  for (int x = 0; x < 256; ++x) lut[x] = 0;
  if (!n) return;
  for (int x = 0; x < p[0][0]; ++x) lut[x] = p[0][1];
  for (int i = 0; i + 1 < n; ++i) {
    const int dy = (int)p[i + 1][1] - (int)p[i][1], dx = (int)p[i + 1][0] - (int)p[i][0];
    const int delta = dy * ((65536 + (dx >> 1)) / dx);
    for (int x = 0; x < dx; ++x) lut[p[i][0] + x] = p[i][1] + ((x * delta + 32768) >> 16);
  }
  for (int x = p[n - 1][0]; x < 256; ++x) lut[x] = p[n - 1][1];
}
inline void scaling_lut(const g1s_segment_t &sg, int lut[256]) { scaling_lut_points(sg.scaling_points_y, sg.num_y_points, lut); }

// 7.18.3.5 scale_lut at `index` of a plane of `bit_depth` bits
inline int scale_lut(const int lut[256], int index, uint32_t bit_depth) {
  const int sh = (int)bit_depth - 8, x = index >> sh;
  if (!sh || x == 255) return lut[x];
  const int rem = index - (x << sh), start = lut[x], end = lut[x + 1];
  return start + (((end - start) * rem + (1 << (sh - 1))) >> sh);
}

// the bit depths and ranges rule 12 has.  "" when fine, else the refusal.
inline std::string check_depth_range(uint32_t bit_depth, uint32_t range) {
  if (bit_depth == 12) return "a grain prior needs headroom above the clip's bit depth: the stabilised domain is 12 bits, so a 12-bit clip is refused";
  if (bit_depth != 8 && bit_depth != 10) return "a grain prior is defined for bit depths 8 and 10";
  const uint32_t rmax = 1u << (kStabBits - bit_depth);
  if (range > rmax) return "prior range must be 1.." + std::to_string(rmax) + " at " + std::to_string(bit_depth) + " bits (0 = the default)";
  return "";
}

// Rule 12 up to s(v): the mean scaling function of the segments, v = 0 .. M.  "" when fine, else the refusal.
inline std::string s_from_segments(const g1s_segment_t *segs, size_t n, uint32_t bit_depth, std::vector<uint64_t> &s) {
  if (!segs || n < 1) return "a grain prior needs at least one segment";
  for (size_t i = 0; i < n; ++i) {
    if (segs[i].num_y_points > G1S_NUM_Y_POINTS) return "segment " + std::to_string(i) + ": more than 14 luma scaling points";
    for (int k = 0; k + 1 < segs[i].num_y_points; ++k)
      if (segs[i].scaling_points_y[k + 1][0] <= segs[i].scaling_points_y[k][0])
        return "segment " + std::to_string(i) + ": luma scaling points must have increasing values";
  }
  const uint32_t M = (1u << bit_depth) - 1;
  s.assign((size_t)M + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    int lut[256];
    scaling_lut(segs[i], lut);
    for (uint32_t v = 0; v <= M; ++v) s[v] += (uint64_t)scale_lut(lut, (int)v, bit_depth);
  }
  for (uint32_t v = 0; v <= M; ++v) s[v] = (s[v] + (n >> 1)) / n;
  return "";
}

// Rule 12 from "floor = ..." onwards and rule 13, on s(v), v = 0 .. M (a bit depth and a range check_depth_range passed):
// fwd[1 << B], inv[4096].  "" when fine, else the refusal.
inline std::string curve_from_s(const std::vector<uint64_t> &s, uint32_t bit_depth, uint32_t range, uint16_t *fwd, uint16_t *inv) {
  const uint32_t rmax = 1u << (kStabBits - bit_depth);
  const uint32_t R = range ? range : (rmax < 4u ? rmax : 4u), M = (1u << bit_depth) - 1;
  uint64_t top = 0;
  for (uint32_t v = 0; v <= M; ++v) top = s[v] > top ? s[v] : top;
  const uint64_t floor = top ? (top + R - 1) / R : 1;  // max(1, ceil(max s / R))
  std::vector<uint64_t> Cs((size_t)M + 2, 0);          // C(x) = sum over v < x of r(v)
  for (uint32_t v = 0; v <= M; ++v) Cs[v + 1] = Cs[v] + ((1ull << 24) / (s[v] > floor ? s[v] : floor));
  const uint64_t CM = Cs[M];
  for (uint32_t x = 0; x <= M; ++x) fwd[x] = (uint16_t)((kStabTop * Cs[x] + (CM >> 1)) / CM);
  if (fwd[0] != 0 || fwd[M] != kStabTop) return "internal error: the curve does not span the stabilised domain";
  for (uint32_t x = 0; x < M; ++x)
    if (fwd[x + 1] <= fwd[x]) return "internal error: the curve is not strictly increasing";
  // rule 13: the smallest x with |f(x) - y| minimal
  uint32_t x = 0;
  for (uint32_t y = 0; y < kInvEntries; ++y) {
    while (x < M && fwd[x + 1] <= y) ++x;  // f(x) <= y < f(x + 1), or x = M
    inv[y] = (uint16_t)(x < M && (uint32_t)fwd[x + 1] - y < y - (uint32_t)fwd[x] ? x + 1 : x);
  }
  return "";
}

// Rules 12 and 13: fwd[1 << B], inv[4096].  "" when fine, else the refusal.
inline std::string build(const g1s_segment_t *segs, size_t n, uint32_t bit_depth, uint32_t range, uint16_t *fwd, uint16_t *inv) {
  std::string why = check_depth_range(bit_depth, range);
  std::vector<uint64_t> s;
  if (why.empty()) why = s_from_segments(segs, n, bit_depth, s);
  return why.empty() ? curve_from_s(s, bit_depth, range, fwd, inv) : why;
}

// The same from a given s[1 << B] (noise levels, rule N6): the refusals of the bit depth and the range, then the curve.
inline std::string build_sigma(const uint8_t *s8, uint32_t bit_depth, uint32_t range, uint16_t *fwd, uint16_t *inv) {
  const std::string why = check_depth_range(bit_depth, range);
  if (!why.empty()) return why;
  if (!s8) return "a curve needs the scaling function it is made from";
  const std::vector<uint64_t> s(s8, s8 + ((size_t)1 << bit_depth));
  return curve_from_s(s, bit_depth, range, fwd, inv);
}

// what g1s_denoise_new_curve asks of a pair it is handed.  "" when fine.
inline std::string check(uint32_t bit_depth, const uint16_t *fwd, const uint16_t *inv) {
  if (bit_depth == 12) return "a grain prior needs headroom above the clip's bit depth: the stabilised domain is 12 bits, so a 12-bit clip is refused";
  if (bit_depth != 8 && bit_depth != 10) return "a grain prior is defined for bit depths 8 and 10";
  if (!fwd || !inv) return "g1s_denoise_new_curve needs both tables of the curve";
  const uint32_t M = (1u << bit_depth) - 1;
  if (fwd[0] != 0 || fwd[M] != kStabTop) return "curve: fwd must run from 0 to 4095";
  for (uint32_t x = 0; x < M; ++x)
    if (fwd[x + 1] <= fwd[x]) return "curve: fwd must be strictly increasing (at " + std::to_string(x + 1) + ")";
  for (uint32_t y = 0; y < kInvEntries; ++y) {
    if (inv[y] > M) return "curve: inv must stay within the clip's bit depth (at " + std::to_string(y) + ")";
    if (y && inv[y] < inv[y - 1]) return "curve: inv must be non-decreasing (at " + std::to_string(y) + ")";
  }
  for (uint32_t x = 0; x <= M; ++x)
    if (inv[fwd[x]] != x) return "curve: inv[fwd[x]] must be x (at " + std::to_string(x) + ")";
  return "";
}

// ---- a chroma gain (rules 21 - 24): the Q8 multiplier m[256] of the joint chroma distance, indexed by the guide's top 8 bits
constexpr int kGainEntries = 256;
constexpr uint32_t kGainMax = 16384, kGainRangeMax = 8;

// Rule 21: m from s(i), i = 0 .. 255, and a range R (0 = 4).  "" when fine, else the refusal.
inline std::string gain_from_s(const uint8_t s[256], uint32_t range, uint16_t gain[256]) {
  if (range > kGainRangeMax) return "chroma gain range must be 1..8 (0 = the default)";
  if (!s || !gain) return "a chroma gain needs the scaling function it is made from and the output table";
  const uint64_t R = range ? range : 4;
  uint64_t top = 0;
  for (int i = 0; i < kGainEntries; ++i) top = s[i] > top ? s[i] : top;
  const uint64_t floor = top ? (top + R - 1) / R : 1;  // max(1, ceil(top / R))
  uint64_t sum = 0;
  for (int i = 0; i < kGainEntries; ++i) sum += s[i] > floor ? s[i] : floor;
  const uint64_t sbar = (sum + 128) >> 8;
  for (int i = 0; i < kGainEntries; ++i) {
    const uint64_t v = s[i] > floor ? s[i] : floor, v2 = v * v;
    const uint64_t m = (256 * sbar * sbar + (v2 >> 1)) / v2;
    gain[i] = (uint16_t)(m < 1 ? 1 : m > kGainMax ? kGainMax : m);
  }
  return "";
}

// Rule 22: s(v), v = 0 .. 255, the rounded mean of the chroma scaling functions of both chroma planes of n >= 1 segments at
// the luma v under them.  "" when fine, else the refusal.
inline std::string chroma_s_from_segments(const g1s_segment_t *segs, size_t n, uint8_t s[256]) {
  if (!segs || n < 1) return "a grain prior needs at least one segment";
  for (size_t i = 0; i < n; ++i) {
    const g1s_segment_t &sg = segs[i];
    if (sg.num_y_points > G1S_NUM_Y_POINTS) return "segment " + std::to_string(i) + ": more than 14 luma scaling points";
    if (sg.num_cb_points > G1S_NUM_UV_POINTS || sg.num_cr_points > G1S_NUM_UV_POINTS)
      return "segment " + std::to_string(i) + ": more than " + std::to_string(G1S_NUM_UV_POINTS) + " chroma scaling points";
    for (int k = 0; k + 1 < sg.num_y_points; ++k)
      if (sg.scaling_points_y[k + 1][0] <= sg.scaling_points_y[k][0]) return "segment " + std::to_string(i) + ": luma scaling points must have increasing values";
    for (int k = 0; k + 1 < sg.num_cb_points; ++k)
      if (sg.scaling_points_cb[k + 1][0] <= sg.scaling_points_cb[k][0]) return "segment " + std::to_string(i) + ": chroma scaling points must have increasing values";
    for (int k = 0; k + 1 < sg.num_cr_points; ++k)
      if (sg.scaling_points_cr[k + 1][0] <= sg.scaling_points_cr[k][0]) return "segment " + std::to_string(i) + ": chroma scaling points must have increasing values";
  }
  uint64_t sum[256] = {0};
  for (size_t i = 0; i < n; ++i) {
    const g1s_segment_t &sg = segs[i];
    for (int c = 0; c < 2; ++c) {
      int lut[256];
      if (sg.chroma_scaling_from_luma) scaling_lut(sg, lut);
      else if (c == 0) scaling_lut_points(sg.scaling_points_cb, sg.num_cb_points, lut);
      else scaling_lut_points(sg.scaling_points_cr, sg.num_cr_points, lut);
      const int lm = (c ? sg.cr_luma_mult : sg.cb_luma_mult) - 128, mu = (c ? sg.cr_mult : sg.cb_mult) - 128, off = (int)(c ? sg.cr_offset : sg.cb_offset) - 256;
      for (int v = 0; v < 256; ++v) {
        int idx = v;
        if (!sg.chroma_scaling_from_luma) {
          idx = ((v * lm + 128 * mu) >> 6) + off;  // (>> of a negative int: arithmetic with every compiler this builds with)
          idx = idx < 0 ? 0 : idx > 255 ? 255 : idx;
        }
        sum[v] += (uint64_t)lut[idx];
      }
    }
  }
  for (int v = 0; v < 256; ++v) s[v] = (uint8_t)((sum[v] + n) / (2 * n));
  return "";
}

// Rules 22 + 21.  "" when fine, else the refusal.
inline std::string build_gain(const g1s_segment_t *segs, size_t n, uint32_t range, uint16_t gain[256]) {
  if (range > kGainRangeMax) return "chroma gain range must be 1..8 (0 = the default)";
  if (!gain) return "a chroma gain needs the scaling function it is made from and the output table";
  uint8_t s[256];
  const std::string why = chroma_s_from_segments(segs, n, s);
  return why.empty() ? gain_from_s(s, range, gain) : why;
}

// what g1s_denoise_new_gain asks of a table it is handed: any 256 entries in 1 .. 16384.  "" when fine.
inline std::string check_gain(const uint16_t gain[256]) {
  for (int i = 0; i < kGainEntries; ++i)
    if (gain[i] < 1 || gain[i] > kGainMax) return "chroma gain must be 1..16384 (at " + std::to_string(i) + ")";
  return "";
}

}  // namespace g1s_cv
