// nlf_table.h -- what is done with a lag record once it is off the device (include/g1s_diff.h, "lagged noise levels", rule
// L5): the checked sum of records; and rules L6 - L7 up to the solve: the normal equations of a plane's AR fit.  Host code only: it calls nothing of HIP and builds with a host compiler alone.  The
// kernels that make the records are in nlf_lags.hip.
#pragma once
#include <stdint.h>

#include <cstring>
#include <string>

#include "../../include/g1s_diff.h"

namespace g1s_nl {

constexpr int kLags = 46, kCross = 25;
// L2: lag i as (dx, dy)
inline void lag_offset(int i, int *dx, int *dy) {
  if (i < 7) *dx = i, *dy = 0;
  else *dx = (i - 7) % 13 - 6, *dy = (i - 7) / 13 + 1;
}

// L5: false when a sum leaves 64 bits (then *total is untouched)
inline bool sum_lags(const g1s_nlf_lrecord_t *recs, size_t n, g1s_nlf_lrecord_t *total) {
  g1s_nlf_lrecord_t t;
  std::memset(&t, 0, sizeof t);
  bool ok = true;
  const auto add = [&ok](auto &to, auto v) { ok = !__builtin_add_overflow(to, v, &to) && ok; };
  for (size_t f = 0; f < n; ++f) {
    const g1s_nlf_lrecord_t &r = recs[f];
    for (int c = 0; c < 3; ++c) {
      for (int i = 0; i < kLags; ++i) add(t.n[c][i], r.n[c][i]), add(t.r[c][i], r.r[c][i]);
      add(t.s[c], r.s[c]);
    }
    for (int c = 0; c < 2; ++c)
      for (int j = 0; j < kCross; ++j) add(t.xn[c][j], r.xn[c][j]), add(t.xr[c][j], r.xr[c][j]);
    add(t.ln, r.ln), add(t.ls, r.ls), add(t.l2, r.l2);
  }
  if (ok) *total = t;
  return ok;
}

constexpr const char *kTooFewPairs = "too few static sample pairs for a table";

// L2 backwards: the index of lag d or of -d, whichever the record holds (|dx| <= 6, |dy| <= 3)
inline int lag_index(int dx, int dy) {
  if (dy < 0 || (dy == 0 && dx < 0)) dx = -dx, dy = -dy;
  return dy ? 7 + 13 * (dy - 1) + dx + 6 : dx;
}
// L4: the index of offset delta among rule 4 of `measure`'s 25 (|dx| <= 3, -3 <= dy <= 0, causal or (0, 0))
inline int cross_index(int dx, int dy) { return (dy + 3) * 7 + dx + 3; }
// the table's causal offsets at lag L, in coefficient order: m = 2 L (L + 1) of them
inline int causal_offsets(int L, int (*o)[2]) {
  int m = 0;
  for (int dy = -L; dy <= 0; ++dy)
    for (int dx = -L; dx <= L && (dy < 0 || dx < 0); ++dx) o[m][0] = dx, o[m][1] = dy, ++m;
  return m;
}

// L6 - L7 up to the solve: plane c's normal equations at lag L from a clip's lag record, row-major A[nc * nc] and b[nc],
// nc = m (luma) or m + 1 (chroma), in the units compute_latest (fold.cpp) gives ar_solve: code values of 8 bits over 255,
// so a covariance at depth B is divided by 4^(B - 8) 255^2.  *N = n[c][0], the observations.  "" when fine, else L6's refusal.
inline const char *ar_system(const g1s_nlf_lrecord_t &t, int c, uint32_t bit_depth, int L, uint64_t min_count, double *A, double *b, int *nc_out, uint64_t *N) {
  const uint64_t nmin = min_count ? min_count : 4096;
  int o[24][2];
  const int m = causal_offsets(L, o), nc = m + (c ? 1 : 0);
  *nc_out = nc;
  if (t.n[c][0] < nmin) return kTooFewPairs;
  const double mean = (double)t.s[c] / (double)t.n[c][0];
  bool enough = true;
  const auto C = [&](int dx, int dy) {
    const int i = lag_index(dx, dy);
    if (t.n[c][i] < nmin) return enough = false, 0.0;
    return (double)t.r[c][i] / (double)t.n[c][i] - mean * mean;
  };
  const double den = (double)(1u << (2 * (bit_depth - 8))) * (255.0 * 255.0), n0 = (double)t.n[c][0];
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < m; ++j) A[i * nc + j] = n0 * C(o[i][0] - o[j][0], o[i][1] - o[j][1]) / den;
    b[i] = n0 * C(o[i][0], o[i][1]) / den;
  }
  if (c) {
    if (t.ln < nmin) return kTooFewPairs;
    const double mean_l = (double)t.ls / (double)t.ln, var_l = (double)t.l2 / (double)t.ln - mean_l * mean_l;
    const auto X = [&](int dx, int dy) {
      const int j = cross_index(dx, dy);
      if (t.xn[c - 1][j] < nmin) return enough = false, 0.0;
      return (double)t.xr[c - 1][j] / (double)t.xn[c - 1][j] - mean_l * mean;
    };
    for (int i = 0; i < m; ++i) A[i * nc + m] = A[m * nc + i] = n0 * X(o[i][0], o[i][1]) / den;
    A[m * nc + m] = n0 * var_l / den;
    b[m] = n0 * X(0, 0) / den;
  }
  *N = t.n[c][0];
  return enough ? "" : kTooFewPairs;
}

// L10 (nlf_table.cpp: it takes the fit): the report of a clip's lag record of `pairs` pairs
std::string lag_report(const g1s_nlf_lrecord_t &t, uint64_t pairs, uint32_t bit_depth, uint32_t nplanes, uint32_t lag, uint64_t min_count);

}  // namespace g1s_nl
