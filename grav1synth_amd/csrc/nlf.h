// nlf.h -- what is done with a noise-level record once it is off the device (include/g1s_diff.h, "noise levels", rules N4 -
// N8): the checked sum of records, the levels and the prior's scaling function, the strength, the report.  Host code only:
// it calls nothing of HIP and builds with a host compiler alone.  The kernels that make the records are in nlf.hip.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/g1s_diff.h"

namespace g1s_nl {

constexpr int kBins = 32;
constexpr uint64_t kDefaultMinCount = 4096;
constexpr double kSqrtPiBy2 = 1.2533141373155003;  // SQRT_PI_BY_2, the estimator's

inline uint64_t min_count_of(uint64_t min_count) { return min_count ? min_count : kDefaultMinCount; }

// N4: false when a sum leaves 64 bits (then *total is untouched)
inline bool sum(const g1s_nlf_record_t *recs, size_t n, g1s_nlf_record_t *total) {
  g1s_nlf_record_t t;
  std::memset(&t, 0, sizeof t);
  bool ok = true;
  for (size_t f = 0; f < n; ++f)
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < kBins; ++k)
        ok = !__builtin_add_overflow(t.n[c][k], recs[f].n[c][k], &t.n[c][k]) && !__builtin_add_overflow(t.a[c][k], recs[f].a[c][k], &t.a[c][k]) &&
             !__builtin_add_overflow(t.q[c][k], recs[f].q[c][k], &t.q[c][k]) && ok;
  if (ok) *total = t;
  return ok;
}

// floor(sqrt(v)) of a 128-bit value whose root fits 64 bits
inline uint64_t isqrt(unsigned __int128 v) {
  uint64_t r = 0;
  for (int b = 63; b >= 0; --b) {
    const uint64_t t = r | (1ull << b);
    if ((unsigned __int128)t * t <= v) r = t;
  }
  return r;
}

// N5: t of a bin with sums q and n > 0
inline uint64_t level_of(unsigned __int128 q, unsigned __int128 n) { return isqrt((q << 16) / ((unsigned __int128)36 * n)); }
// N5: t[k] of plane c's bin k (a bin with n > 0)
inline uint64_t level(const g1s_nlf_record_t &r, int c, int k) { return level_of(r.q[c][k], r.n[c][k]); }

// N5 - N6 on the bins (n[k], q[k]): s[1 << B].  false when no bin is valid.
inline bool sigma_of_bins(const unsigned __int128 *n, const unsigned __int128 *q, uint32_t bit_depth, uint64_t min_count, uint8_t *s) {
  const uint64_t nmin = min_count_of(min_count);
  int valid[kBins], nvalid = 0;
  uint64_t t[kBins], tmax = 0;
  for (int k = 0; k < kBins; ++k)
    if (n[k] >= nmin) {
      t[k] = level_of(q[k], n[k]);
      tmax = t[k] > tmax ? t[k] : tmax;
      valid[nvalid++] = k;
    }
  if (!nvalid) return false;
  int64_t y[kBins], c[kBins];
  for (int i = 0; i < nvalid; ++i) {
    const int k = valid[i];
    const uint64_t v = 255 * t[k] / (tmax ? tmax : 1);
    y[i] = (int64_t)(v ? v : 1);
    c[i] = ((int64_t)k << (bit_depth - 5)) + ((int64_t)1 << (bit_depth - 6));
  }
  const int64_t top = ((int64_t)1 << bit_depth) - 1;
  int i = 0;  // the last valid centre at or below v
  for (int64_t v = 0; v <= top; ++v) {
    while (i + 1 < nvalid && c[i + 1] <= v) ++i;
    int64_t sv;
    if (v <= c[0]) sv = y[0];
    else if (i + 1 >= nvalid) sv = y[nvalid - 1];
    else {
      const int64_t den = 2 * (c[i + 1] - c[i]), num = (y[i + 1] - y[i]) * (v - c[i]) * 2 + (c[i + 1] - c[i]);
      const int64_t fl = num >= 0 ? num / den : -((-num + den - 1) / den);  // towards minus infinity
      sv = y[i] + fl;
    }
    s[v] = (uint8_t)sv;
  }
  return true;
}

// N5 - N6: s[1 << B] from the luma bins.  "" when fine, else the refusal (the bit depths: rule 12's texts, by the caller).
inline std::string sigma(const g1s_nlf_record_t &r, uint32_t bit_depth, uint64_t min_count, uint8_t *s) {
  unsigned __int128 n[kBins], q[kBins];
  for (int k = 0; k < kBins; ++k) n[k] = r.n[0][k], q[k] = r.q[0][k];
  return sigma_of_bins(n, q, bit_depth, min_count, s) ? "" : "no luma bin has enough smooth samples for a prior";
}

// N9: s[256] from the bins of the two chroma planes pooled -- N5 and N6 at B = 8 whatever the clip's depth (the bins are bins of
// averageLuma's top five bits).  "" when fine, else the refusal.
inline std::string chroma_sigma(const g1s_nlf_record_t &r, uint64_t min_count, uint8_t s[256]) {
  unsigned __int128 n[kBins], q[kBins];
  for (int k = 0; k < kBins; ++k) n[k] = (unsigned __int128)r.n[1][k] + r.n[2][k], q[k] = (unsigned __int128)r.q[1][k] + r.q[2][k];
  return sigma_of_bins(n, q, 8, min_count, s) ? "" : "no chroma bin has enough smooth samples for a prior";
}

// N7 for a plane class (0: luma; 1: the chroma planes pooled).  "" when fine, else the refusal.
inline std::string strength(const g1s_nlf_record_t &r, uint32_t bit_depth, uint64_t min_count, uint32_t plane_class, double *h) {
  unsigned __int128 Q = 0, N = 0;
  for (int c = plane_class ? 1 : 0; c < (plane_class ? 3 : 1); ++c)
    for (int k = 0; k < kBins; ++k) Q += r.q[c][k], N += r.n[c][k];
  if (N < min_count_of(min_count)) return "too few smooth samples for a strength";
  const double v = std::sqrt((2.0 * (double)Q) / (36.0 * (double)N)) / (double)(1u << (bit_depth - 8));
  if (!(v > 0.0 && v <= 1000.0)) return "the measured strength is outside 0 < h <= 1000";
  *h = v;
  return "";
}

// N8
inline std::string report(const g1s_nlf_record_t &r, uint64_t frames, uint32_t bit_depth, uint32_t nplanes, uint64_t min_count) {
  auto value = [](bool defined, double v) -> std::string {
    if (!defined) return "-";
    char s[64];
    snprintf(s, sizeof s, "%.4f", v);
    return s;
  };
  std::string s = "noiselevels1\n";
  s += "frames " + std::to_string(frames) + " bit_depth " + std::to_string(bit_depth) + " planes " + std::to_string(nplanes) + "\n";
  const double scale = (double)(1u << (bit_depth - 8));
  for (int c = 0; c < (int)nplanes; ++c) {
    s += "plane " + std::to_string(c) + "\n";
    unsigned __int128 Q = 0, N = 0;
    for (int k = 0; k < kBins; ++k) {
      const uint64_t n = r.n[c][k];
      if (!n) continue;
      Q += r.q[c][k], N += n;
      const double sq = std::sqrt((double)r.q[c][k] / (double)((unsigned __int128)36 * n));
      const double sa = (double)r.a[c][k] / (double)((unsigned __int128)6 * n) * kSqrtPiBy2 * scale;
      s += "bin " + std::to_string(k) + " " + std::to_string(n) + " " + value(true, sq) + " " + value(true, sa) + "\n";
    }
    s += "plane_sigma " + value(N != 0, N != 0 ? std::sqrt((double)Q / (double)(36 * N)) : 0.0) + "\n";
  }
  double hl = 0, hc = 0;
  const bool has_l = strength(r, bit_depth, min_count, 0, &hl).empty(), has_c = strength(r, bit_depth, min_count, 1, &hc).empty();
  s += "auto_strength " + value(has_l, hl) + " " + value(has_c, hc) + "\n";
  return s;
}

}  // namespace g1s_nl
