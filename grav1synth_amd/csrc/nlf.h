// nlf.h -- what is done with a noise-level record once it is off the device (include/g1s_diff.h, "noise levels", rules N4 -
// N8): the checked sum of records, the levels and the prior's scaling function, the strength, the report.  Host code only:
// it calls nothing of HIP and builds with a host compiler alone.  The kernels that make the records are in nlf.hip.  Behind
// that the same for a temporal record ("temporal noise levels", rules T5 - T8).
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

// the middle field of a record of either kind: a (sums of |L|, unsigned) or s (sums of e, signed)
inline auto &mid(g1s_nlf_record_t &r) { return r.a; }
inline auto &mid(const g1s_nlf_record_t &r) { return r.a; }
inline auto &mid(g1s_nlf_trecord_t &r) { return r.s; }
inline auto &mid(const g1s_nlf_trecord_t &r) { return r.s; }

constexpr const char *kSumsLeave64 = "the clip's sums leave 64 bits";

// N4 and T5: false when a sum leaves 64 bits (then *total is untouched)
template <class Record>
inline bool sum_records(const Record *recs, size_t n, Record *total) {
  Record t;
  std::memset(&t, 0, sizeof t);
  bool ok = true;
  for (size_t f = 0; f < n; ++f)
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < kBins; ++k)
        ok = !__builtin_add_overflow(t.n[c][k], recs[f].n[c][k], &t.n[c][k]) && !__builtin_add_overflow(mid(t)[c][k], mid(recs[f])[c][k], &mid(t)[c][k]) &&
             !__builtin_add_overflow(t.q[c][k], recs[f].q[c][k], &t.q[c][k]) && ok;
  if (ok) *total = t;
  return ok;
}
inline bool sum(const g1s_nlf_record_t *recs, size_t n, g1s_nlf_record_t *total) { return sum_records(recs, n, total); }
inline bool sum_t(const g1s_nlf_trecord_t *recs, size_t n, g1s_nlf_trecord_t *total) { return sum_records(recs, n, total); }

// the ordinary record of the frames with a predecessor: a run's total less its first frame's
inline g1s_nlf_record_t without_first(const g1s_nlf_record_t &total, const g1s_nlf_record_t &first) {
  g1s_nlf_record_t later = total;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < kBins; ++k) later.n[c][k] -= first.n[c][k], later.a[c][k] -= first.a[c][k], later.q[c][k] -= first.q[c][k];
  return later;
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

// N6 on the levels t[k] of the bins with valid[k]: s[1 << B].  false when no bin is valid.
inline bool sigma_of_levels(const bool *is_valid, const uint64_t *t, uint32_t bit_depth, uint8_t *s) {
  int valid[kBins], nvalid = 0;
  uint64_t tmax = 0;
  for (int k = 0; k < kBins; ++k)
    if (is_valid[k]) {
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

// N5 - N6 on the bins (n[k], q[k]): s[1 << B].  false when no bin is valid.
inline bool sigma_of_bins(const unsigned __int128 *n, const unsigned __int128 *q, uint32_t bit_depth, uint64_t min_count, uint8_t *s) {
  const uint64_t nmin = min_count_of(min_count);
  bool valid[kBins];
  uint64_t t[kBins];
  for (int k = 0; k < kBins; ++k)
    if ((valid[k] = n[k] >= nmin)) t[k] = level_of(q[k], n[k]);
  return sigma_of_levels(valid, t, bit_depth, s);
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

// N7 and T7 behind the sums: the refusals, and rms() -- the strength in the clip's code values, asked for only where N
// suffices -- scaled to 8-bit code values.  "" when fine, else the refusal.
template <class Rms>
inline std::string strength_of(unsigned __int128 N, uint32_t bit_depth, uint64_t min_count, Rms rms, double *h) {
  if (N < min_count_of(min_count)) return "too few smooth samples for a strength";
  const double v = rms() / (double)(1u << (bit_depth - 8));
  if (!(v > 0.0 && v <= 1000.0)) return "the measured strength is outside 0 < h <= 1000";
  *h = v;
  return "";
}

// N7 for a plane class (0: luma; 1: the chroma planes pooled).  "" when fine, else the refusal.
inline std::string strength(const g1s_nlf_record_t &r, uint32_t bit_depth, uint64_t min_count, uint32_t plane_class, double *h) {
  unsigned __int128 Q = 0, N = 0;
  for (int c = plane_class ? 1 : 0; c < (plane_class ? 3 : 1); ++c)
    for (int k = 0; k < kBins; ++k) Q += r.q[c][k], N += r.n[c][k];
  return strength_of(N, bit_depth, min_count, [&] { return std::sqrt((2.0 * (double)Q) / (36.0 * (double)N)); }, h);
}

// a value of a report, "-" where it is not defined
inline std::string value(bool defined, double v) {
  if (!defined) return "-";
  char s[64];
  snprintf(s, sizeof s, "%.4f", v);
  return s;
}

// N8
inline std::string report(const g1s_nlf_record_t &r, uint64_t frames, uint32_t bit_depth, uint32_t nplanes, uint64_t min_count) {
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

// ---- temporal noise levels, rules T5 - T8: the same for a record of frame differences ----
// T6: t_T of a bin with sums n > 0, s, q
inline uint64_t level_t(uint64_t n, int64_t s, uint64_t q) {
  const unsigned __int128 a = s < 0 ? (unsigned __int128)0 - (unsigned __int128)(__int128)s : (unsigned __int128)s;
  const unsigned __int128 nq = (unsigned __int128)n * q, ss = a * a;
  const unsigned __int128 d = nq > ss ? nq - ss : 0;  // (sums of integers never make it negative)
  // floor(2^15 d / n), d / n <= q: nothing leaves 128 bits
  const unsigned __int128 x = ((d / n) << 15) + (((d % n) << 15) / n);
  return isqrt(x / n);
}

// the bins a plane class is judged by (0: plane 0; 1: planes 1 and 2 pooled).  false when a pooled sum leaves 64 bits
inline bool class_bins(const g1s_nlf_trecord_t &r, uint32_t plane_class, uint64_t *n, int64_t *s, uint64_t *q) {
  bool ok = true;
  for (int k = 0; k < kBins; ++k) {
    if (!plane_class) n[k] = r.n[0][k], s[k] = r.s[0][k], q[k] = r.q[0][k];
    else
      ok = !__builtin_add_overflow(r.n[1][k], r.n[2][k], &n[k]) && !__builtin_add_overflow(r.s[1][k], r.s[2][k], &s[k]) &&
           !__builtin_add_overflow(r.q[1][k], r.q[2][k], &q[k]) && ok;
  }
  return ok;
}

// T6 - T7: N6 (plane_class 0, at the clip's depth) or N9 (plane_class 1, at B = 8) on t_T.  "" when fine
inline std::string sigma_t(const g1s_nlf_trecord_t &r, uint32_t plane_class, uint32_t bit_depth, uint64_t min_count, uint8_t *out) {
  uint64_t n[kBins], q[kBins], t[kBins];
  int64_t s[kBins];
  bool valid[kBins];
  if (!class_bins(r, plane_class, n, s, q)) return kSumsLeave64;
  const uint64_t nmin = min_count_of(min_count);
  for (int k = 0; k < kBins; ++k)
    if ((valid[k] = n[k] >= nmin)) t[k] = level_t(n[k], s[k], q[k]);
  if (sigma_of_levels(valid, t, plane_class ? 8 : bit_depth, out)) return "";
  return plane_class ? "no chroma bin has enough smooth samples for a prior" : "no luma bin has enough smooth samples for a prior";
}

// Q / N - (S / N)^2 of sums N > 0, S, Q, the two quotients in f64 in that order; not below zero
inline double variance_of(unsigned __int128 N, __int128 S, unsigned __int128 Q) {
  const double m2 = (double)Q / (double)N, m = (double)S / (double)N;
  const double v = m2 - m * m;
  return v > 0.0 ? v : 0.0;
}

// the sums of plane c over all bins
inline void plane_sums(const g1s_nlf_trecord_t &r, int c, unsigned __int128 &N, __int128 &S, unsigned __int128 &Q) {
  for (int k = 0; k < kBins; ++k) N += r.n[c][k], S += r.s[c][k], Q += r.q[c][k];
}

// T7's strength for a plane class.  "" when fine, else N7's refusal.
inline std::string strength_t(const g1s_nlf_trecord_t &r, uint32_t bit_depth, uint64_t min_count, uint32_t plane_class, double *h) {
  unsigned __int128 Q = 0, N = 0;
  __int128 S = 0;
  for (int c = plane_class ? 1 : 0; c < (plane_class ? 3 : 1); ++c) plane_sums(r, c, N, S, Q);
  return strength_of(N, bit_depth, min_count, [&] { return std::sqrt(variance_of(N, S, Q)); }, h);
}

// T8; `ordinary`: the ordinary record of the frames with a predecessor, or null
inline std::string report_t(const g1s_nlf_trecord_t &r, const g1s_nlf_record_t *ordinary, uint64_t pairs, uint32_t bit_depth, uint32_t nplanes,
                            uint64_t min_count) {
  std::string s = "noiselevels_t1\n";
  s += "pairs " + std::to_string(pairs) + " bit_depth " + std::to_string(bit_depth) + " planes " + std::to_string(nplanes) + "\n";
  for (int c = 0; c < (int)nplanes; ++c) {
    s += "plane " + std::to_string(c) + "\n";
    for (int k = 0; k < kBins; ++k) {
      const uint64_t n = r.n[c][k];
      if (!n) continue;
      s += "bin " + std::to_string(k) + " " + std::to_string(n) + " " + value(true, std::sqrt(variance_of(n, r.s[c][k], r.q[c][k]) / 2.0)) + "\n";
    }
    unsigned __int128 Q = 0, N = 0;
    __int128 S = 0;
    plane_sums(r, c, N, S, Q);
    const double st = N != 0 ? std::sqrt(variance_of(N, S, Q) / 2.0) : 0.0;
    s += "plane_sigma_t " + value(N != 0, st) + "\n";
    unsigned __int128 oq = 0, on = 0;
    if (ordinary)
      for (int k = 0; k < kBins; ++k) oq += ordinary->q[c][k], on += ordinary->n[c][k];
    const double so = on != 0 ? std::sqrt((double)oq / (double)(36 * on)) : 0.0;
    s += "ratio " + value(N != 0 && on != 0 && so > 0.0, so > 0.0 ? st / so : 0.0) + "\n";
  }
  double hl = 0, hc = 0;
  const bool has_l = strength_t(r, bit_depth, min_count, 0, &hl).empty(), has_c = strength_t(r, bit_depth, min_count, 1, &hc).empty();
  s += "auto_strength_t " + value(has_l, hl) + " " + value(has_c, hc) + "\n";
  return s;
}

}  // namespace g1s_nl
