// measure_report.cpp -- what `measure` and `check` do with the records once they are on the host: the clip's record from
// its pairs' (g1s_measure_sum*) and the four reports (g1s_format_measure*), rules 5 - 6, 10 - 11, 16 - 17 and 22 - 23 of
// include/g1s_diff.h.  No device, no HIP header, not frame_op.h: builds with a host compiler alone, and
// tests/measure_report_host.cpp runs it under the sanitizers.  Every printed value is formed one operation a step in the
// order of the grammar; tests/measure_ref.py restates them in numpy.
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/g1s_diff.h"

namespace {

constexpr int kBins = 32, kLags = 25, kScales = 5;
constexpr int kTHalo = 2, kTWin = 2 * kTHalo + 1, kTLags = kTWin * kTWin;

bool checked_add(uint64_t &t, uint64_t v) { return !__builtin_add_overflow(t, v, &t); }
bool checked_add(int64_t &t, int64_t v) { return !__builtin_add_overflow(t, v, &t); }

// "%.4f" of v, or "-"
std::string value(bool defined, double v) {
  if (!defined) return "-";
  char s[64];
  snprintf(s, sizeof s, "%.4f", v);
  return s;
}

// the report into the caller's buffer: its size, or G1S_ERR_CAPACITY
long hand_out(const std::string &s, char *buf, size_t cap) {
  if (s.size() > cap) return G1S_ERR_CAPACITY;
  std::memcpy(buf, s.data(), s.size());
  return (long)s.size();
}

// a side of plane c of a frame whose luma side is `luma` (as PlaneGeom of frame_op.h has it: int arithmetic)
int64_t plane_side(uint32_t luma, uint32_t dec, int c) {
  const int side = (int)luma, d = (int)dec;
  return (int64_t)(size_t)(c ? (side + d) >> d : side);
}

// rule 4's offsets in the table's coefficient order, (0, 0) last
void lag_offset(int i, int *dx, int *dy) {
  if (i == 24) *dx = 0, *dy = 0;
  else *dy = i / 7 - 3, *dx = i % 7 - 3;
}

// rule 8's offsets: raster order, (0, 0) is index 12
void temporal_offset(int i, int *dx, int *dy) { *dy = i / kTWin - kTHalo, *dx = i % kTWin - kTHalo; }

// the samples of a pw x ph plane that have their neighbour at offset i inside it: *tw columns of *th rows (false: none).
// A report multiplies them with its count of planes in its own order.
bool lag_extent(void (*offset)(int, int *, int *), int i, int64_t pw, int64_t ph, double *tw, double *th) {
  int dx, dy;
  offset(i, &dx, &dy);
  const int64_t w = pw - std::abs(dx), h = ph - std::abs(dy);
  *tw = (double)w, *th = (double)h;
  return w > 0 && h > 0;
}

struct Profile {
  bool has[kBins];
  double mean[kBins], sigma[kBins];
  bool has_rho[24];
  double rho[24];
};

// the printed values of plane c of a clip's record (one division or one square root a step, in this order)
Profile profile_of(const g1s_measure_record_t &t, int c, const double terms[kLags]) {
  Profile p{};
  for (int k = 0; k < kBins; ++k) {
    p.has[k] = t.n[c][k] > 0;
    if (!p.has[k]) continue;
    const double n = (double)t.n[c][k];
    p.mean[k] = (double)t.s1[c][k] / n;
    const double var = (double)t.s2[c][k] / n - p.mean[k] * p.mean[k];
    p.sigma[k] = std::sqrt(var > 0.0 ? var : 0.0);
  }
  for (int i = 0; i < 24; ++i) {
    p.has_rho[i] = t.r[c][24] != 0 && terms[i] > 0.0;
    if (p.has_rho[i]) p.rho[i] = ((double)t.r[c][i] / terms[i]) / ((double)t.r[c][24] / terms[24]);
  }
  return p;
}

// the printed values of plane c of a clip's temporal record (one operation a step, in the order of the grammar)
struct TProfile {
  bool has_bin[kBins];
  double bin[kBins];
  bool has_lag[kTLags];
  double lag[kTLags];
  int peak;  // the lag of largest |rho|, the first on ties; -1: none is defined
};

TProfile tprofile_of(const g1s_measure_trecord_t &t, int c, const double terms[kTLags]) {
  TProfile p{};
  uint64_t U = 0, V = 0;
  for (int k = 0; k < kBins; ++k) {
    U += t.u[c][k], V += t.v[c][k];
    p.has_bin[k] = t.u[c][k] != 0 && t.v[c][k] != 0;
    if (p.has_bin[k]) p.bin[k] = (double)t.x[c][k] / std::sqrt((double)t.u[c][k] * (double)t.v[c][k]);
  }
  const double T = terms[kTLags / 2];
  p.peak = -1;
  for (int i = 0; i < kTLags; ++i) {
    p.has_lag[i] = U != 0 && V != 0 && terms[i] > 0.0;
    if (!p.has_lag[i]) continue;
    p.lag[i] = ((double)t.c[c][i] / terms[i]) / std::sqrt(((double)U / T) * ((double)V / T));
    if (p.peak < 0 || std::fabs(p.lag[i]) > std::fabs(p.lag[p.peak])) p.peak = i;
  }
  return p;
}

std::string peak_text(const TProfile &p) {
  if (p.peak < 0) return "- - -";
  int dx, dy;
  temporal_offset(p.peak, &dx, &dy);
  return std::to_string(dx) + " " + std::to_string(dy) + " " + value(true, p.lag[p.peak]);
}

// the printed values of a pairing of a cross record: rule 11's profile (the layouts are one), the slopes beside it
struct XProfile {
  TProfile t;
  bool has_slope[kBins], has_beta;
  double slope[kBins], beta;
};

XProfile xprofile_of(const g1s_measure_xrecord_t &r, int j, const double terms[kTLags]) {
  XProfile p{};
  p.t = tprofile_of(r, j, terms);
  uint64_t V = 0;
  for (int k = 0; k < kBins; ++k) {
    V += r.v[j][k];
    p.has_slope[k] = r.v[j][k] != 0;
    if (p.has_slope[k]) p.slope[k] = (double)r.x[j][k] / (double)r.v[j][k];
  }
  p.has_beta = V != 0;
  if (p.has_beta) p.beta = (double)r.c[j][kTLags / 2] / (double)V;
  return p;
}

// partial_rho of the three zero_rho of a column
std::string partial_rho(const XProfile q[3]) {
  const int z = kTLags / 2;
  if (!q[0].t.has_lag[z] || !q[1].t.has_lag[z] || !q[2].t.has_lag[z]) return value(false, 0.0);
  const double r0 = q[0].t.lag[z], r1 = q[1].t.lag[z], r2 = q[2].t.lag[z];
  const double f0 = 1.0 - r0 * r0, f1 = 1.0 - r1 * r1;
  if (f0 <= 0.0 || f1 <= 0.0) return value(false, 0.0);
  return value(true, (r2 - r0 * r1) / std::sqrt(f0 * f1));
}

// the "lag DX DY RHO [RHO]" lines of a temporal profile, or of a pairing's
void lag_lines(std::string &s, const TProfile &a, const TProfile *b) {
  for (int i = 0; i < kTLags; ++i) {
    int dx, dy;
    temporal_offset(i, &dx, &dy);
    s += "lag " + std::to_string(dx) + " " + std::to_string(dy) + " " + value(a.has_lag[i], a.lag[i]);
    if (b) s += " " + value(b->has_lag[i], b->lag[i]);
    s += "\n";
  }
}

struct ScaleColumn {
  bool has_sigma[kScales], has_gain[kScales];
  double sigma[kScales], gain[kScales];
};

// S / m of rule 23 over the bins (n, s1, s2 of one plane and scale, or of a plane of the plain record); false: m = 0
bool pooled_variance(const uint64_t *n, const int64_t *s1, const uint64_t *s2, uint64_t *m_out, double *v) {
  uint64_t m = 0;
  double S = 0.0;
  for (int j = 0; j < kBins; ++j) {
    if (!n[j]) continue;
    m += n[j];
    const double sq = (double)s1[j] * (double)s1[j];
    const double part = sq / (double)n[j];
    S = S + ((double)s2[j] - part);
  }
  *m_out = m;
  if (m) *v = S / (double)m;
  return m != 0;
}

ScaleColumn scale_column(const g1s_measure_record_t &t, const g1s_measure_srecord_t &s, int c) {
  ScaleColumn col{};
  uint64_t m0 = 0, m = 0;
  double v0 = 0.0, v = 0.0;
  const bool has0 = pooled_variance(t.n[c], t.s1[c], t.s2[c], &m0, &v0);
  for (int k = 0; k < kScales; ++k) {
    col.has_sigma[k] = pooled_variance(s.n[c][k], s.s1[c][k], s.s2[c][k], &m, &v);
    if (!col.has_sigma[k]) continue;
    const double L = (double)(2u << k);
    col.sigma[k] = std::sqrt(v > 0.0 ? v : 0.0) / L;
    col.has_gain[k] = has0 && v0 > 0.0;
    if (col.has_gain[k]) {
      const double den = (L * L) * v0;
      col.gain[k] = v / den;
    }
  }
  return col;
}

}  // namespace

extern "C" {

int g1s_measure_sum(const g1s_measure_record_t *recs, size_t n, g1s_measure_record_t *total) {
  if (!total || (n && !recs)) return G1S_ERR_INVALID;
  g1s_measure_record_t t;
  std::memset(&t, 0, sizeof t);
  bool ok = true;
  for (size_t f = 0; f < n; ++f)
    for (int c = 0; c < 3; ++c) {
      for (int k = 0; k < kBins; ++k)
        ok = checked_add(t.n[c][k], recs[f].n[c][k]) && checked_add(t.s1[c][k], recs[f].s1[c][k]) && checked_add(t.s2[c][k], recs[f].s2[c][k]) && ok;
      for (int i = 0; i < kLags; ++i) ok = checked_add(t.r[c][i], recs[f].r[c][i]) && ok;
    }
  if (!ok) return G1S_ERR_INVALID;
  *total = t;
  return G1S_OK;
}

long g1s_format_measure(const g1s_measure_record_t *total, const g1s_measure_record_t *synth, uint64_t frames, uint32_t bit_depth, uint32_t width,
                        uint32_t height, uint32_t xdec, uint32_t ydec, uint32_t nplanes, char *buf, size_t cap) {
  if (!total || (!buf && cap) || (nplanes != 1 && nplanes != 3) || xdec > 1 || ydec > xdec || width < 1 || height < 1) return G1S_ERR_INVALID;
  std::string s = "grainprofile1\n";
  s += "frames " + std::to_string(frames) + " bit_depth " + std::to_string(bit_depth) + " planes " + std::to_string(nplanes) + "\n";
  for (int c = 0; c < (int)nplanes; ++c) {
    s += "plane " + std::to_string(c) + "\n";
    double terms[kLags], tw, th;
    for (int i = 0; i < kLags; ++i)
      terms[i] = lag_extent(lag_offset, i, plane_side(width, xdec, c), plane_side(height, ydec, c), &tw, &th) ? tw * th * (double)frames : 0.0;
    const Profile a = profile_of(*total, c, terms);
    Profile b{};
    if (synth) b = profile_of(*synth, c, terms);
    for (int k = 0; k < kBins; ++k) {
      if (!a.has[k]) continue;
      s += "bin " + std::to_string(k) + " " + std::to_string(total->n[c][k]) + " " + value(true, a.mean[k]) + " " + value(true, a.sigma[k]);
      if (synth) s += " " + value(b.has[k], b.mean[k]) + " " + value(b.has[k], b.sigma[k]);
      s += "\n";
    }
    for (int i = 0; i < 24; ++i) {
      int dx, dy;
      lag_offset(i, &dx, &dy);
      s += "lag " + std::to_string(dx) + " " + std::to_string(dy) + " " + value(a.has_rho[i], a.rho[i]);
      if (synth) s += " " + value(b.has_rho[i], b.rho[i]);
      s += "\n";
    }
    if (synth) {
      bool any = false;
      double worst = 0.0, num = 0.0, den = 0.0;
      for (int i = 0; i < 24; ++i)
        if (a.has_rho[i] && b.has_rho[i]) {
          const double e = std::fabs(b.rho[i] - a.rho[i]);
          worst = !any || e > worst ? e : worst, any = true;
        }
      s += "max_rho_diff " + value(any, worst) + "\n";
      for (int k = 0; k < kBins; ++k)
        if (a.has[k] && b.has[k] && a.sigma[k] > 0.0 && b.sigma[k] > 0.0) {
          const double n = (double)total->n[c][k];
          num += n * (b.sigma[k] / a.sigma[k]), den += n;
        }
      s += "sigma_ratio " + value(den > 0.0, den > 0.0 ? num / den : 0.0) + "\n";
    }
  }
  return hand_out(s, buf, cap);
}

int g1s_measure_sum_temporal(const g1s_measure_trecord_t *recs, size_t n, g1s_measure_trecord_t *total) {
  if (!total || (n && !recs)) return G1S_ERR_INVALID;
  g1s_measure_trecord_t t;
  std::memset(&t, 0, sizeof t);
  bool ok = true;
  for (size_t f = 0; f < n; ++f)
    for (int c = 0; c < 3; ++c) {
      for (int k = 0; k < kBins; ++k)
        ok = checked_add(t.n[c][k], recs[f].n[c][k]) && checked_add(t.x[c][k], recs[f].x[c][k]) && checked_add(t.u[c][k], recs[f].u[c][k]) &&
             checked_add(t.v[c][k], recs[f].v[c][k]) && ok;
      for (int i = 0; i < kTLags; ++i) ok = checked_add(t.c[c][i], recs[f].c[c][i]) && ok;
    }
  if (!ok) return G1S_ERR_INVALID;
  *total = t;
  return G1S_OK;
}

long g1s_format_measure_temporal(const g1s_measure_trecord_t *total, const g1s_measure_trecord_t *synth, uint64_t pairs, uint32_t bit_depth,
                                 uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec, uint32_t nplanes, char *buf, size_t cap) {
  if (!total || (!buf && cap) || (nplanes != 1 && nplanes != 3) || xdec > 1 || ydec > xdec || width < 1 || height < 1) return G1S_ERR_INVALID;
  std::string s = "graintemporal1\n";
  s += "pairs " + std::to_string(pairs) + " bit_depth " + std::to_string(bit_depth) + " planes " + std::to_string(nplanes) + "\n";
  for (int c = 0; c < (int)nplanes; ++c) {
    s += "plane " + std::to_string(c) + "\n";
    if (!pairs) continue;
    double terms[kTLags], tw, th;
    for (int i = 0; i < kTLags; ++i)
      terms[i] = lag_extent(temporal_offset, i, plane_side(width, xdec, c), plane_side(height, ydec, c), &tw, &th) ? (double)pairs * tw * th : 0.0;
    const TProfile a = tprofile_of(*total, c, terms);
    TProfile b{};
    if (synth) b = tprofile_of(*synth, c, terms);
    for (int k = 0; k < kBins; ++k) {
      if (!total->n[c][k]) continue;
      s += "bin " + std::to_string(k) + " " + std::to_string(total->n[c][k]) + " " + value(a.has_bin[k], a.bin[k]);
      if (synth) s += " " + value(b.has_bin[k], b.bin[k]);
      s += "\n";
    }
    lag_lines(s, a, synth ? &b : nullptr);
    s += "temporal_rho " + value(a.has_lag[kTLags / 2], a.lag[kTLags / 2]);
    if (synth) s += " " + value(b.has_lag[kTLags / 2], b.lag[kTLags / 2]);
    s += "\npeak_rho " + peak_text(a);
    if (synth) s += " " + peak_text(b);
    s += "\n";
  }
  return hand_out(s, buf, cap);
}

int g1s_measure_sum_cross(const g1s_measure_xrecord_t *recs, size_t n, g1s_measure_xrecord_t *total) {
  return g1s_measure_sum_temporal(recs, n, total);  // (one type, one body: the pairing stands where the plane does)
}

long g1s_format_measure_cross(const g1s_measure_xrecord_t *total, const g1s_measure_xrecord_t *synth, uint64_t frames, uint32_t bit_depth,
                              uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec, char *buf, size_t cap) {
  if (!total || (!buf && cap) || xdec > 1 || ydec > xdec || width < 1 || height < 1) return G1S_ERR_INVALID;
  static const char *const names[3] = {"cb_luma", "cr_luma", "cb_cr"};
  std::string s = "graincross1\n";
  s += "frames " + std::to_string(frames) + " bit_depth " + std::to_string(bit_depth) + "\n";
  double terms[kTLags], tw, th;
  for (int i = 0; i < kTLags; ++i)
    terms[i] = lag_extent(temporal_offset, i, plane_side(width, xdec, 1), plane_side(height, ydec, 1), &tw, &th) ? (double)frames * tw * th : 0.0;
  XProfile a[3], b[3];
  for (int j = 0; j < 3; ++j) {
    s += std::string("pairing ") + names[j] + "\n";
    if (!frames) continue;
    a[j] = xprofile_of(*total, j, terms);
    if (synth) b[j] = xprofile_of(*synth, j, terms);
    for (int k = 0; k < kBins; ++k) {
      if (!total->n[j][k]) continue;
      s += "bin " + std::to_string(k) + " " + std::to_string(total->n[j][k]) + " " + value(a[j].t.has_bin[k], a[j].t.bin[k]) + " " +
           value(a[j].has_slope[k], a[j].slope[k]);
      if (synth) s += " " + value(b[j].t.has_bin[k], b[j].t.bin[k]) + " " + value(b[j].has_slope[k], b[j].slope[k]);
      s += "\n";
    }
    lag_lines(s, a[j].t, synth ? &b[j].t : nullptr);
    s += "zero_rho " + value(a[j].t.has_lag[kTLags / 2], a[j].t.lag[kTLags / 2]);
    if (synth) s += " " + value(b[j].t.has_lag[kTLags / 2], b[j].t.lag[kTLags / 2]);
    s += "\npeak_rho " + peak_text(a[j].t);
    if (synth) s += " " + peak_text(b[j].t);
    s += "\nbeta " + value(a[j].has_beta, a[j].beta);
    if (synth) s += " " + value(b[j].has_beta, b[j].beta);
    s += "\n";
    if (j == 2) {
      s += "partial_rho " + partial_rho(a);
      if (synth) s += " " + partial_rho(b);
      s += "\n";
    }
  }
  return hand_out(s, buf, cap);
}

int g1s_measure_sum_scales(const g1s_measure_srecord_t *recs, size_t n, g1s_measure_srecord_t *total) {
  if (!total || (n && !recs)) return G1S_ERR_INVALID;
  g1s_measure_srecord_t t;
  std::memset(&t, 0, sizeof t);
  bool ok = true;
  for (size_t f = 0; f < n; ++f)
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < kScales; ++k)
        for (int j = 0; j < kBins; ++j)
          ok = checked_add(t.n[c][k][j], recs[f].n[c][k][j]) && checked_add(t.s1[c][k][j], recs[f].s1[c][k][j]) &&
               checked_add(t.s2[c][k][j], recs[f].s2[c][k][j]) && ok;
  if (!ok) return G1S_ERR_INVALID;
  *total = t;
  return G1S_OK;
}

long g1s_format_measure_scales(const g1s_measure_record_t *total, const g1s_measure_srecord_t *stotal, const g1s_measure_record_t *synth,
                               const g1s_measure_srecord_t *ssynth, uint64_t frames, uint32_t bit_depth, uint32_t nplanes, char *buf, size_t cap) {
  if (!total || !stotal || (!buf && cap) || (nplanes != 1 && nplanes != 3) || (synth == nullptr) != (ssynth == nullptr)) return G1S_ERR_INVALID;
  std::string s = "grainscales1\n";
  s += "frames " + std::to_string(frames) + " bit_depth " + std::to_string(bit_depth) + " planes " + std::to_string(nplanes) + "\n";
  for (int c = 0; c < (int)nplanes; ++c) {
    s += "plane " + std::to_string(c) + "\n";
    if (!frames) continue;
    const ScaleColumn a = scale_column(*total, *stotal, c);
    ScaleColumn b{};
    if (synth) b = scale_column(*synth, *ssynth, c);
    for (int k = 0; k < kScales; ++k) {
      uint64_t m = 0;
      for (int j = 0; j < kBins; ++j) m += stotal->n[c][k][j];
      s += "scale " + std::to_string(k + 1) + " boxes " + std::to_string(m) + " " + value(a.has_sigma[k], a.sigma[k]) + " " +
           value(a.has_gain[k], a.gain[k]);
      if (synth) s += " " + value(b.has_sigma[k], b.sigma[k]) + " " + value(b.has_gain[k], b.gain[k]);
      s += "\n";
    }
    // a bin's own sigma at a scale
    auto bin_sigma = [](const g1s_measure_srecord_t &r, int c_, int k, int j) {
      const double n = (double)r.n[c_][k][j];
      const double mean = (double)r.s1[c_][k][j] / n;
      const double var = (double)r.s2[c_][k][j] / n - mean * mean;
      return std::sqrt(var > 0.0 ? var : 0.0) / (double)(2u << k);
    };
    for (int k = 0; k < kScales; ++k)
      for (int j = 0; j < kBins; ++j) {
        if (!stotal->n[c][k][j]) continue;
        s += "sbin " + std::to_string(k + 1) + " " + std::to_string(j) + " " + std::to_string(stotal->n[c][k][j]) + " " +
             value(true, bin_sigma(*stotal, c, k, j));
        if (synth) s += " " + value(ssynth->n[c][k][j] != 0, ssynth->n[c][k][j] ? bin_sigma(*ssynth, c, k, j) : 0.0);
        s += "\n";
      }
    if (synth)
      for (int k = 0; k < kScales; ++k) {
        const bool both = a.has_gain[k] && b.has_gain[k] && a.gain[k] > 0.0;
        s += "gain_ratio " + std::to_string(k + 1) + " " + value(both, both ? b.gain[k] / a.gain[k] : 0.0) + "\n";
      }
  }
  return hand_out(s, buf, cap);
}

}  // extern "C"
