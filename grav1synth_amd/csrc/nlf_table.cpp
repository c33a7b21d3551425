// nlf_table.cpp -- the exported host-only functions on lag records (nlf_table.h; the solve is fold.cpp's).  Builds with a
// host compiler alone.
#include "nlf_table.h"

#include <cstdio>
#include <string>

#include <cmath>

#include "fold.h"
#include "nlf.h"

extern "C" void g1s_set_global_error_(const char *text);  // (host_abi.cpp)

// L6 - L7 for plane c into st: the system, the fold's solve, its gain, its chroma fallback.  "" when fine, else the refusal.
static std::string fit_plane(const g1s_nlf_lrecord_t &t, int c, uint32_t bit_depth, int lag, uint64_t min_count, g1s::PlaneState &st) {
  double A[25 * 25], b[25];
  int nc = 0;
  uint64_t N = 0;
  const char *why = g1s_nl::ar_system(t, c, bit_depth, lag, min_count, A, b, &nc, &N);
  if (*why) return why;
  st.ar.resize(nc);
  std::copy(A, A + nc * nc, st.ar.A.begin());
  std::copy(b, b + nc, st.ar.b.begin());
  st.num_observations = (int64_t)N;
  if (!g1s::ar_solve(st, c != 0)) {
    if (c == 0) return "Solving latest noise equation system failed 0!";
    g1s::chroma_fallback(st);
  }
  return "";
}

// L10
std::string g1s_nl::lag_report(const g1s_nlf_lrecord_t &t, uint64_t pairs, uint32_t bit_depth, uint32_t nplanes, uint32_t lag, uint64_t min_count) {
  const uint64_t nmin = min_count_of(min_count);
  std::string s = "noiselags1\n";
  s += "pairs " + std::to_string(pairs) + " bit_depth " + std::to_string(bit_depth) + " planes " + std::to_string(nplanes) + " lag " + std::to_string(lag) + "\n";
  int o[24][2];
  const int m = causal_offsets((int)lag, o);
  for (int c = 0; c < (int)nplanes; ++c) {
    s += "plane " + std::to_string(c) + "\n";
    const uint64_t n0 = t.n[c][0];
    const bool have0 = n0 >= nmin;
    const double mean = have0 ? (double)t.s[c] / (double)n0 : 0.0;
    const double c0 = have0 ? (double)t.r[c][0] / (double)n0 - mean * mean : 0.0;
    g1s::PlaneState st;
    const bool fit = fit_plane(t, c, bit_depth, (int)lag, min_count, st).empty();
    s += "n0 " + std::to_string(n0) + " sigma_t " + value(have0, std::sqrt((c0 > 0.0 ? c0 : 0.0) / 2.0)) + " gain " + value(fit, st.ar_gain) + "\n";
    for (int i = 0; i < m; ++i) {
      const int k = lag_index(o[i][0], o[i][1]);
      const bool ok = have0 && c0 > 0.0 && t.n[c][k] >= nmin;
      const double ci = ok ? (double)t.r[c][k] / (double)t.n[c][k] - mean * mean : 0.0;
      s += "rho " + std::to_string(i) + " " + std::to_string(o[i][0]) + " " + std::to_string(o[i][1]) + " " + value(ok, ok ? ci / c0 : 0.0) + "\n";
    }
    for (int i = 0; i < m; ++i) s += "coef " + std::to_string(i) + " " + value(fit, fit ? st.ar.x[i] : 0.0) + "\n";
    if (c) s += "luma " + value(fit, fit ? st.ar.x[m] : 0.0) + "\n";
  }
  return s;
}

extern "C" {

long g1s_format_noise_lags(const g1s_nlf_lrecord_t *ltotal, uint64_t pairs, uint32_t bit_depth, uint32_t nplanes, uint32_t lag, uint64_t min_count, char *buf,
                           size_t cap) {
  if (!ltotal || (!buf && cap) || (nplanes != 1 && nplanes != 3) || (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) || lag < 1 || lag > 3)
    return G1S_ERR_INVALID;
  const std::string s = g1s_nl::lag_report(*ltotal, pairs, bit_depth, nplanes, lag, min_count);
  if (s.size() > cap) return G1S_ERR_CAPACITY;
  std::memcpy(buf, s.data(), s.size());
  return (long)s.size();
}

int g1s_nlf_sum_lags(const g1s_nlf_lrecord_t *recs, size_t n, g1s_nlf_lrecord_t *total) {
  if (!total || (n && !recs)) return G1S_ERR_INVALID;
  return g1s_nl::sum_lags(recs, n, total) ? G1S_OK : G1S_ERR_INVALID;
}

int g1s_nlf_ar(const g1s_nlf_lrecord_t *ltotal, uint32_t plane, uint32_t bit_depth, uint32_t xdec, uint32_t ydec, uint32_t lag, uint64_t min_count, double x[25],
               double *gain) {
  const auto refuse = [](const std::string &why) {
    g1s_set_global_error_(why.c_str());
    return G1S_ERR_INVALID;
  };
  if (!ltotal || !x || !gain) return refuse("g1s_nlf_ar needs a record and the two outputs");
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return refuse("noise levels are defined for bit depths 8, 10 and 12");
  if (plane > 2 || lag < 1 || lag > 3 || xdec > 1 || ydec > xdec) return refuse("g1s_nlf_ar: plane 0 .. 2, lag 1 .. 3, 4:2:0 / 4:2:2 / 4:4:4");
  g1s::PlaneState st;
  const std::string why = fit_plane(*ltotal, (int)plane, bit_depth, (int)lag, min_count, st);
  if (!why.empty()) return refuse(why);
  const int nc = st.ar.n;
  for (int i = 0; i < 25; ++i) x[i] = i < nc ? st.ar.x[i] : 0.0;
  *gain = st.ar_gain;
  return G1S_OK;
}

int g1s_nlf_table(const g1s_nlf_trecord_t *ttotal, const g1s_nlf_lrecord_t *ltotal, uint32_t bit_depth, uint32_t xdec, uint32_t ydec, uint32_t nplanes,
                  uint32_t lag, uint64_t min_count, g1s_segment_t *out) {
  const auto refuse = [](const std::string &why) {
    g1s_set_global_error_(why.c_str());
    return G1S_ERR_INVALID;
  };
  if (!ttotal || !ltotal || !out) return refuse("g1s_nlf_table needs the two records and the output segment");
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return refuse("noise levels are defined for bit depths 8, 10 and 12");
  if ((nplanes != 1 && nplanes != 3) || lag < 1 || lag > 3 || xdec > 1 || ydec > xdec) return refuse("g1s_nlf_table: 1 or 3 planes, lag 1 .. 3, 4:2:0 / 4:2:2 / 4:4:4");
  const uint64_t nmin = g1s_nl::min_count_of(min_count);
  const int m = (int)g1s::num_coeffs(lag);
  g1s::PlaneState st[3];
  for (int c = 0; c < 3; ++c) st[c].ar.resize(m + (c > 0));  // (a plane the clip lacks: the fold's cleared state)
  const double scale2 = (double)(1u << (2 * (bit_depth - 8)));
  bool points[3] = {false, false, false};
  for (int c = 0; c < (int)nplanes; ++c) {
    const std::string why = fit_plane(*ltotal, c, bit_depth, (int)lag, min_count, st[c]);
    if (!why.empty()) return refuse(why);
    // L8: a measurement a bin with enough samples, in ascending k: N6's centre and the bin's deviation in eight-bit code values,
    // the deviation over the plane's gain as compute_latest has it (chroma: less what the luma curve there explains)
    const double luma_gain = st[0].ar_gain, noise_gain = st[c].ar_gain, corr = c ? st[c].ar.x[m] : 0.0;
    for (int k = 0; k < g1s_nl::kBins; ++k) {
      if (ttotal->n[c][k] < nmin) continue;
      const double centre = (double)(8 * k + 4);
      const double nv = g1s_nl::variance_of(ttotal->n[c][k], ttotal->s[c][k], ttotal->q[c][k]) / 2.0 / scale2;
      const double cl = corr * (c ? luma_gain * st[0].strength.value_at(centre) : 0.0);
      const double t0 = nv / 16, t1 = nv - cl * cl;
      st[c].strength.add_measurement(centre, std::sqrt(t0 > t1 ? t0 : t1) / noise_gain);
      points[c] = true;
    }
    if (c == 0 && !points[0]) return refuse("no luma bin has enough smooth samples for a prior");
    if (points[c] && !st[c].strength.solve()) return refuse("Solving latest noise strength failed!");
  }
  const g1s::PlaneState *ptr[3] = {&st[0], &st[1], &st[2]};
  g1s_segment_t g = g1s::grain_parameters_of(ptr, lag, 0, (uint64_t)INT64_MAX);
  if (!points[1]) g.num_cb_points = 0;
  if (!points[2]) g.num_cr_points = 0;
  *out = g;
  return G1S_OK;
}

}  // extern "C"
