// nlf_t_host.cpp -- the host-only half of the temporal noise levels (grav1synth_amd/csrc/nlf.h, rules T5 - T8) built with a
// host compiler alone, as a stand-alone program: the layout of g1s_nlf_trecord_t as the compiler sees it, then T5's sum,
// T6's level, T7's prior and strengths and T8's report on records made here, each checked against what the rules say in
// closed form.  tests/test_nlf_t_cpu.py compiles it under the address and undefined-behaviour sanitizers and reads the
// layout from its first line.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../grav1synth_amd/csrc/nlf.h"

static void require(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "nlf_t_host: %s\n", what);
    std::exit(1);
  }
}

int main() {
  std::printf("%zu %zu %zu %zu\n", sizeof(g1s_nlf_trecord_t), offsetof(g1s_nlf_trecord_t, n), offsetof(g1s_nlf_trecord_t, s), offsetof(g1s_nlf_trecord_t, q));
  // differences of variance 2 sigma^2 around a mean d: q = n (2 sigma^2 + d^2), s = n d.  sigma = 3 with d = 0 in bin 4,
  // sigma = 3 with d = -7 (a fade) in bin 20, sigma = 6 with d = 5 in bin 12
  g1s_nlf_trecord_t r;
  std::memset(&r, 0, sizeof r);
  const uint64_t n = 5000;
  r.n[0][4] = r.n[0][20] = r.n[0][12] = n;
  r.q[0][4] = 18 * n, r.q[0][20] = (18 + 49) * n, r.q[0][12] = (72 + 25) * n;
  r.s[0][20] = -7 * (int64_t)n, r.s[0][12] = 5 * (int64_t)n;
  require(g1s_nl::level_t(n, 0, 18 * n) == 3 * 256, "t_T = 256 sigma");
  require(g1s_nl::level_t(n, r.s[0][20], r.q[0][20]) == 3 * 256 && g1s_nl::level_t(n, r.s[0][12], r.q[0][12]) == 6 * 256, "with the mean removed");
  require(g1s_nl::level_t(~0ull, INT64_MIN, ~0ull) > 0 && g1s_nl::level_t(~0ull, 0, ~0ull) == 181, "the largest sums stay inside 128 bits");
  require(g1s_nl::level_t(7, 7 * 4095, 7ull * 4095 * 4095) == 0, "a constant difference has no noise");
  for (uint32_t bd = 8; bd <= 10; bd += 2) {
    std::vector<uint8_t> s((size_t)1 << bd);
    require(g1s_nl::sigma_t(r, 0, bd, 0, s.data()).empty(), "three valid bins make a prior");
    const size_t c4 = (4u << (bd - 5)) + (1u << (bd - 6)), c12 = (12u << (bd - 5)) + (1u << (bd - 6)), c20 = (20u << (bd - 5)) + (1u << (bd - 6));
    require(s[0] == 127 && s[c4] == 127 && s[c12] == 255 && s[c20] == 127 && s[s.size() - 1] == 127, "y = floor(255 t / tmax) at the centres and outside");
    double h = 0;
    require(g1s_nl::strength_t(r, bd, 0, 0, &h).empty(), "a strength");
    // Q / N = (18 + 67 + 97) / 3, S / N = -2 / 3
    const double want = std::sqrt(182.0 * (double)n / (3.0 * (double)n) - (-2.0 * (double)n / (3.0 * (double)n)) * (-2.0 * (double)n / (3.0 * (double)n)));
    require(h == want / (double)(1u << (bd - 8)), "h = sqrt(Q / N - (S / N)^2) in 8-bit code values");
    require(g1s_nl::strength_t(r, bd, 0, 1, &h) == "too few smooth samples for a strength", "no chroma");
  }
  uint8_t sc[256];
  require(g1s_nl::sigma_t(r, 1, 8, 0, sc) == "no chroma bin has enough smooth samples for a prior", "no chroma bin");
  r.n[1][3] = r.n[2][3] = n / 2, r.q[1][3] = 18 * (n / 2), r.q[2][3] = 18 * (n / 2) + 50 * (n / 2), r.s[1][3] = -5 * (int64_t)(n / 2),
  r.s[2][3] = 5 * (int64_t)(n / 2);
  require(g1s_nl::sigma_t(r, 1, 8, n, sc).empty() && sc[0] == 255 && sc[255] == 255, "the chroma planes pooled reach the count together");
  r.n[1][3] = ~0ull;
  require(g1s_nl::sigma_t(r, 1, 8, 0, sc) == std::string(g1s_nl::kSumsLeave64), "a pooled sum that leaves 64 bits");
  r.n[1][3] = n / 2;
  r.n[0][4] = r.n[0][12] = r.n[0][20] = g1s_nl::kDefaultMinCount - 1;
  std::vector<uint8_t> s(1024);
  require(g1s_nl::sigma_t(r, 0, 10, 0, s.data()) == "no luma bin has enough smooth samples for a prior", "one below the default count");
  require(g1s_nl::sigma_t(r, 0, 10, g1s_nl::kDefaultMinCount - 1, s.data()).empty(), "on the count");
  double h = 0;
  r.q[0][4] = r.q[0][12] = r.q[0][20] = 0, r.s[0][12] = r.s[0][20] = 0;
  require(g1s_nl::strength_t(r, 10, 1, 0, &h) == "the measured strength is outside 0 < h <= 1000", "no difference at all");
  g1s_nlf_trecord_t two[2], total;
  std::memset(two, 0, sizeof two);
  two[0].s[2][31] = INT64_MIN, two[1].s[2][31] = -1;
  total.n[0][0] = 77;
  require(!g1s_nl::sum_t(two, 2, &total) && total.n[0][0] == 77, "an overflow of s downwards is refused and the total untouched");
  two[0].s[2][31] = INT64_MAX, two[1].s[2][31] = 1;
  require(!g1s_nl::sum_t(two, 2, &total), "and upwards");
  two[1].s[2][31] = 0, two[0].q[1][0] = ~0ull, two[1].q[1][0] = 1;
  require(!g1s_nl::sum_t(two, 2, &total), "and of q");
  two[1].q[1][0] = 0;
  require(g1s_nl::sum_t(two, 2, &total) && total.s[2][31] == INT64_MAX && total.q[1][0] == ~0ull && total.n[0][0] == 0, "the largest sums that fit");
  std::memset(&r, 0, sizeof r);
  require(g1s_nl::report_t(r, nullptr, 0, 8, 1, 0) == "noiselevels_t1\npairs 0 bit_depth 8 planes 1\nplane 0\nplane_sigma_t -\nratio -\nauto_strength_t - -\n",
          "the report of no pair");
  std::printf("ok\n");
  return 0;
}
