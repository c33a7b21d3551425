// nlf_host.cpp -- the host-only half of the noise levels (grav1synth_amd/csrc/nlf.h, and curve.h's curve from a scaling
// function) built with a host compiler alone, as a stand-alone program: the layout of g1s_nlf_record_t and g1s_nlf_opts_t
// as the compiler sees it, then N4's sum, N5 - N7 and the curve on records made here, each checked against what the rules
// say in closed form.  tests/test_nlf_cpu.py compiles it under the address and undefined-behaviour sanitizers and reads the
// layout from its first line.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../grav1synth_amd/csrc/curve.h"
#include "../grav1synth_amd/csrc/nlf.h"

static void require(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "nlf_host: %s\n", what);
    std::exit(1);
  }
}

int main() {
  std::printf("%zu %zu %zu %zu %zu %zu\n", sizeof(g1s_nlf_record_t), offsetof(g1s_nlf_record_t, n), offsetof(g1s_nlf_record_t, a),
              offsetof(g1s_nlf_record_t, q), sizeof(g1s_nlf_opts_t), offsetof(g1s_nlf_opts_t, batch_frames));
  // white noise of sigma = 3 code values in bins 4 and 20, sigma = 6 in bin 12: q = 36 sigma^2 n
  g1s_nlf_record_t r;
  std::memset(&r, 0, sizeof r);
  const uint64_t n = 5000;
  r.n[0][4] = r.n[0][20] = r.n[0][12] = n;
  r.q[0][4] = r.q[0][20] = 36 * 9 * n, r.q[0][12] = 36 * 36 * n;
  require(g1s_nl::level(r, 0, 4) == 3 * 256 && g1s_nl::level(r, 0, 12) == 6 * 256, "t = 256 sigma");
  for (uint32_t bd = 8; bd <= 10; bd += 2) {
    std::vector<uint8_t> s((size_t)1 << bd);
    require(g1s_nl::sigma(r, bd, 0, s.data()).empty(), "three valid bins make a prior");
    const size_t c4 = (4u << (bd - 5)) + (1u << (bd - 6)), c12 = (12u << (bd - 5)) + (1u << (bd - 6)), c20 = (20u << (bd - 5)) + (1u << (bd - 6));
    require(s[0] == 127 && s[c4] == 127 && s[c12] == 255 && s[c20] == 127 && s[s.size() - 1] == 127, "y = floor(255 t / tmax) at the centres and outside");
    for (size_t v = c4; v < c12; ++v) require(s[v] <= s[v + 1], "rising between the centres");
    for (size_t v = c12; v < c20; ++v) require(s[v] >= s[v + 1], "falling between the centres");
    std::vector<uint16_t> fwd((size_t)1 << bd), inv(4096);
    require(g1s_cv::build_sigma(s.data(), bd, 0, fwd.data(), inv.data()).empty(), "the curve of that s");
    require(g1s_cv::check(bd, fwd.data(), inv.data()).empty(), "and the constructor's checks take it");
    double h = 0;
    require(g1s_nl::strength(r, bd, 0, 0, &h).empty(), "a strength");
    // sigma^2 = (9 + 9 + 36) / 3 = 18; h = sqrt(2 x 18) / 2^(B - 8)
    require(h == 6.0 / (double)(1u << (bd - 8)), "h = sqrt(2) sigma in 8-bit code values");
    require(g1s_nl::strength(r, bd, 0, 1, &h) == "too few smooth samples for a strength", "no chroma");
  }
  r.n[0][4] = r.n[0][12] = r.n[0][20] = g1s_nl::kDefaultMinCount - 1;
  std::vector<uint8_t> s(1024);
  require(g1s_nl::sigma(r, 10, 0, s.data()) == "no luma bin has enough smooth samples for a prior", "one below the default count");
  require(g1s_nl::sigma(r, 10, g1s_nl::kDefaultMinCount - 1, s.data()).empty(), "on the count");
  g1s_nlf_record_t two[2], total;
  std::memset(two, 0, sizeof two);
  two[0].q[2][31] = ~0ull, two[1].q[2][31] = 1;
  total.n[0][0] = 77;
  require(!g1s_nl::sum(two, 2, &total) && total.n[0][0] == 77, "an overflow is refused and the total untouched");
  two[1].q[2][31] = 0;
  require(g1s_nl::sum(two, 2, &total) && total.q[2][31] == ~0ull && total.n[0][0] == 0, "the largest sum that fits");
  require(g1s_nl::isqrt((unsigned __int128)~0ull * ~0ull) == ~0ull && g1s_nl::isqrt(0) == 0 && g1s_nl::isqrt(99) == 9, "isqrt");
  std::printf("ok\n");
  return 0;
}
