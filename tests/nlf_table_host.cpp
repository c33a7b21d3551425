// nlf_table_host.cpp -- the host-only half of the lagged noise levels (grav1synth_amd/csrc/nlf_table.cpp, rule L5) built with
// a host compiler alone, as a stand-alone program: the size of g1s_nlf_lrecord_t as the compiler sees it, the exported sum on
// the records of the file given first, written to the file given second, and the refusal of an overflow in every kind of
// field, and the AR fit of rules L6 - L7 (with fold.cpp's solver) on that sum, printed as hexadecimal floats.
// tests/test_nlf_lags_cpu.py compiles it under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../grav1synth_amd/csrc/nlf_table.h"

// (what host_abi.cpp gives the library: where a refusal's text goes)
static std::string g_error;
extern "C" void g1s_set_global_error_(const char *text) { g_error = text ? text : ""; }

static void require(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "nlf_table_host: %s\n", what);
    std::exit(1);
  }
}

int main(int argc, char **argv) {
  require(argc == 3, "usage: nlf_table_host RECORDS SUM");
  std::printf("sizeof %zu\n", sizeof(g1s_nlf_lrecord_t));
  std::FILE *f = std::fopen(argv[1], "rb");
  require(f != nullptr, "cannot open the records");
  std::vector<g1s_nlf_lrecord_t> recs;
  g1s_nlf_lrecord_t one;
  while (std::fread(&one, sizeof one, 1, f) == 1) recs.push_back(one);
  std::fclose(f);
  g1s_nlf_lrecord_t total;
  require(g1s_nlf_sum_lags(recs.data(), recs.size(), &total) == G1S_OK, "the sum of the given records");
  f = std::fopen(argv[2], "wb");
  require(f != nullptr && std::fwrite(&total, sizeof total, 1, f) == 1, "cannot write the sum");
  std::fclose(f);

  int dx, dy;
  g1s_nl::lag_offset(0, &dx, &dy);
  require(dx == 0 && dy == 0, "lag 0");
  g1s_nl::lag_offset(7, &dx, &dy);
  require(dx == -6 && dy == 1, "lag 7");
  g1s_nl::lag_offset(45, &dx, &dy);
  require(dx == 6 && dy == 3, "lag 45");

  // an overflow in each kind of field: refused, the total untouched
  g1s_nlf_lrecord_t two[2];
  const g1s_nlf_lrecord_t before = total;
  for (int kind = 0; kind < 8; ++kind) {
    std::memset(two, 0, sizeof two);
    switch (kind) {
      case 0: two[0].n[2][45] = ~0ull, two[1].n[2][45] = 1; break;
      case 1: two[0].r[1][3] = INT64_MIN, two[1].r[1][3] = -1; break;
      case 2: two[0].s[0] = INT64_MAX, two[1].s[0] = 1; break;
      case 3: two[0].xn[1][24] = ~0ull, two[1].xn[1][24] = 1; break;
      case 4: two[0].xr[0][0] = INT64_MAX, two[1].xr[0][0] = 1; break;
      case 5: two[0].ln = ~0ull, two[1].ln = 1; break;
      case 6: two[0].ls = INT64_MIN, two[1].ls = -1; break;
      default: two[0].l2 = ~0ull, two[1].l2 = 1; break;
    }
    require(g1s_nlf_sum_lags(two, 2, &total) == G1S_ERR_INVALID && !std::memcmp(&total, &before, sizeof total), "an overflow is refused");
    require(g1s_nlf_sum_lags(two, 1, &total) == G1S_OK && !std::memcmp(&total, &two[0], sizeof total), "the largest value alone is fine");
    total = before;
  }
  require(g1s_nlf_sum_lags(nullptr, 1, &total) == G1S_ERR_INVALID && g1s_nlf_sum_lags(two, 2, nullptr) == G1S_ERR_INVALID, "null arguments");
  std::printf("overflow refused\n");

  // L6 - L7 on the sum of the given records, every plane at lag 3; then the default Nmin, which these records do not reach
  g1s_nlf_sum_lags(recs.data(), recs.size(), &total);
  for (uint32_t c = 0; c < 3; ++c) {
    double x[25], gain = 0;
    require(g1s_nlf_ar(&total, c, 10, 1, 1, 3, 400, x, &gain) == G1S_OK, "the fit");
    std::printf("ar %u", c);
    for (double v : x) std::printf(" %a", v);
    std::printf(" %a\n", gain);
  }
  double x[25], gain = 0;
  require(g1s_nlf_ar(&total, 1, 10, 1, 1, 3, 0, x, &gain) == G1S_ERR_INVALID, "too few pairs");
  std::printf("refused: %s\n", g_error.c_str());

  // L10 on the same sum, with a capacity one byte short first
  std::vector<char> text(1 << 14);
  const long w = g1s_format_noise_lags(&total, recs.size(), 10, 3, 3, 400, text.data(), text.size());
  require(w > 0 && g1s_format_noise_lags(&total, recs.size(), 10, 3, 3, 400, text.data(), (size_t)w - 1) == G1S_ERR_CAPACITY, "the report and its capacity");
  std::printf("report-begin\n%.*s", (int)w, text.data());
  return 0;
}
