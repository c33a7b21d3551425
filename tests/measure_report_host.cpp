// measure_report_host.cpp -- csrc/measure_report.cpp on the host under the sanitizers (tests/test_measure_cpu.py builds both
// with -fsanitize=address,undefined and runs this).  Usage: measure_report_host RECORDS
// RECORDS, little-endian: 13 u64 -- frames, pairs, bit_depth, width, height, xdec, ydec, nplanes, the numbers of plain,
// temporal, cross and scale records, with_synth -- then the records of the four kinds in that order, and with_synth times
// the same numbers of records again for the second column.
// Out: for each kind "report KIND BYTES\n" and the report, made from the sums of the records; every report is asked for
// three times: into a buffer of 64 KiB, into one of exactly its size, and into one a byte shorter, which must be refused
// with nothing written past it (the buffers are heap blocks of those sizes: the sanitizer sees a byte too many).  Then each
// sum with a pair that leaves 64 bits, which must be refused with the total untouched, and "refusals ok\n".
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../include/g1s_diff.h"

namespace {

[[noreturn]] void die(const char *what) {
  std::fprintf(stderr, "measure_report_host: %s\n", what);
  std::exit(1);
}

template <class Rec>
std::vector<Rec> read_records(FILE *f, uint64_t n) {
  std::vector<Rec> v(n);
  if (n && std::fread(v.data(), sizeof(Rec), n, f) != n) die("short file");
  return v;
}

// the sum of `recs`; the call must take no records too
template <class Rec, class Sum>
Rec total_of(const std::vector<Rec> &recs, Sum sum) {
  Rec t;
  std::memset(&t, 0xA5, sizeof t);
  if (sum(recs.empty() ? nullptr : recs.data(), recs.size(), &t) != G1S_OK) die("a sum was refused");
  return t;
}

// the report three times over (see above); format(buf, cap) is the call
void print_report(const char *kind, const std::function<long(char *, size_t)> &format) {
  std::vector<char> big(1 << 16);
  const long n = format(big.data(), big.size());
  if (n < 0) die("a report was refused");
  char *exact = static_cast<char *>(std::malloc(n ? (size_t)n : 1));
  if (format(exact, (size_t)n) != n || std::memcmp(exact, big.data(), (size_t)n) != 0) die("a report differs in a buffer of its own size");
  std::free(exact);
  if (n > 0) {
    char *small = static_cast<char *>(std::malloc((size_t)n - 1 ? (size_t)n - 1 : 1));
    if (format(small, (size_t)n - 1) != G1S_ERR_CAPACITY) die("a report fitted a buffer a byte too small");
    std::free(small);
  }
  std::printf("report %s %ld\n", kind, n);
  std::fwrite(big.data(), 1, (size_t)n, stdout);
}

// a pair of records whose entry `field` leaves 64 bits: refused, *total as it was
template <class Rec, class Sum, class Set>
void overflow_refused(Sum sum, Set set) {
  Rec pair[2], total;
  std::memset(pair, 0, sizeof pair);
  set(pair[0]), set(pair[1]);
  std::memset(&total, 0x5A, sizeof total);
  const Rec before = total;
  if (sum(pair, 2, &total) != G1S_ERR_INVALID) die("an overflowing pair was summed");
  if (std::memcmp(&before, &total, sizeof total) != 0) die("a refused sum wrote the total");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) die("usage: measure_report_host RECORDS");
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) die("cannot open the records");
  uint64_t h[13];
  if (std::fread(h, sizeof h[0], 13, f) != 13) die("short header");
  const uint64_t frames = h[0], pairs = h[1];
  const uint32_t bd = (uint32_t)h[2], w = (uint32_t)h[3], ht = (uint32_t)h[4], xdec = (uint32_t)h[5], ydec = (uint32_t)h[6], np = (uint32_t)h[7];
  const bool with_synth = h[12] != 0;
  g1s_measure_record_t plain[2];
  g1s_measure_trecord_t temporal[2];
  g1s_measure_xrecord_t cross[2];
  g1s_measure_srecord_t scales[2];
  for (int col = 0; col < (with_synth ? 2 : 1); ++col) {
    plain[col] = total_of(read_records<g1s_measure_record_t>(f, h[8]), g1s_measure_sum);
    temporal[col] = total_of(read_records<g1s_measure_trecord_t>(f, h[9]), g1s_measure_sum_temporal);
    cross[col] = total_of(read_records<g1s_measure_xrecord_t>(f, h[10]), g1s_measure_sum_cross);
    scales[col] = total_of(read_records<g1s_measure_srecord_t>(f, h[11]), g1s_measure_sum_scales);
  }
  std::fclose(f);
  const int s = with_synth ? 1 : -1;  // (the second column, or none)
  print_report("plain", [&](char *buf, size_t cap) { return g1s_format_measure(&plain[0], s < 0 ? nullptr : &plain[s], frames, bd, w, ht, xdec, ydec, np, buf, cap); });
  print_report("temporal", [&](char *buf, size_t cap) {
    return g1s_format_measure_temporal(&temporal[0], s < 0 ? nullptr : &temporal[s], pairs, bd, w, ht, xdec, ydec, np, buf, cap);
  });
  print_report("cross", [&](char *buf, size_t cap) { return g1s_format_measure_cross(&cross[0], s < 0 ? nullptr : &cross[s], frames, bd, w, ht, xdec, ydec, buf, cap); });
  print_report("scales", [&](char *buf, size_t cap) {
    return g1s_format_measure_scales(&plain[0], &scales[0], s < 0 ? nullptr : &plain[s], s < 0 ? nullptr : &scales[s], frames, bd, np, buf, cap);
  });
  overflow_refused<g1s_measure_record_t>(g1s_measure_sum, [](g1s_measure_record_t &r) { r.s2[2][31] = 1ull << 63; });
  overflow_refused<g1s_measure_record_t>(g1s_measure_sum, [](g1s_measure_record_t &r) { r.r[0][24] = INT64_MIN / 2 - 1; });
  overflow_refused<g1s_measure_trecord_t>(g1s_measure_sum_temporal, [](g1s_measure_trecord_t &r) { r.x[1][0] = INT64_MAX / 2 + 1; });
  overflow_refused<g1s_measure_trecord_t>(g1s_measure_sum_temporal, [](g1s_measure_trecord_t &r) { r.v[2][31] = 1ull << 63; });
  overflow_refused<g1s_measure_xrecord_t>(g1s_measure_sum_cross, [](g1s_measure_xrecord_t &r) { r.c[2][24] = INT64_MIN / 2 - 1; });
  overflow_refused<g1s_measure_xrecord_t>(g1s_measure_sum_cross, [](g1s_measure_xrecord_t &r) { r.n[0][0] = 1ull << 63; });
  overflow_refused<g1s_measure_srecord_t>(g1s_measure_sum_scales, [](g1s_measure_srecord_t &r) { r.s1[2][4][31] = INT64_MAX / 2 + 1; });
  overflow_refused<g1s_measure_srecord_t>(g1s_measure_sum_scales, [](g1s_measure_srecord_t &r) { r.s2[0][0][0] = 1ull << 63; });
  std::printf("refusals ok\n");
  return 0;
}
