// curve_host.cpp -- curve_row of grav1synth_amd/csrc/curve_row.hip.h (what a lane of kd_curve does with a row) on the host as
// it stands, the 64 lanes one after the other, against the plain lookup.  tests/test_denoise_curve_cpu.py builds it with the
// address and undefined-behaviour sanitizers and runs it; it takes no arguments.
//
// For both directions and byte widths (u8 -> u16 and u16 -> u16 forward, u16 -> u8 and u16 -> u16 back), every width of
// 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65 and a few beyond a wave's first step, three rows a pitch above the row apart, and
// every pair of offsets 0 .. 15 of the two planes' first bytes from a 16-byte address (two-byte samples: the even ones):
// a plane's allocation ends with its extent -- pitch x (rows - 1) + the row -- so a read or a write one byte beyond the
// last row's samples is the sanitizer's, and the bytes between the rows and in front of the plane, filled with a pattern,
// have to come back as they were.  Input values run over the whole sample type, above the
// table's last entry too: they read the last entry.  On success one line on stdout: "rows N".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../grav1synth_amd/csrc/curve_row.hip.h"

using namespace g1s_cv;

namespace {

// a plane of `bytes` bytes whose first byte is `offset` beyond a 16-byte address: the allocation ends with the plane (a
// byte beyond it is the sanitizer's), and the `offset` bytes in front of it hold a pattern that intact() looks at
struct Exact {
  uint8_t *raw, *p;
  size_t offset;
  Exact(size_t bytes, size_t offset_) : raw(static_cast<uint8_t *>(malloc(offset_ + bytes))), p(raw + offset_), offset(offset_) {
    if (!raw || ((uintptr_t)raw & 15)) abort();
    for (size_t i = 0; i < offset; ++i) raw[i] = (uint8_t)(0x3c + i);
  }
  bool intact() const {
    for (size_t i = 0; i < offset; ++i)
      if (raw[i] != (uint8_t)(0x3c + i)) return false;
    return true;
  }
  ~Exact() { free(raw); }
};

uint32_t rnd(uint64_t &s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(s >> 33);
}

template <int BI, int BO>
long run(uint32_t entries, uint64_t &seed) {
  static const uint32_t widths[] = {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65, 1023, 1024, 1025, 1040, 2049};
  std::vector<uint16_t> lut(entries);
  for (uint32_t i = 0; i < entries; ++i) lut[i] = (uint16_t)(BO == 1 ? (i * 7 + 3) & 0xff : (i * 37 + 11) & 0xfff);
  const uint32_t rows = 3, last = entries - 1;
  long done = 0;
  for (uint32_t w : widths)
    for (uint32_t so = 0; so < 16; so += BI)
      for (uint32_t dof = 0; dof < 16 * 2; dof += BO) {
        // a pitch above the row: one that moves the next row's first byte, and (the second round of the offsets) one that
        // keeps the rows' alignment, so rows 1 and 2 take the first row's path
        const bool keep = dof >= 16;
        const uint32_t dofs = dof & 15;
        const size_t srow = (size_t)w * BI, drow = (size_t)w * BO;
        const size_t sp = keep ? (srow + 16 + 15) / 16 * 16 : srow + 2 * BI + (BI == 1 ? 1 : 0), dp = keep ? (drow + 32 + 15) / 16 * 16 : drow + 2 * BO + (BO == 1 ? 3 : 0);
        const size_t sbytes = sp * (rows - 1) + srow, dbytes = dp * (rows - 1) + drow;
        Exact src(sbytes, so), dst(dbytes, dofs);
        for (size_t i = 0; i < sbytes; ++i) src.p[i] = (uint8_t)rnd(seed);
        // (every fourth sample at or above the table's end, the sample type's largest value among them)
        for (uint32_t y = 0; y < rows; ++y)
          for (uint32_t x = 0; x < w; x += 4) store1<BI>(src.p + y * sp, x, (x & 4) ? (BI == 1 ? 0xffu : 0xffffu) : last + (rnd(seed) & 1));
        std::vector<uint8_t> before(src.p, src.p + sbytes), want(dbytes);
        for (size_t i = 0; i < dbytes; ++i) want[i] = dst.p[i] = (uint8_t)(0xa5 ^ i);
        for (uint32_t y = 0; y < rows; ++y)
          for (uint32_t x = 0; x < w; ++x) {
            const uint32_t v = load1<BI>(src.p + y * sp, x);
            store1<BO>(want.data() + y * dp, x, lut[v < last ? v : last]);
          }
        for (uint32_t y = 0; y < rows; ++y)
          for (uint32_t lane = 0; lane < kLanes; ++lane) curve_row<BI, BO>(lut.data(), last, src.p + y * sp, dst.p + y * dp, w, lane);
        if (memcmp(dst.p, want.data(), dbytes) != 0 || memcmp(src.p, before.data(), sbytes) != 0 || !dst.intact() || !src.intact()) {
          fprintf(stderr, "curve_row<%d, %d>: width %u, offsets %u / %u, pitches %zu / %zu: %s\n", BI, BO, w, so, dofs, sp, dp,
                  memcmp(src.p, before.data(), sbytes) ? "the input changed" : "the output differs from the plain lookup");
          exit(1);
        }
        done += rows;
      }
  return done;
}

}  // namespace

int main() {
  uint64_t seed = 12;
  long rows = 0;
  rows += run<1, 2>(256, seed);    // forward, 8 bits
  rows += run<2, 2>(1024, seed);   // forward, 10 bits
  rows += run<2, 1>(4096, seed);   // the inverse, 8 bits
  rows += run<2, 2>(4096, seed);   // the inverse, 10 bits
  printf("rows %ld\n", rows);
  return 0;
}
