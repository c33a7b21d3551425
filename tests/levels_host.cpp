// levels_host.cpp -- box_lane and add_lane of grav1synth_amd/csrc/levels_row.hip.h (what a lane of kd_down, kd_lowres and
// kd_add does) on the host as they stand, lane after lane in the kernels' own walk, against rules 25 and 27 of
// include/g1s_diff.h as plain loops.  tests/test_denoise_levels_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it; it takes no arguments.
//
// For both sample sizes, widths and heights below, on and above a lane's 8 coarse samples and a wave's 16-byte steps, odd and
// even, and every offset 0 .. 15 of the fine planes' first byte from a 16-byte address with a pitch that moves the next row's
// alignment or keeps it: a fine plane's allocation ends with its extent -- pitch x (rows - 1) + the row -- so a read or a
// write one byte beyond the last row's samples is the sanitizer's, and the bytes between the rows and in front of the plane
// have to come back as they were.  The coarse planes and d are laid out as the denoiser lays out its own: rows on 16-byte
// addresses, padded to 16 bytes.  On success one line on stdout: "planes N".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../grav1synth_amd/csrc/levels_row.hip.h"

using namespace g1s_lv;

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

size_t up16(size_t v) { return (v + 15) / 16 * 16; }

template <int BPS>
int at(const uint8_t *plane, size_t pitch, int x, int y) { return (int)load1<BPS>(plane + (size_t)y * pitch, (uint32_t)x); }

template <int BPS>
int box(const uint8_t *v, size_t pitch, int W, int H, int x, int y) {
  const int x0 = imin(2 * x, W - 1), x1 = imin(2 * x + 1, W - 1), y0 = imin(2 * y, H - 1), y1 = imin(2 * y + 1, H - 1);
  return (at<BPS>(v, pitch, x0, y0) + at<BPS>(v, pitch, x1, y0) + at<BPS>(v, pitch, x0, y1) + at<BPS>(v, pitch, x1, y1) + 2) >> 2;
}

// every lane of every workgroup of the kernels' grid over a W x H fine plane
template <class Fn>
void walk(int W, int H, Fn &&lane) {
  const int CW = (W + 1) >> 1, CH = (H + 1) >> 1;
  for (int ty = 0; ty * kTileRows < CH; ++ty)
    for (int tx = 0; tx * kTileW < CW; ++tx)
      for (int t = 0; t < kThreads; ++t) {
        const int cx0 = tx * kTileW + (t % kTileLanes) * kLaneCoarse, cy = ty * kTileRows + t / kTileLanes;
        if (cx0 < CW && cy < CH) lane(cx0, cy);
      }
}

template <int BPS>
long run(int bits, uint64_t &seed) {
  static const int widths[] = {1, 2, 3, 7, 15, 16, 17, 18, 31, 32, 33, 34, 63, 65, 130, 513, 530};
  static const int heights[] = {1, 2, 3, 5, 16, 17};
  const int maxv = (1 << bits) - 1;
  long done = 0;
  for (int W : widths)
    for (int H : heights)
      for (int off = 0; off < 32; off += BPS) {
        const bool keep = off >= 16;
        const size_t offset = (size_t)(off & 15), row = (size_t)W * BPS;
        const size_t pitch = keep ? up16(row + 16) : row + 2 * BPS + (BPS == 1 ? 1 : 0);
        const size_t bytes = pitch * (size_t)(H - 1) + row;
        const int CW = (W + 1) >> 1, CH = (H + 1) >> 1;
        const size_t crow = up16((size_t)CW * BPS), drow = up16((size_t)CW * 2);
        Exact in(bytes, offset), out(bytes, offset);
        Exact cin(crow * CH, 0), cout(crow * CH, 0), d(drow * CH, 0);
        for (size_t i = 0; i < bytes; ++i) in.p[i] = (uint8_t)rnd(seed), out.p[i] = (uint8_t)rnd(seed);
        // samples over the whole range, the ends of it often: the clip of rule 27 at both ends
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            const uint32_t r = rnd(seed);
            store1<BPS>(in.p + y * pitch, (uint32_t)x, r % (uint32_t)(maxv + 1));
            store1<BPS>(out.p + y * pitch, (uint32_t)x, (r >> 12) % 3 == 0 ? 0u : (r >> 12) % 3 == 1 ? (uint32_t)maxv : (r >> 14) % (uint32_t)(maxv + 1));
          }
        memset(cin.p, 0xee, crow * CH), memset(d.p, 0xee, drow * CH);
        for (size_t i = 0; i < crow * CH; ++i) cout.p[i] = (uint8_t)rnd(seed);
        for (int y = 0; y < CH; ++y)
          for (int x = 0; x < CW; ++x) store1<BPS>(cout.p + y * crow, (uint32_t)x, rnd(seed) % (uint32_t)(maxv + 1));
        const std::vector<uint8_t> in_before(in.p, in.p + bytes), out_before(out.p, out.p + bytes);
        // rule 25
        walk(W, H, [&](int cx0, int cy) { box_lane<false, BPS>(in.p, pitch, W, H, nullptr, 0, cin.p, crow, cx0, cy); });
        for (int y = 0; y < CH; ++y)
          for (int x = 0; x < CW; ++x)
            if (at<BPS>(cin.p, crow, x, y) != box<BPS>(in.p, pitch, W, H, x, y)) {
              fprintf(stderr, "box_lane<false, %d>: %d x %d offset %zu pitch %zu: coarse sample (%d, %d) differs\n", BPS, W, H, offset, pitch, x, y);
              exit(1);
            }
        // rule 27: what the plain loop wants
        std::vector<uint8_t> want(out_before);
        std::vector<int> dd((size_t)CW * CH);
        for (int y = 0; y < CH; ++y)
          for (int x = 0; x < CW; ++x) dd[(size_t)y * CW + x] = at<BPS>(cout.p, crow, x, y) - box<BPS>(out.p, pitch, W, H, x, y);
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            const int xa = x >> 1, ya = y >> 1, xb = imin(imax(xa + ((x & 1) ? 1 : -1), 0), CW - 1), yb = imin(imax(ya + ((y & 1) ? 1 : -1), 0), CH - 1);
            const int s = 9 * dd[(size_t)ya * CW + xa] + 3 * dd[(size_t)ya * CW + xb] + 3 * dd[(size_t)yb * CW + xa] + dd[(size_t)yb * CW + xb] + 8;
            const int U = s >= 0 ? s / 16 : -((-s + 15) / 16);  // floor
            store1<BPS>(want.data() + y * pitch, (uint32_t)x, (uint32_t)imin(imax(at<BPS>(out.p, pitch, x, y) + U, 0), maxv));
          }
        walk(W, H, [&](int cx0, int cy) { box_lane<true, BPS>(out.p, pitch, W, H, cout.p, crow, d.p, drow, cx0, cy); });
        for (int y = 0; y < CH; ++y)
          for (int x = 0; x < CW; ++x)
            if ((int16_t)load1<2>(d.p + y * drow, (uint32_t)x) != dd[(size_t)y * CW + x]) {
              fprintf(stderr, "box_lane<true, %d>: %d x %d offset %zu pitch %zu: d(%d, %d) differs\n", BPS, W, H, offset, pitch, x, y);
              exit(1);
            }
        walk(W, H, [&](int cx0, int cy) { add_lane<BPS>(out.p, pitch, W, H, d.p, drow, cx0, cy, maxv); });
        if (memcmp(out.p, want.data(), bytes) != 0 || memcmp(in.p, in_before.data(), bytes) != 0 || !in.intact() || !out.intact()) {
          fprintf(stderr, "add_lane<%d>: %d x %d offset %zu pitch %zu: %s\n", BPS, W, H, offset, pitch,
                  memcmp(in.p, in_before.data(), bytes) ? "the input changed" : "the output differs from the plain loop, or a byte outside it changed");
          exit(1);
        }
        ++done;
      }
  return done;
}

}  // namespace

int main() {
  uint64_t seed = 27;
  long planes = 0;
  planes += run<1>(8, seed);
  planes += run<2>(10, seed);
  planes += run<2>(12, seed);
  printf("planes %ld\n", planes);
  return 0;
}
