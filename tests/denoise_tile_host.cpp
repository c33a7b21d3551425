// denoise_tile_host.cpp -- the temporal tile of grav1synth_amd/csrc/denoise_tile.hip.h on the host, thread by thread
// (tests/test_denoise_temporal_cpu.py builds it with the address and undefined-behaviour sanitizers and compares its output
// with tests/denoise_temporal_ref.py).  Every phase of the header takes the thread index as an argument, so a workgroup is
// each phase run for tid = 0 .. 255 in turn, in the order dn_tile_t gives the phases; the end of such a loop is the barrier.
// (Where the barriers of dn_tile_t itself stand is checked by denoise_wg_host.cpp, which runs it with a real barrier.)
//
//   denoise_tile_host BPS S A q W H NNB TABLE IN OUT
//
// TABLE: 1024 u16.  IN: the frame's plane, W x H samples of BPS bytes, then NNB neighbours, each a byte that says whether
// it takes part (0: a null pointer) and a plane.  OUT: the W x H plane, every tile.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../grav1synth_amd/csrc/denoise_tile.hip.h"

using namespace g1s_dn;

namespace {

// a workgroup's registers: what dn_tile_t keeps per thread
struct Thread {
  uint32_t aw[kSPT], au32[kSPT];
  uint64_t au[kSPT];
};

// dn_tile_t with the loop over threads inside every phase: the barrier is the end of each loop
template <int S, int BPS>
void tile(const TileGeom &g, uint8_t *lds, const uint16_t *table, int q, const uint8_t *in, uint32_t stride, const uint8_t *const *nb,
          const uint32_t *nb_stride, int nnb, uint8_t *out, int W, int H, int x0, int y0) {
  uint32_t *Hb = reinterpret_cast<uint32_t *>(lds + g.offH);
  uint16_t *L = reinterpret_cast<uint16_t *>(lds + g.offL), *Wb = reinterpret_cast<uint16_t *>(lds + g.offW),
           *T = reinterpret_cast<uint16_t *>(lds + g.offT), *N = reinterpret_cast<uint16_t *>(lds + g.offN);
  std::vector<Thread> th(kThreads);
#define ALL for (int tid = 0; tid < kThreads; ++tid)
  ALL {
    dn_stage<BPS>(tid, g, L, in, stride, W, H, x0, y0);
    for (int i = tid; i < kTable / 2; i += kThreads) reinterpret_cast<uint32_t *>(T)[i] = reinterpret_cast<const uint32_t *>(table)[i];
  }
  ALL dn_init(tid, g, L, th[tid].aw, th[tid].au32);
  for (int dy = 0; dy <= g.A; ++dy) {
    const int NR = kTH + dy + 2 * S, RH = kTH + dy;
    for (int dx = dy ? -g.A : 1; dx <= g.A; ++dx) {
      const int RW = kTW + (dx < 0 ? -dx : dx);
      ALL dn_hsum<S>(tid, g, L, Hb, dx, dy, RW, NR, magic(NR));
      ALL dn_weights<S>(tid, g, Hb, Wb, T, q, dx, dy, RW, RH, magic(RW), x0, y0, W, H);
      ALL dn_accumulate(tid, g, L, Wb, dx, dy, th[tid].aw, th[tid].au32);
    }
  }
  ALL for (int j = 0; j < kSPT; ++j) th[tid].au[j] = th[tid].au32[j];
  for (int k = 0; k < nnb; ++k) {
    if (!nb[k]) continue;
    ALL dn_stage<BPS>(tid, g, N, nb[k], nb_stride[k], W, H, x0, y0);
    for (int dy = -g.A; dy <= g.A; ++dy)
      for (int dx = -g.A; dx <= g.A; ++dx) {
        ALL dn_hsum_t<S>(tid, g, L, N, Hb, dx, dy);
        ALL dn_weights_t<S>(tid, g, Hb, Wb, T, q, dx, dy, x0, y0, W, H);
        ALL dn_accumulate_t(tid, g, N, Wb, dx, dy, th[tid].aw, th[tid].au);
      }
  }
  ALL dn_store_t<BPS>(tid, out, stride, W, H, x0, y0, th[tid].aw, th[tid].au);
#undef ALL
}

template <int S>
void tile_bps(int bps, const TileGeom &g, uint8_t *lds, const uint16_t *table, int q, const uint8_t *in, uint32_t stride, const uint8_t *const *nb,
              const uint32_t *nb_stride, int nnb, uint8_t *out, int W, int H, int x0, int y0) {
  if (bps == 2) tile<S, 2>(g, lds, table, q, in, stride, nb, nb_stride, nnb, out, W, H, x0, y0);
  else tile<S, 1>(g, lds, table, q, in, stride, nb, nb_stride, nnb, out, W, H, x0, y0);
}

bool read_all(const char *path, std::vector<uint8_t> &v, size_t n) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  v.resize(n);
  const bool ok = std::fread(v.data(), 1, n, f) == n && std::fgetc(f) == EOF;
  std::fclose(f);
  return ok;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 11) return std::fprintf(stderr, "usage: %s BPS S A q W H NNB TABLE IN OUT\n", argv[0]), 2;
  const int bps = std::atoi(argv[1]), S = std::atoi(argv[2]), A = std::atoi(argv[3]), q = std::atoi(argv[4]), W = std::atoi(argv[5]),
            H = std::atoi(argv[6]), nnb = std::atoi(argv[7]);
  if ((bps != 1 && bps != 2) || S < 1 || S > kMaxS || A < 1 || A > kMaxA || W < 1 || H < 1 || nnb < 0 || nnb > 2 * kMaxD) return 2;
  const size_t plane = (size_t)W * H * bps;
  std::vector<uint8_t> table, in;
  if (!read_all(argv[8], table, kTable * 2) || !read_all(argv[9], in, plane + (size_t)nnb * (plane + 1))) return std::fprintf(stderr, "bad input\n"), 2;
  // every plane in an allocation of exactly its size: a read past it is the sanitizer's
  std::vector<std::vector<uint8_t>> planes;
  planes.reserve((size_t)nnb + 1);
  planes.emplace_back(in.begin(), in.begin() + plane);
  const uint8_t *nb[2 * kMaxD] = {};
  uint32_t nb_stride[2 * kMaxD] = {};
  size_t at = plane;
  for (int k = 0; k < nnb; ++k) {
    const bool present = in[at] != 0;
    planes.emplace_back(in.begin() + at + 1, in.begin() + at + 1 + plane);
    at += 1 + plane;
    nb[k] = present ? planes.back().data() : nullptr, nb_stride[k] = (uint32_t)(W * bps);
  }
  const TileGeom g = tile_geom(A, S);
  std::vector<uint8_t> lds((size_t)g.bytes_t), out(plane);
  for (int y0 = 0; y0 < H; y0 += kTH)
    for (int x0 = 0; x0 < W; x0 += kTW) {
      const uint16_t *T = reinterpret_cast<const uint16_t *>(table.data());
      switch (S) {
        case 1: tile_bps<1>(bps, g, lds.data(), T, q, planes[0].data(), (uint32_t)(W * bps), nb, nb_stride, nnb, out.data(), W, H, x0, y0); break;
        case 2: tile_bps<2>(bps, g, lds.data(), T, q, planes[0].data(), (uint32_t)(W * bps), nb, nb_stride, nnb, out.data(), W, H, x0, y0); break;
        case 3: tile_bps<3>(bps, g, lds.data(), T, q, planes[0].data(), (uint32_t)(W * bps), nb, nb_stride, nnb, out.data(), W, H, x0, y0); break;
        default: tile_bps<4>(bps, g, lds.data(), T, q, planes[0].data(), (uint32_t)(W * bps), nb, nb_stride, nnb, out.data(), W, H, x0, y0); break;
      }
    }
  FILE *f = std::fopen(argv[10], "wb");
  if (!f || std::fwrite(out.data(), 1, plane, f) != plane || std::fclose(f) != 0) return std::fprintf(stderr, "cannot write %s\n", argv[10]), 2;
  return 0;
}
