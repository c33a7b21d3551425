// denoise_joint_tile_host.cpp -- the joint chroma tile of grav1synth_amd/csrc/denoise_tile.hip.h (rules 8 - 11t) on the
// host, thread by thread (tests/test_denoise_joint_cpu.py builds it with the address and undefined-behaviour sanitizers and
// compares its output with tests/denoise_joint_ref.py).  Every phase of the header takes the thread index as an argument, so
// a workgroup is each phase run for tid = 0 .. 255 in turn, in the order dn_tile_j / dn_tile_jt give the phases; the end of
// such a loop is the barrier.  NNB = 0 runs the spatial tile (32-bit sums, dn_store), NNB > 0 the temporal one.
// (Where the barriers of dn_tile_j / dn_tile_jt themselves stand is checked by denoise_wg_host.cpp, with a real barrier.)
//
//   denoise_joint_tile_host BPS S A q W H XDEC YDEC NNB TABLE IN OUT
//
// TABLE: 1024 u16.  IN: the frame's planes Y (W x H), Cb, Cr (cw x ch), samples of BPS bytes, then NNB neighbours, each a
// byte that says whether it takes part (0: null pointers) and its three planes.  OUT: Cb then Cr, cw x ch, every tile.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../grav1synth_amd/csrc/denoise_tile.hip.h"

using namespace g1s_dn;

namespace {

struct Thread {
  uint32_t aw[kSPT], aub32[kSPT], aur32[kSPT];
  uint64_t aub[kSPT], aur[kSPT];
};

template <int S, int BPS>
void tile(const TileGeom &g, const JointGeom &jg, uint8_t *lds, const uint16_t *table, int q, const JointPlanes &p, const JointPlanes *nb, int nnb,
          const JointShape &s, uint8_t *out_cb, uint8_t *out_cr, int x0, int y0) {
  uint32_t *Hb = reinterpret_cast<uint32_t *>(lds + jg.offH);
  uint16_t *L = reinterpret_cast<uint16_t *>(lds + jg.offL), *Wb = reinterpret_cast<uint16_t *>(lds + jg.offW),
           *T = reinterpret_cast<uint16_t *>(lds + jg.offT), *N = reinterpret_cast<uint16_t *>(lds + jg.offN);
  const uint32_t out_stride = (uint32_t)(s.cw * BPS);
  std::vector<Thread> th(kThreads);
#define ALL for (int tid = 0; tid < kThreads; ++tid)
  ALL {
    dn_stage_j<BPS>(tid, g, jg.LP, L, p, s, x0, y0);
    for (int i = tid; i < kTable / 2; i += kThreads) reinterpret_cast<uint32_t *>(T)[i] = reinterpret_cast<const uint32_t *>(table)[i];
  }
  ALL dn_init(tid, g, L, th[tid].aw, th[tid].aub32), dn_init(tid, g, L + jg.LP, th[tid].aw, th[tid].aur32);
  for (int dy = 0; dy <= g.A; ++dy) {
    const int NR = kTH + dy + 2 * S, RH = kTH + dy;
    for (int dx = dy ? -g.A : 1; dx <= g.A; ++dx) {
      const int RW = kTW + (dx < 0 ? -dx : dx);
      ALL dn_hsum_j<S>(tid, g, jg.LP, L, Hb, dx, dy, RW, NR, magic(NR));
      ALL dn_weights<S>(tid, g, Hb, Wb, T, q, dx, dy, RW, RH, magic(RW), x0, y0, s.cw, s.ch);
      ALL dn_accumulate_j(tid, g, jg.LP, L, Wb, dx, dy, th[tid].aw, th[tid].aub32, th[tid].aur32);
    }
  }
  if (!nnb) {
    ALL dn_store<BPS>(tid, out_cb, out_stride, s.cw, s.ch, x0, y0, th[tid].aw, th[tid].aub32);
    ALL dn_store<BPS>(tid, out_cr, out_stride, s.cw, s.ch, x0, y0, th[tid].aw, th[tid].aur32);
    return;
  }
  ALL for (int j = 0; j < kSPT; ++j) th[tid].aub[j] = th[tid].aub32[j], th[tid].aur[j] = th[tid].aur32[j];
  for (int k = 0; k < nnb; ++k) {
    if (!nb[k].luma) continue;
    ALL dn_stage_j<BPS>(tid, g, jg.LP, N, nb[k], s, x0, y0);
    for (int dy = -g.A; dy <= g.A; ++dy)
      for (int dx = -g.A; dx <= g.A; ++dx) {
        ALL dn_hsum_jt<S>(tid, g, jg.LP, L, N, Hb, dx, dy);
        ALL dn_weights_t<S>(tid, g, Hb, Wb, T, q, dx, dy, x0, y0, s.cw, s.ch);
        ALL dn_accumulate_jt(tid, g, jg.LP, N, Wb, dx, dy, th[tid].aw, th[tid].aub, th[tid].aur);
      }
  }
  ALL dn_store_t<BPS>(tid, out_cb, out_stride, s.cw, s.ch, x0, y0, th[tid].aw, th[tid].aub);
  ALL dn_store_t<BPS>(tid, out_cr, out_stride, s.cw, s.ch, x0, y0, th[tid].aw, th[tid].aur);
#undef ALL
}

template <int S, class... Args>
void tile_bps(int bps, Args... args) {
  if (bps == 2) tile<S, 2>(args...);
  else tile<S, 1>(args...);
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
  if (argc != 13) return std::fprintf(stderr, "usage: %s BPS S A q W H XDEC YDEC NNB TABLE IN OUT\n", argv[0]), 2;
  const int bps = std::atoi(argv[1]), S = std::atoi(argv[2]), A = std::atoi(argv[3]), q = std::atoi(argv[4]), W = std::atoi(argv[5]),
            H = std::atoi(argv[6]), xdec = std::atoi(argv[7]), ydec = std::atoi(argv[8]), nnb = std::atoi(argv[9]);
  if ((bps != 1 && bps != 2) || S < 1 || S > kMaxS || A < 1 || A > kMaxA || W < 1 || H < 1 || xdec < 0 || xdec > 1 || ydec < 0 || ydec > 1 || nnb < 0 ||
      nnb > 2 * kMaxD)
    return 2;
  const JointShape s{W, H, xdec, ydec, (W + xdec) >> xdec, (H + ydec) >> ydec};
  const size_t luma = (size_t)W * H * bps, chroma = (size_t)s.cw * s.ch * bps, frame = luma + 2 * chroma;
  std::vector<uint8_t> table, in;
  if (!read_all(argv[10], table, kTable * 2) || !read_all(argv[11], in, frame + (size_t)nnb * (frame + 1))) return std::fprintf(stderr, "bad input\n"), 2;
  // every plane in an allocation of exactly its size: a read past it is the sanitizer's
  std::vector<std::vector<uint8_t>> planes;
  planes.reserve(3 * ((size_t)nnb + 1));
  auto take = [&](size_t at) {
    planes.emplace_back(in.begin() + at, in.begin() + at + luma);
    planes.emplace_back(in.begin() + at + luma, in.begin() + at + luma + chroma);
    planes.emplace_back(in.begin() + at + luma + chroma, in.begin() + at + frame);
    const size_t k = planes.size() - 3;
    return JointPlanes{planes[k + 1].data(), planes[k + 2].data(), planes[k].data(), (uint32_t)(s.cw * bps), (uint32_t)(s.cw * bps), (uint32_t)(W * bps)};
  };
  const JointPlanes p = take(0);
  JointPlanes nb[2 * kMaxD] = {};
  size_t at = frame;
  for (int k = 0; k < nnb; ++k) {
    const bool present = in[at] != 0;
    const JointPlanes n = take(at + 1);
    at += 1 + frame;
    if (present) nb[k] = n;
  }
  const TileGeom g = tile_geom(A, S);
  const JointGeom jg = joint_geom(g);
  std::vector<uint8_t> lds((size_t)(nnb ? jg.bytes_t : jg.bytes)), out(2 * chroma);
  const uint16_t *T = reinterpret_cast<const uint16_t *>(table.data());
  for (int y0 = 0; y0 < s.ch; y0 += kTH)
    for (int x0 = 0; x0 < s.cw; x0 += kTW) {
      switch (S) {
        case 1: tile_bps<1>(bps, g, jg, lds.data(), T, q, p, nb, nnb, s, out.data(), out.data() + chroma, x0, y0); break;
        case 2: tile_bps<2>(bps, g, jg, lds.data(), T, q, p, nb, nnb, s, out.data(), out.data() + chroma, x0, y0); break;
        case 3: tile_bps<3>(bps, g, jg, lds.data(), T, q, p, nb, nnb, s, out.data(), out.data() + chroma, x0, y0); break;
        default: tile_bps<4>(bps, g, jg, lds.data(), T, q, p, nb, nnb, s, out.data(), out.data() + chroma, x0, y0); break;
      }
    }
  FILE *f = std::fopen(argv[12], "wb");
  if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f) != 0) return std::fprintf(stderr, "cannot write %s\n", argv[12]), 2;
  return 0;
}
