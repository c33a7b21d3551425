// denoise_wg_host.cpp -- the four tile functions of grav1synth_amd/csrc/denoise_tile.hip.h (dn_tile, dn_tile_t, dn_tile_j,
// dn_tile_jt: what kd_nlm and kd_nlm_j call in their forms kPlain and kTemporal) on the host as they stand, with a real barrier for `sync`
// (tests/wg_host.h): 256 logical threads a tile, run one at a time between two barriers in an order the caller names, the
// LDS buffer filled with a pattern before every tile.  tests/denoise_wg.py builds it with the address and undefined-behaviour
// sanitizers; tests/test_denoise_schedule_cpu.py compares its output with the numpy references under every schedule and fill
// -- the composition: the order of the phases, the loops' ranges and where every barrier stands -- and
// tests/test_denoise_temporal_cpu.py and tests/test_denoise_joint_cpu.py over their own content, threads ascending.
//
//   denoise_wg_host KIND BPS S A q W H XDEC YDEC NNB TABLE IN OUT SCHEDULE SEED FILL SKIP
//
// KIND      tile | tile_t: one plane, W x H (XDEC, YDEC ignored; tile: NNB = 0);
//           tile_j | tile_jt: a frame's chroma, (W + XDEC >> XDEC) x (H + YDEC >> YDEC), W x H the luma plane (tile_j: NNB = 0).
// TABLE     1024 u16.
// IN        the frame -- the plane, or Y, Cb, Cr -- in samples of BPS bytes, then NNB neighbours, each a byte that says whether
//           it takes part (0: null pointers) and its plane(s).
// OUT       the plane, or Cb then Cr: every tile.
// SCHEDULE  ascending | descending | waves-reversed | random | stragglers, with SEED (wg_host.h).
// FILL      zero | ones | random: the bytes every tile finds in LDS (random from SEED).
// SKIP      -1, or k: the k-th sync() call (from 0) of every thread of every tile is no barrier.
//
// Every plane lies in an allocation of exactly its size and the LDS buffer is exactly TileGeom / JointGeom `bytes`
// (tile, tile_j) or `bytes_t` long, so a read or write past either is the sanitizer's.  On success one line on stdout:
// "syncs N tiles M": the sync() calls of a thread in a tile (the last tile's), and the tiles run.
//
//   denoise_wg_host selftest early-return | extra-sync
//
// runs a workgroup whose thread 7 returns before a barrier, or calls one barrier more than the others: the executor has to
// end with its message and status 3.
//
//   denoise_wg_host order SCHEDULE SEED INTERVALS
//
// prints the order of the 256 threads in each of the first INTERVALS intervals, a line an interval.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../grav1synth_amd/csrc/denoise_tile.hip.h"
#include "wg_host.h"

using namespace g1s_dn;

namespace {

enum Kind { kTile, kTileT, kTileJ, kTileJT };

struct Run {
  Kind kind;
  int q, nnb, W, H;
  const uint16_t *table;
  // tile, tile_t
  const uint8_t *in;
  const uint8_t *nb[2 * kMaxD];
  uint32_t nb_stride[2 * kMaxD];
  uint32_t stride;
  // tile_j, tile_jt
  JointPlanes p, jnb[2 * kMaxD];
  JointShape s;
  uint8_t *out, *out2;  // the plane; or Cb and Cr
  wg::Schedule schedule;
  wg::Fill fill;
  long skip;
};

template <int S, int BPS>
wg::Stats tiles(Run &r, int A, long &ntiles) {
  const TileGeom g = tile_geom(A, S);
  const JointGeom jg = joint_geom(g);
  const size_t bytes = (size_t)(r.kind == kTile ? g.bytes : r.kind == kTileT ? g.bytes_t : r.kind == kTileJ ? jg.bytes : jg.bytes_t);
  const bool joint = r.kind == kTileJ || r.kind == kTileJT;
  const int pw = joint ? r.s.cw : r.W, ph = joint ? r.s.ch : r.H;
  std::vector<uint8_t> lds(bytes);
  wg::Workgroup group(kThreads);
  wg::Stats st;
  for (int y0 = 0; y0 < ph; y0 += kTH)
    for (int x0 = 0; x0 < pw; x0 += kTW, ++ntiles) {
      r.fill.apply(lds.data(), bytes);
      uint8_t *l = lds.data();
      const Run &c = r;
      switch (r.kind) {
        case kTile:
          st = group.run(r.schedule, r.skip, [&c, &g, l, x0, y0](int tid, wg::Sync sync) {
            dn_tile<S, BPS>(tid, g, l, c.table, c.q, c.in, c.stride, c.out, c.stride, c.W, c.H, x0, y0, sync);
          });
          break;
        case kTileT:
          st = group.run(r.schedule, r.skip, [&c, &g, l, x0, y0](int tid, wg::Sync sync) {
            dn_tile_t<S, BPS>(tid, g, l, c.table, c.q, c.in, c.stride, c.nb, c.nb_stride, c.nnb, c.out, c.stride, c.W, c.H, x0, y0, sync);
          });
          break;
        case kTileJ:
          st = group.run(r.schedule, r.skip, [&c, &g, &jg, l, x0, y0](int tid, wg::Sync sync) {
            const uint32_t os = (uint32_t)(c.s.cw * BPS);
            dn_tile_j<S, BPS>(tid, g, jg, l, c.table, c.q, c.p, c.s, c.out, os, c.out2, os, x0, y0, sync);
          });
          break;
        case kTileJT:
          st = group.run(r.schedule, r.skip, [&c, &g, &jg, l, x0, y0](int tid, wg::Sync sync) {
            const uint32_t os = (uint32_t)(c.s.cw * BPS);
            const JointPlanes *jnb = c.jnb;
            dn_tile_jt<S, BPS>(tid, g, jg, l, c.table, c.q, c.p, [jnb](int k) { return jnb[k]; }, c.nnb, c.s, c.out, os, c.out2, os, x0, y0, sync);
          });
          break;
      }
    }
  return st;
}

template <int S>
wg::Stats tiles_bps(int bps, Run &r, int A, long &ntiles) {
  return bps == 2 ? tiles<S, 2>(r, A, ntiles) : tiles<S, 1>(r, A, ntiles);
}

bool read_all(const char *path, std::vector<uint8_t> &v, size_t n) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  v.resize(n);
  const bool ok = std::fread(v.data(), 1, n, f) == n && std::fgetc(f) == EOF;
  std::fclose(f);
  return ok;
}

int selftest(const char *what) {
  const bool early = !std::strcmp(what, "early-return");
  if (!early && std::strcmp(what, "extra-sync")) return 2;
  wg::Schedule s;
  wg::Schedule::parse("random", 1, s);
  wg::Workgroup group(kThreads);
  std::vector<int> cell(kThreads);
  group.run(s, -1, [&](int tid, wg::Sync sync) {
    cell[(size_t)tid] = tid;
    sync();
    if (early && tid == 7) return;
    sync();
    if (!early && tid == 7) sync();
    cell[(size_t)tid] += cell[(size_t)(tid ^ 1)];
  });
  std::printf("no divergence found\n");
  return 0;
}

int print_order(const char *name, const char *seed, const char *intervals) {
  wg::Schedule s;
  if (!wg::Schedule::parse(name, std::strtoull(seed, nullptr, 10), s)) return std::fprintf(stderr, "unknown schedule %s\n", name), 2;
  std::vector<int> o;
  for (long i = 0; i < std::atol(intervals); ++i) {
    s.order(kThreads, (uint64_t)i, o);
    for (size_t k = 0; k < o.size(); ++k) std::printf("%d%c", o[k], k + 1 == o.size() ? '\n' : ' ');
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 3 && !std::strcmp(argv[1], "selftest")) return selftest(argv[2]);
  if (argc == 5 && !std::strcmp(argv[1], "order")) return print_order(argv[2], argv[3], argv[4]);
  if (argc != 18) return std::fprintf(stderr, "usage: %s KIND BPS S A q W H XDEC YDEC NNB TABLE IN OUT SCHEDULE SEED FILL SKIP\n", argv[0]), 2;
  static const char *const kinds[] = {"tile", "tile_t", "tile_j", "tile_jt"};
  int kind = 0;
  while (kind < 4 && std::strcmp(argv[1], kinds[kind])) ++kind;
  const int bps = std::atoi(argv[2]), S = std::atoi(argv[3]), A = std::atoi(argv[4]), q = std::atoi(argv[5]), W = std::atoi(argv[6]),
            H = std::atoi(argv[7]), xdec = std::atoi(argv[8]), ydec = std::atoi(argv[9]), nnb = std::atoi(argv[10]);
  if (kind == 4 || (bps != 1 && bps != 2) || S < 1 || S > kMaxS || A < 1 || A > kMaxA || W < 1 || H < 1 || xdec < 0 || xdec > 1 || ydec < 0 ||
      ydec > 1 || nnb < 0 || nnb > 2 * kMaxD || ((kind == kTile || kind == kTileJ) && nnb))
    return std::fprintf(stderr, "bad arguments\n"), 2;
  Run r = {};
  r.kind = (Kind)kind, r.q = q, r.nnb = nnb, r.W = W, r.H = H;
  const unsigned long long seed = std::strtoull(argv[15], nullptr, 10);
  if (!wg::Schedule::parse(argv[14], seed, r.schedule)) return std::fprintf(stderr, "unknown schedule %s\n", argv[14]), 2;
  if (!wg::Fill::parse(argv[16], seed, r.fill)) return std::fprintf(stderr, "unknown fill %s\n", argv[16]), 2;
  r.skip = std::atol(argv[17]);

  const bool joint = kind == kTileJ || kind == kTileJT;
  r.s = JointShape{W, H, xdec, ydec, (W + xdec) >> xdec, (H + ydec) >> ydec};
  const size_t luma = (size_t)W * H * bps, chroma = (size_t)r.s.cw * r.s.ch * bps;
  const size_t frame = joint ? luma + 2 * chroma : luma;
  std::vector<uint8_t> table, in;
  if (!read_all(argv[11], table, kTable * 2) || !read_all(argv[12], in, frame + (size_t)nnb * (frame + 1))) return std::fprintf(stderr, "bad input\n"), 2;
  r.table = reinterpret_cast<const uint16_t *>(table.data());
  // every plane in an allocation of exactly its size: a read past it is the sanitizer's
  std::vector<std::vector<uint8_t>> planes;
  planes.reserve(3 * ((size_t)nnb + 1));
  auto take = [&](size_t at, size_t n) {
    planes.emplace_back(in.begin() + at, in.begin() + at + n);
    return planes.back().data();
  };
  auto take_frame = [&](size_t at) {
    const uint8_t *y = take(at, luma), *cb = take(at + luma, chroma), *cr = take(at + luma + chroma, chroma);
    return JointPlanes{cb, cr, y, (uint32_t)(r.s.cw * bps), (uint32_t)(r.s.cw * bps), (uint32_t)(W * bps)};
  };
  r.stride = (uint32_t)(W * bps);
  if (joint) r.p = take_frame(0);
  else r.in = take(0, luma);
  size_t at = frame;
  for (int k = 0; k < nnb; ++k, at += 1 + frame) {
    const bool present = in[at] != 0;
    if (joint) {
      const JointPlanes n = take_frame(at + 1);
      if (present) r.jnb[k] = n;
    } else {
      const uint8_t *n = take(at + 1, luma);
      r.nb[k] = present ? n : nullptr, r.nb_stride[k] = r.stride;
    }
  }
  std::vector<uint8_t> out(joint ? chroma : luma), out2(joint ? chroma : 0);  // (Cb and Cr apart: each is watched)
  r.out = out.data(), r.out2 = out2.data();

  long ntiles = 0;
  wg::Stats st;
  switch (S) {
    case 1: st = tiles_bps<1>(bps, r, A, ntiles); break;
    case 2: st = tiles_bps<2>(bps, r, A, ntiles); break;
    case 3: st = tiles_bps<3>(bps, r, A, ntiles); break;
    default: st = tiles_bps<4>(bps, r, A, ntiles); break;
  }
  FILE *f = std::fopen(argv[13], "wb");
  if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || (!out2.empty() && std::fwrite(out2.data(), 1, out2.size(), f) != out2.size()) || std::fclose(f) != 0)
    return std::fprintf(stderr, "cannot write %s\n", argv[13]), 2;
  std::printf("syncs %ld tiles %ld\n", st.syncs, ntiles);
  return 0;
}
