// denoise_motion_wg_host.cpp -- the motion tile functions of grav1synth_amd/csrc/denoise_tile.hip.h (dn_motion_tile, dn_tile_tm,
// dn_tile_jtm: what kd_motion, kd_nlm<kMotion> and kd_nlm_j<kMotion> call) on the host as they stand, with a real barrier for `sync`
// (tests/wg_host.h), as tests/denoise_wg_host.cpp runs the four tile functions without motion.  tests/denoise_motion_wg.py
// builds it with the address and undefined-behaviour sanitizers; tests/test_denoise_motion_schedule_cpu.py compares its output
// with the numpy reference under every schedule and fill.
//
//   denoise_motion_wg_host KIND BPS S A q W H XDEC YDEC NNB M TABLE IN OUT SCHEDULE SEED FILL SKIP
//
// KIND      search: one plane, W x H, frame and NNB neighbours: OUT is NNB fields of int8 pairs, blocks in raster order;
//           search_j: a frame's chroma pair (Cb and Cr of (W + XDEC >> XDEC) x (H + YDEC >> YDEC)): the shared field;
//           tile_tm | tile_jtm: the search first (threads ascending, no skip), then the temporal tile function under it.
// M         the motion range on the search plane (Mr / 2), 1 .. 32.
// IN, TABLE, SCHEDULE, SEED, FILL, SKIP and the line on stdout: as denoise_wg_host has them; every neighbour takes part
// or not by its byte.  For tile_tm / tile_jtm, SCHEDULE, FILL and SKIP apply to the filter's tiles, for the search kinds to
// the search.  The LDS buffer is exactly MotionGeom::bytes (the search) or bytes_t (the filter) long.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../grav1synth_amd/csrc/denoise_tile.hip.h"
#include "wg_host.h"

using namespace g1s_dn;

namespace {

struct Run {
  int kind, q, nnb, M, W, H;  // W x H: the plane the tiles cover (the chroma grid for the joint kinds)
  const uint16_t *table;
  const uint8_t *in;
  const uint8_t *nb[2 * kMaxD];
  uint32_t nb_stride[2 * kMaxD];
  uint32_t stride;
  JointPlanes p, jnb[2 * kMaxD];
  JointShape s;
  uint8_t *out, *out2;
  std::vector<int8_t> mv;  // [nnb][blocks] pairs
  wg::Schedule schedule;
  wg::Fill fill;
  long skip;
};

// the fields of every neighbour that takes part (an absent one keeps (0, 0), as kd_motion writes it)
template <int BPS, int NA>
wg::Stats search(Run &r, wg::Schedule &schedule, wg::Fill &fill, long skip, long &nblocks) {
  const MotionGeom m = motion_geom(r.M, NA);
  std::vector<uint8_t> lds((size_t)m.bytes);
  wg::Workgroup group(kThreads);
  wg::Stats st;
  const int bx = (r.W + kTW - 1) / kTW, by = (r.H + kTH - 1) / kTH;
  r.mv.assign((size_t)(2 * r.nnb * bx * by), 0);
  for (int k = 0; k < r.nnb; ++k) {
    MotionPlanes cur, ref;
    if (NA == 2) {
      if (!r.jnb[k].luma) continue;
      cur = MotionPlanes{{r.p.cb, r.p.cr}, {r.p.cb_stride, r.p.cr_stride}};
      ref = MotionPlanes{{r.jnb[k].cb, r.jnb[k].cr}, {r.jnb[k].cb_stride, r.jnb[k].cr_stride}};
    } else {
      if (!r.nb[k]) continue;
      cur = MotionPlanes{{r.in, nullptr}, {r.stride, 0}};
      ref = MotionPlanes{{r.nb[k], nullptr}, {r.nb_stride[k], 0}};
    }
    for (int y = 0; y < by; ++y)
      for (int x = 0; x < bx; ++x, ++nblocks) {
        fill.apply(lds.data(), lds.size());
        uint8_t *l = lds.data();
        int8_t *mv = r.mv.data() + 2 * ((size_t)k * bx * by + (size_t)y * bx + x);
        const int W = r.W, H = r.H;
        st = group.run(schedule, skip, [&m, l, &cur, &ref, W, H, x, y, mv](int tid, wg::Sync sync) {
          dn_motion_tile<BPS, NA>(tid, m, l, cur, ref, W, H, x, y, sync, mv);
        });
      }
  }
  return st;
}

template <int S, int BPS>
wg::Stats tiles(Run &r, int A, long &ntiles) {
  const TileGeom g = tile_geom(A, S);
  const JointGeom jg = joint_geom(g);
  const bool joint = r.kind == 3;
  const size_t bytes = (size_t)(joint ? jg.bytes_t : g.bytes_t);
  std::vector<uint8_t> lds(bytes);
  wg::Workgroup group(kThreads);
  wg::Stats st;
  const int bx = (r.W + kTW - 1) / kTW, by = (r.H + kTH - 1) / kTH;
  for (int y0 = 0; y0 < r.H; y0 += kTH)
    for (int x0 = 0; x0 < r.W; x0 += kTW, ++ntiles) {
      r.fill.apply(lds.data(), bytes);
      uint8_t *l = lds.data();
      const Run &c = r;
      const int8_t *mv = r.mv.data() + 2 * ((y0 / kTH) * bx + x0 / kTW);
      const int mvs = 2 * bx * by;
      if (!joint)
        st = group.run(r.schedule, r.skip, [&c, &g, l, x0, y0, mv, mvs](int tid, wg::Sync sync) {
          dn_tile_tm<S, BPS>(tid, g, l, c.table, c.q, c.in, c.stride, c.nb, c.nb_stride, c.nnb, mv, mvs, c.out, c.stride, c.W, c.H, x0, y0, sync);
        });
      else
        st = group.run(r.schedule, r.skip, [&c, &g, &jg, l, x0, y0, mv, mvs](int tid, wg::Sync sync) {
          const uint32_t os = (uint32_t)(c.s.cw * BPS);
          const JointPlanes *jnb = c.jnb;
          dn_tile_jtm<S, BPS>(tid, g, jg, l, c.table, c.q, c.p, [jnb](int k) { return jnb[k]; }, c.nnb, mv, mvs, c.s, c.out, os, c.out2, os, x0, y0, sync);
        });
    }
  return st;
}

template <int BPS>
wg::Stats run_kind(Run &r, int S, int A, long &n) {
  const bool joint = r.kind == 1 || r.kind == 3;
  if (r.kind < 2) return joint ? search<BPS, 2>(r, r.schedule, r.fill, r.skip, n) : search<BPS, 1>(r, r.schedule, r.fill, r.skip, n);
  wg::Schedule up;
  wg::Schedule::parse("ascending", 0, up);
  wg::Fill zero;
  long nb = 0;
  if (joint) search<BPS, 2>(r, up, zero, -1, nb);
  else search<BPS, 1>(r, up, zero, -1, nb);
  switch (S) {
    case 1: return tiles<1, BPS>(r, A, n);
    case 2: return tiles<2, BPS>(r, A, n);
    case 3: return tiles<3, BPS>(r, A, n);
    default: return tiles<4, BPS>(r, A, n);
  }
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
  if (argc != 19) return std::fprintf(stderr, "usage: %s KIND BPS S A q W H XDEC YDEC NNB M TABLE IN OUT SCHEDULE SEED FILL SKIP\n", argv[0]), 2;
  static const char *const kinds[] = {"search", "search_j", "tile_tm", "tile_jtm"};
  int kind = 0;
  while (kind < 4 && std::strcmp(argv[1], kinds[kind])) ++kind;
  const int bps = std::atoi(argv[2]), S = std::atoi(argv[3]), A = std::atoi(argv[4]), q = std::atoi(argv[5]), W = std::atoi(argv[6]),
            H = std::atoi(argv[7]), xdec = std::atoi(argv[8]), ydec = std::atoi(argv[9]), nnb = std::atoi(argv[10]), M = std::atoi(argv[11]);
  if (kind == 4 || (bps != 1 && bps != 2) || S < 1 || S > kMaxS || A < 1 || A > kMaxA || W < 1 || H < 1 || xdec < 0 || xdec > 1 || ydec < 0 ||
      ydec > 1 || nnb < 1 || nnb > 2 * kMaxD || M < 1 || M > kMaxM)
    return std::fprintf(stderr, "bad arguments\n"), 2;
  Run r = {};
  r.kind = kind, r.q = q, r.nnb = nnb, r.M = M;
  const unsigned long long seed = std::strtoull(argv[16], nullptr, 10);
  if (!wg::Schedule::parse(argv[15], seed, r.schedule)) return std::fprintf(stderr, "unknown schedule %s\n", argv[15]), 2;
  if (!wg::Fill::parse(argv[17], seed, r.fill)) return std::fprintf(stderr, "unknown fill %s\n", argv[17]), 2;
  r.skip = std::atol(argv[18]);

  const bool joint = kind == 1 || kind == 3;
  r.s = JointShape{W, H, xdec, ydec, (W + xdec) >> xdec, (H + ydec) >> ydec};
  r.W = joint ? r.s.cw : W, r.H = joint ? r.s.ch : H;
  const size_t luma = (size_t)W * H * bps, chroma = (size_t)r.s.cw * r.s.ch * bps;
  const size_t frame = joint ? luma + 2 * chroma : luma;
  std::vector<uint8_t> table, in;
  if (!read_all(argv[12], table, kTable * 2) || !read_all(argv[13], in, frame + (size_t)nnb * (frame + 1))) return std::fprintf(stderr, "bad input\n"), 2;
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
  const size_t plane = (size_t)r.W * r.H * bps;
  std::vector<uint8_t> out(plane), out2(joint ? plane : 0);
  r.out = out.data(), r.out2 = out2.data();

  long n = 0;
  const wg::Stats st = bps == 2 ? run_kind<2>(r, S, A, n) : run_kind<1>(r, S, A, n);
  FILE *f = std::fopen(argv[14], "wb");
  bool ok = f != nullptr;
  if (ok && kind < 2) ok = std::fwrite(r.mv.data(), 1, r.mv.size(), f) == r.mv.size();
  else if (ok) ok = std::fwrite(out.data(), 1, out.size(), f) == out.size() && (out2.empty() || std::fwrite(out2.data(), 1, out2.size(), f) == out2.size());
  if (!ok || std::fclose(f) != 0) return std::fprintf(stderr, "cannot write %s\n", argv[14]), 2;
  std::printf("syncs %ld tiles %ld\n", st.syncs, n);
  return 0;
}
