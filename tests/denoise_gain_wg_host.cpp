// denoise_gain_wg_host.cpp -- the gain instantiations of the three joint tile functions of
// grav1synth_amd/csrc/denoise_tile.hip.h (dn_tile_j, dn_tile_jt and dn_tile_jtm with a Gain: what the three forms of
// kd_nlm_j<.., GainArg> call) on the host as they stand, with a real barrier for `sync` (tests/wg_host.h), as
// tests/denoise_wg_host.cpp runs the tile functions without a gain -- and, in the same program, rule 24 of
// include/g1s_diff.h as a plain loop over pairs, which the tiles' output is compared with.  tests/denoise_gain_wg.py builds it
// with the address and undefined-behaviour sanitizers; tests/test_denoise_gain_schedule_cpu.py runs it.
//
//   denoise_gain_wg_host KIND BPS S A q W H XDEC YDEC NNB SHIFT TABLE GAIN IN OUT SCHEDULE SEED FILL SKIP
//
// KIND      tile_j | tile_jt | tile_jtm: a frame's chroma, (W + XDEC >> XDEC) x (H + YDEC >> YDEC), W x H the luma plane
//           (tile_j: NNB = 0).
// SHIFT     B - 8: the guide's sample >> SHIFT indexes the gain.
// TABLE     1024 u16.  GAIN: 256 u16.
// IN        the frame -- Y, Cb, Cr -- in samples of BPS bytes, then NNB neighbours, each a byte that says whether it takes
//           part (0: null pointers) and its planes; for tile_jtm then NNB x tiles pairs of int8 (mx, my), a neighbour after
//           the other, tiles in raster order.
// OUT       Cb then Cr: every tile, as the tile functions wrote them.
// SCHEDULE  ascending | descending | waves-reversed | random | stragglers, with SEED (wg_host.h).
// FILL      zero | ones | random: the bytes every tile finds in LDS (random from SEED).
// SKIP      -1, or k: the k-th sync() call (from 0) of every thread of every tile is no barrier.
//
// Every plane lies in an allocation of exactly its size and the LDS buffer is exactly joint_gain_geom(g)'s `bytes` (tile_j)
// or `bytes_t` long, so a read or write past either is the sanitizer's.  One line on stdout: "syncs N tiles M differ K" -- the
// sync() calls of a thread in a tile (the last tile's), the tiles run, and the samples of Cb and Cr that are not the plain
// loop's.  Status 0 whatever K is: the caller looks at it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../grav1synth_amd/csrc/denoise_tile.hip.h"
#include "wg_host.h"

using namespace g1s_dn;

namespace {

enum Kind { kTileJ, kTileJT, kTileJTM };

struct Run {
  Kind kind;
  int q, nnb, bps;
  const uint16_t *table, *gain;
  int shift;
  JointPlanes p, jnb[2 * kMaxD];
  JointShape s;
  const int8_t *mv;  // [nnb][tiles][2]
  int tiles;
  uint8_t *out, *out2;
  wg::Schedule schedule;
  wg::Fill fill;
  long skip;
};

template <int S, int BPS>
wg::Stats tiles(Run &r, int A, long &ntiles) {
  const TileGeom g = tile_geom(A, S);
  const JointGainGeom jg = joint_gain_geom(g);
  const size_t bytes = (size_t)(r.kind == kTileJ ? jg.bytes : jg.bytes_t);
  std::vector<uint8_t> lds(bytes);
  wg::Workgroup group(kThreads);
  wg::Stats st;
  const Gain gain{r.gain, r.shift};
  for (int y0 = 0; y0 < r.s.ch; y0 += kTH)
    for (int x0 = 0; x0 < r.s.cw; x0 += kTW, ++ntiles) {
      r.fill.apply(lds.data(), bytes);
      uint8_t *l = lds.data();
      const Run &c = r;
      const uint32_t os = (uint32_t)(c.s.cw * BPS);
      const JointPlanes *jnb = c.jnb;
      const int8_t *mv = c.mv ? c.mv + 2 * ntiles : nullptr;
      switch (r.kind) {
        case kTileJ:
          st = group.run(r.schedule, r.skip, [&, l, x0, y0](int tid, wg::Sync sync) {
            dn_tile_j<S, BPS>(tid, g, jg, l, c.table, c.q, c.p, c.s, c.out, os, c.out2, os, x0, y0, sync, gain);
          });
          break;
        case kTileJT:
          st = group.run(r.schedule, r.skip, [&, l, x0, y0](int tid, wg::Sync sync) {
            dn_tile_jt<S, BPS>(tid, g, jg, l, c.table, c.q, c.p, [jnb](int k) { return jnb[k]; }, c.nnb, c.s, c.out, os, c.out2, os, x0, y0, sync, gain);
          });
          break;
        case kTileJTM:
          st = group.run(r.schedule, r.skip, [&, l, x0, y0](int tid, wg::Sync sync) {
            dn_tile_jtm<S, BPS>(tid, g, jg, l, c.table, c.q, c.p, [jnb](int k) { return jnb[k]; }, c.nnb, mv, 2 * c.tiles, c.s, c.out, os, c.out2, os,
                                x0, y0, sync, gain);
          });
          break;
      }
    }
  return st;
}

template <int S>
wg::Stats tiles_bps(Run &r, int A, long &ntiles) {
  return r.bps == 2 ? tiles<S, 2>(r, A, ntiles) : tiles<S, 1>(r, A, ntiles);
}

// ---- rule 24 as a plain loop over pairs ------------------------------------------------------------------------------------
int clampi(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }

struct Triple {  // Cb, Cr and the guide (rule 8) of a frame, cw x ch, as 32-bit samples
  std::vector<uint32_t> a[3];
};

uint32_t sample(const uint8_t *base, uint32_t stride, int bps, int x, int y) {
  const uint8_t *row = base + (size_t)y * stride;
  return bps == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(row)[x] : (uint32_t)row[x];
}

Triple triple(const JointPlanes &p, const JointShape &s, int bps) {
  Triple t;
  for (auto &v : t.a) v.resize((size_t)s.cw * s.ch);
  for (int y = 0; y < s.ch; ++y)
    for (int x = 0; x < s.cw; ++x) {
      t.a[0][(size_t)y * s.cw + x] = sample(p.cb, p.cb_stride, bps, x, y);
      t.a[1][(size_t)y * s.cw + x] = sample(p.cr, p.cr_stride, bps, x, y);
      uint32_t sum = 0;
      for (int j = 0; j <= s.ydec; ++j)
        for (int i = 0; i <= s.xdec; ++i) sum += sample(p.luma, p.luma_stride, bps, clampi((x << s.xdec) + i, s.W), clampi((y << s.ydec) + j, s.H));
      t.a[2][(size_t)y * s.cw + x] = (sum + ((1u << (s.xdec + s.ydec)) >> 1)) >> (s.xdec + s.ydec);
    }
  return t;
}

long plain_loop(const Run &r, int A, int S, const uint8_t *got_cb, const uint8_t *got_cr) {
  const int cw = r.s.cw, ch = r.s.ch, tiles_x = (cw + kTW - 1) / kTW;
  const Triple cur = triple(r.p, r.s, r.bps);
  std::vector<Triple> nb((size_t)r.nnb);
  for (int k = 0; k < r.nnb; ++k)
    if (r.jnb[k].luma) nb[(size_t)k] = triple(r.jnb[k], r.s, r.bps);
  auto m_at = [&](uint32_t G) {
    const uint32_t v = G >> r.shift;
    return (uint64_t)r.gain[v < 255 ? v : 255];
  };
  long differ = 0;
  for (int y = 0; y < ch; ++y)
    for (int x = 0; x < cw; ++x) {
      uint64_t num[2] = {0, 0}, den = 0;
      const int tile = (y / kTH) * tiles_x + x / kTW;
      for (int k = -1; k < r.nnb; ++k) {  // -1: the frame itself
        if (k >= 0 && !r.jnb[k].luma) continue;
        const Triple &o = k < 0 ? cur : nb[(size_t)k];
        const int mx = k >= 0 && r.mv ? r.mv[2 * (k * r.tiles + tile)] : 0, my = k >= 0 && r.mv ? r.mv[2 * (k * r.tiles + tile) + 1] : 0;
        for (int dy = -A; dy <= A; ++dy)
          for (int dx = -A; dx <= A; ++dx) {
            const int px = x + mx + dx, py = y + my + dy;
            uint64_t w;
            if (k < 0 && !dx && !dy) {
              w = 4096;
            } else {
              if (px < 0 || px >= cw || py < 0 || py >= ch) continue;
              uint64_t D = 0;
              for (int ky = -S; ky <= S; ++ky)
                for (int kx = -S; kx <= S; ++kx)
                  for (int n = 0; n < 3; ++n) {
                    const int64_t t = (int64_t)cur.a[n][(size_t)clampi(y + ky, ch) * cw + clampi(x + kx, cw)] -
                                      (int64_t)o.a[n][(size_t)clampi(py + ky, ch) * cw + clampi(px + kx, cw)];
                    D += (uint64_t)(t * t);
                  }
              const uint64_t mp = (m_at(cur.a[2][(size_t)y * cw + x]) + m_at(o.a[2][(size_t)py * cw + px]) + 1) >> 1;
              const uint64_t i = (D * mp) >> (r.q + 8);
              w = r.table[i < 1023 ? i : 1023];
            }
            num[0] += w * o.a[0][(size_t)py * cw + px], num[1] += w * o.a[1][(size_t)py * cw + px], den += w;
          }
      }
      const uint8_t *got[2] = {got_cb, got_cr};
      for (int n = 0; n < 2; ++n) {
        const uint64_t want = (num[n] + (den >> 1)) / den;
        const uint64_t have = r.bps == 2 ? reinterpret_cast<const uint16_t *>(got[n])[(size_t)y * cw + x] : got[n][(size_t)y * cw + x];
        differ += want != have;
      }
    }
  return differ;
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
  if (argc != 20) return std::fprintf(stderr, "usage: %s KIND BPS S A q W H XDEC YDEC NNB SHIFT TABLE GAIN IN OUT SCHEDULE SEED FILL SKIP\n", argv[0]), 2;
  static const char *const kinds[] = {"tile_j", "tile_jt", "tile_jtm"};
  int kind = 0;
  while (kind < 3 && std::strcmp(argv[1], kinds[kind])) ++kind;
  const int bps = std::atoi(argv[2]), S = std::atoi(argv[3]), A = std::atoi(argv[4]), q = std::atoi(argv[5]), W = std::atoi(argv[6]),
            H = std::atoi(argv[7]), xdec = std::atoi(argv[8]), ydec = std::atoi(argv[9]), nnb = std::atoi(argv[10]), shift = std::atoi(argv[11]);
  if (kind == 3 || (bps != 1 && bps != 2) || S < 1 || S > kMaxS || A < 1 || A > kMaxA || W < 1 || H < 1 || xdec < 0 || xdec > 1 || ydec < 0 ||
      ydec > 1 || nnb < 0 || nnb > 2 * kMaxD || (kind == kTileJ && nnb) || q < 0 || q > 40 || shift < 0 || shift > 8)
    return std::fprintf(stderr, "bad arguments\n"), 2;
  Run r = {};
  r.kind = (Kind)kind, r.q = q, r.nnb = nnb, r.bps = bps, r.shift = shift;
  const unsigned long long seed = std::strtoull(argv[17], nullptr, 10);
  if (!wg::Schedule::parse(argv[16], seed, r.schedule)) return std::fprintf(stderr, "unknown schedule %s\n", argv[16]), 2;
  if (!wg::Fill::parse(argv[18], seed, r.fill)) return std::fprintf(stderr, "unknown fill %s\n", argv[18]), 2;
  r.skip = std::atol(argv[19]);

  r.s = JointShape{W, H, xdec, ydec, (W + xdec) >> xdec, (H + ydec) >> ydec};
  r.tiles = ((r.s.cw + kTW - 1) / kTW) * ((r.s.ch + kTH - 1) / kTH);
  const size_t luma = (size_t)W * H * bps, chroma = (size_t)r.s.cw * r.s.ch * bps, frame = luma + 2 * chroma;
  const size_t vectors = kind == kTileJTM ? (size_t)nnb * r.tiles * 2 : 0;
  std::vector<uint8_t> table, gain, in;
  if (!read_all(argv[12], table, kTable * 2) || !read_all(argv[13], gain, kGain * 2) || !read_all(argv[14], in, frame + (size_t)nnb * (frame + 1) + vectors))
    return std::fprintf(stderr, "bad input\n"), 2;
  r.table = reinterpret_cast<const uint16_t *>(table.data()), r.gain = reinterpret_cast<const uint16_t *>(gain.data());
  for (int i = 0; i < kGain; ++i)
    if (r.gain[i] < 1 || r.gain[i] > 16384) return std::fprintf(stderr, "bad gain\n"), 2;
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
  r.p = take_frame(0);
  size_t at = frame;
  for (int k = 0; k < nnb; ++k, at += 1 + frame) {
    const bool present = in[at] != 0;
    const JointPlanes n = take_frame(at + 1);
    if (present) r.jnb[k] = n;
  }
  std::vector<int8_t> mv(in.begin() + at, in.end());
  r.mv = vectors ? mv.data() : nullptr;
  std::vector<uint8_t> out(chroma), out2(chroma);  // (Cb and Cr apart: each is watched)
  r.out = out.data(), r.out2 = out2.data();

  long ntiles = 0;
  wg::Stats st;
  switch (S) {
    case 1: st = tiles_bps<1>(r, A, ntiles); break;
    case 2: st = tiles_bps<2>(r, A, ntiles); break;
    case 3: st = tiles_bps<3>(r, A, ntiles); break;
    default: st = tiles_bps<4>(r, A, ntiles); break;
  }
  FILE *f = std::fopen(argv[15], "wb");
  if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fwrite(out2.data(), 1, out2.size(), f) != out2.size() || std::fclose(f) != 0)
    return std::fprintf(stderr, "cannot write %s\n", argv[15]), 2;
  std::printf("syncs %ld tiles %ld differ %ld\n", st.syncs, ntiles, plain_loop(r, A, S, out.data(), out2.data()));
  return 0;
}
