// denoise_tile.hip.h -- the phases a workgroup of kd_nlm runs on one tile of one plane (denoise.hip).
//
// The filter is the one include/g1s_diff.h defines under "denoise" (rules 1 - 4).  A tile is kTW x kTH output samples;
// with search radius A and patch radius S the workgroup keeps in LDS
//
//   L   the tile and its halo of R = A + S samples, plane edges replicated while staging: (kTW + 2R) x (kTH + 2R) u16,
//   Hb  for the offset d in hand, the horizontal (2S+1)-sums of the squared differences, u32,
//   Wb  for the offset d in hand, the weight of the pair {p, p + d} at p, u16 (0 where the pair takes no part),
//   T   the 1024-entry weight table.
//
// Only the offsets of the upper half plane are visited (dy > 0, or dy = 0 and dx > 0): D(p, d) = D(p + d, -d), so the
// weight image of d, computed over the union of the tile and the tile moved by -d, serves both ends of every pair --
// a sample p reads Wb at p for its neighbour p + d and at p - d for its neighbour p - d.  Per offset: dn_hsum, barrier,
// dn_weights, barrier, dn_accumulate (into registers; the next dn_hsum writes Hb only, so no third barrier).
//
// The temporal filter (rules 5 - 7, kd_nlm<kTemporal>) adds
//
//   N   the same tile and halo of ONE neighbour frame, in the layout of L; the neighbours that take part are staged one
//       after the other, so LDS does not grow with the temporal radius.
//
// After the offsets of the frame itself, for every neighbour that takes part and every one of its (2A+1)^2 offsets:
// dn_hsum_t (one operand from L, one from N), barrier, dn_weights_t, barrier, dn_accumulate_t.  The region is the tile
// itself (kTW x kTH), whatever the offset: the pair {(t, p), (t + k, p + d)} serves two different output frames, so there
// is no half plane to save, and the weight is read at p only.  Hb and Wb as sized for the frame itself are large enough.
// The numerator of rule 7 needs 64 bits (dn_store over uint64_t).
//
// The joint chroma filter (rules 8 - 11t, kd_nlm_j) runs the same phases over three sample arrays and two output
// planes (JointGeom).  Every phase is written once, over NA sample arrays and NP output planes LP samples apart (one plane: NA =
// NP = 1, LP = 0), as the source says (PlaneSrc, JointSrc); dn_spatial and dn_temporal run them; the tile functions own the registers.
//
// A chroma gain (rules 21 - 24, kd_nlm_j<.., GainArg>) adds, to the joint filter alone,
//
//   Mt  the 256-entry gain table m, u16, behind T; staged in T's loop, under the same first barrier.
//
// The weight phase then reads the guide at both ends of the pair -- G is in LDS already -- and looks both up: D_J is
// multiplied by the pair's mean gain before the shift (dn_weights8).  The phases, their order and their barriers are the
// ones above; without a gain (NoGain, the default of every template here) nothing of it is compiled.
//
// Every phase is a loop over tasks dealt to the threads by `tid`; nothing here names threadIdx, so a host program can
// run a phase for tid = 0 .. kThreads - 1 in turn and get the workgroup's result.  The tile functions (dn_tile, dn_tile_t,
// dn_tile_j, dn_tile_jt), too, are run on the host as they stand, with a real barrier for `sync` and hostile thread orders
// (tests/denoise_wg_host.cpp): that is what checks where the barriers stand, the one left out above included.
#pragma once
#include <stdint.h>

namespace g1s_dn {

constexpr int kThreads = 256;
constexpr int kTW = 64, kTH = 48;   // tile
constexpr int kSPT = kTH / 4;       // output samples a thread owns: column tid & 63, rows (tid >> 6) + 4 j
constexpr int kMaxA = 7, kMaxS = 4;
constexpr int kTable = 1024;
constexpr int kMaxD = 3;            // temporal radius: at most kMaxD frames before and kMaxD after

#if defined(__HIPCC__)
#define G1S_DN_HD __host__ __device__ inline
#else
#define G1S_DN_HD inline
#endif

struct TileGeom {
  int A, S, R;
  int LH, LW, LS;  // staged samples: LH rows of LW, row stride LS (u16); LS / 2 is odd: rows fall on distinct banks
  int HS, HR;      // Hb: HR rows, stride HS (u32, odd)
  int WS, WR;      // Wb: WR rows, stride WS (u16)
  int offH, offL, offW, offT, bytes;
  int offN, bytes_t;  // the temporal kernel's LDS: the same buffers and N behind them
};

G1S_DN_HD TileGeom tile_geom(int A, int S) {
  TileGeom g;
  g.A = A, g.S = S, g.R = A + S;
  g.LW = kTW + 2 * g.R, g.LH = kTH + 2 * g.R;
  g.LS = (g.LW + 1) & ~1;
  if (!((g.LS >> 1) & 1)) g.LS += 2;
  g.HS = (kTW + A) | 1, g.HR = kTH + A + 2 * S;
  g.WS = (kTW + A + 1) & ~1, g.WR = kTH + A;
  g.offH = 0;
  g.offL = g.offH + g.HS * g.HR * 4;
  g.offW = (g.offL + g.LS * g.LH * 2 + 15) & ~15;
  g.offT = (g.offW + g.WS * g.WR * 2 + 15) & ~15;
  g.bytes = g.offT + kTable * 2;
  g.offN = (g.bytes + 15) & ~15;
  g.bytes_t = g.offN + g.LS * g.LH * 2;
  return g;
}

// Luma-guided joint chroma (rules 8 - 11t, kd_nlm_j): Cb, Cr and the guide G as one weight.
//
// Three sample arrays in the layout of L, JointGeom::LP samples apart: Cb, Cr, G.  G is the frame's input luma at chroma
// resolution (rule 8), formed while staging.  Hb, Wb and T are the ones of tile_geom: the squared differences of the three
// arrays are summed in registers before the sliding sum (rule 9, exact in uint32_t; dn_weights and dn_weights_t work in
// uint32_t already), the weights are made once, and one read of Wb feeds the accumulators of both chroma planes.  The
// temporal kernel keeps the three arrays of one neighbour frame behind them.
struct JointGeom {
  int LP;  // samples from one array to the next
  int offH, offL, offW, offT, bytes;
  int offN, bytes_t;
};

G1S_DN_HD JointGeom joint_geom(const TileGeom &g) {
  JointGeom j;
  j.LP = (g.LS * g.LH + 7) & ~7;
  j.offH = 0;
  j.offL = g.HS * g.HR * 4;
  j.offW = (j.offL + 3 * j.LP * 2 + 15) & ~15;
  j.offT = (j.offW + g.WS * g.WR * 2 + 15) & ~15;
  j.bytes = j.offT + kTable * 2;
  j.offN = (j.bytes + 15) & ~15;
  j.bytes_t = j.offN + 3 * j.LP * 2;
  return j;
}

// The same under a chroma gain (rules 21 - 24): the gain table Mt behind T, and N behind that
constexpr int kGain = 256;  // entries of a chroma gain (rule 21)
struct JointGainGeom : JointGeom {
  int offM;
};

G1S_DN_HD JointGainGeom joint_gain_geom(const TileGeom &g) {
  JointGainGeom j;
  static_cast<JointGeom &>(j) = joint_geom(g);
  j.offM = j.offT + kTable * 2;
  j.bytes = j.offM + kGain * 2;
  j.offN = (j.bytes + 15) & ~15;
  j.bytes_t = j.offN + 3 * j.LP * 2;
  return j;
}

G1S_DN_HD int dn_lp(const TileGeom &) { return 0; }  // samples from one array to the next under either layout
G1S_DN_HD int dn_lp(const JointGeom &j) { return j.LP; }

// A chroma gain (rules 21 - 24) as the phases see it.  Gain is what a tile function is handed: m[256] in global memory and
// B - 8.  GainLds is the same once staged: Mt in LDS, the guide arrays of the frame (G) and of the neighbour in hand (GN).
// GainPair is one task of dn_weights8: the guide down a column at both ends of the pair, rows LS apart.  NoGain is
// empty: a phase instantiated with it is the phase without a gain.  Under a gain the layout is JointGainGeom.
struct NoGain {
  static constexpr bool on = false;
};
struct Gain {
  static constexpr bool on = true;
  const uint16_t *table;
  int shift;
};
struct GainLds {
  static constexpr bool on = true;
  const uint16_t *Mt, *G, *GN;
  int shift;
};
struct GainPair {
  static constexpr bool on = true;
  const uint16_t *Mt, *ga, *gb;
  int shift;
};
// rule 24's v(p) -> m: a sample above the bit depth's maximum (the caller's error) stays a wrong value, never a wrong address
G1S_DN_HD uint32_t dn_gain_at(const uint16_t *Mt, uint32_t G, int shift) {
  const uint32_t v = G >> shift;
  return Mt[v < (uint32_t)(kGain - 1) ? v : (uint32_t)(kGain - 1)];
}

G1S_DN_HD int imin(int a, int b) { return a < b ? a : b; }
G1S_DN_HD int imax(int a, int b) { return a > b ? a : b; }
// i / n == (i * magic(n)) >> 16 for 0 <= i < 512, 1 <= n <= 128
G1S_DN_HD uint32_t magic(int n) { return (65536u + (uint32_t)n - 1u) / (uint32_t)n; }

// the tile at (x0, y0) of a W x H plane and its halo into L; coordinates clamp to the plane (rule 1)
template <int BPS>
G1S_DN_HD void dn_stage(int tid, const TileGeom &g, uint16_t *L, const uint8_t *in, uint32_t stride, int W, int H, int x0, int y0) {
  for (int r = tid >> 7; r < g.LH; r += kThreads >> 7) {
    const int gy = imin(imax(y0 - g.R + r, 0), H - 1);
    const uint8_t *row = in + (size_t)gy * stride;
    for (int c = tid & 127; c < g.LW; c += 128) {
      const int gx = imin(imax(x0 - g.R + c, 0), W - 1);
      L[r * g.LS + c] = BPS == 2 ? reinterpret_cast<const uint16_t *>(row)[gx] : (uint16_t)row[gx];
    }
  }
}

template <int BPS>
G1S_DN_HD uint32_t dn_sample(const uint8_t *row, int x) { return BPS == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(row)[x] : (uint32_t)row[x]; }

// rule 8 into L: the tile at (x0, y0) of the cw x ch chroma grid and its halo, chroma coordinates clamped to that grid;
// each sample the rounded mean of a (1 << xdec) x (1 << ydec) box of the W x H luma plane, luma coordinates clamped to it
template <int BPS>
G1S_DN_HD void dn_stage_guide(int tid, const TileGeom &g, uint16_t *L, const uint8_t *luma, uint32_t stride, int W, int H, int xdec, int ydec, int cw,
                              int ch, int x0, int y0) {
  const int sh = xdec + ydec;
  const uint32_t half = (1u << sh) >> 1;
  for (int r = tid >> 7; r < g.LH; r += kThreads >> 7) {
    const int gy = imin(imax(y0 - g.R + r, 0), ch - 1) << ydec;
    const uint8_t *row0 = luma + (size_t)imin(gy, H - 1) * stride, *row1 = luma + (size_t)imin(gy + ydec, H - 1) * stride;
    for (int c = tid & 127; c < g.LW; c += 128) {
      const int gx = imin(imax(x0 - g.R + c, 0), cw - 1) << xdec;
      const int xa = imin(gx, W - 1), xb = imin(gx + xdec, W - 1);
      uint32_t s = dn_sample<BPS>(row0, xa);
      if (xdec) s += dn_sample<BPS>(row0, xb);
      if (ydec) {
        s += dn_sample<BPS>(row1, xa);
        if (xdec) s += dn_sample<BPS>(row1, xb);
      }
      L[r * g.LS + c] = (uint16_t)((s + half) >> sh);
    }
  }
}

// what a joint tile reads and writes: the two chroma planes (cw x ch), the luma plane the guide comes from (W x H)
struct JointPlanes {
  const uint8_t *cb, *cr, *luma;
  uint32_t cb_stride, cr_stride, luma_stride;
};
struct JointShape {
  int W, H, xdec, ydec, cw, ch;
};

// Cb, Cr and G of one frame's tile into the three arrays from L
template <int BPS>
G1S_DN_HD void dn_stage_j(int tid, const TileGeom &g, int LP, uint16_t *L, const JointPlanes &p, const JointShape &s, int x0, int y0) {
  dn_stage<BPS>(tid, g, L, p.cb, p.cb_stride, s.cw, s.ch, x0, y0);
  dn_stage<BPS>(tid, g, L + LP, p.cr, p.cr_stride, s.cw, s.ch, x0, y0);
  dn_stage_guide<BPS>(tid, g, L + 2 * LP, p.luma, p.luma_stride, s.W, s.H, s.xdec, s.ydec, s.cw, s.ch, x0, y0);
}

// A source is what one frame's tile is staged from: NA sample arrays LP apart, the first NP of them output planes; the
// grid its weights are bounded by; whether the clip has the frame at all (a null pointer: it has not, rule 5).
struct PlaneSrc {  // one plane
  static constexpr int NP = 1, NA = 1;
  const uint8_t *in;
  uint32_t stride;
  int W, H;
  G1S_DN_HD bool present() const { return in != nullptr; }
  G1S_DN_HD int grid_w() const { return W; }
  G1S_DN_HD int grid_h() const { return H; }
  template <int BPS>
  G1S_DN_HD void stage(int tid, const TileGeom &g, int, uint16_t *L, int x0, int y0) const { dn_stage<BPS>(tid, g, L, in, stride, W, H, x0, y0); }
};
struct JointSrc {  // Cb and Cr, and the guide beside them
  static constexpr int NP = 2, NA = 3;
  JointPlanes p;
  const JointShape &s;
  G1S_DN_HD bool present() const { return p.luma != nullptr; }
  G1S_DN_HD int grid_w() const { return s.cw; }
  G1S_DN_HD int grid_h() const { return s.ch; }
  template <int BPS>
  G1S_DN_HD void stage(int tid, const TileGeom &g, int LP, uint16_t *L, int x0, int y0) const { dn_stage_j<BPS>(tid, g, LP, L, p, s, x0, y0); }
};

// o[j] = sum over the NA arrays and |kx| <= S of (a[j + S + kx] - b[j + S + kx])^2 for j < 8: the squared differences of a
// column summed in registers (exact in uint32_t), then the sliding sum
template <int S, int NA>
G1S_DN_HD void dn_slide8(const uint16_t *a, const uint16_t *b, int LP, uint32_t *o) {
  uint32_t sq[8 + 2 * S];
#pragma unroll
  for (int j = 0; j < 8 + 2 * S; ++j) {
    sq[j] = 0;
#pragma unroll
    for (int n = 0; n < NA; ++n) {
      const int t = (int)a[n * LP + j] - (int)b[n * LP + j];
      sq[j] += (uint32_t)(t * t);
    }
  }
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j <= 2 * S; ++j) s += sq[j];
  o[0] = s;
#pragma unroll
  for (int j = 1; j < 8; ++j) {
    s += sq[j + 2 * S] - sq[j - 1];
    o[j] = s;
  }
}

// Hb(row, x) = sum over the arrays and |kx| <= S of (L(x + kx, r) - L(x + dx + kx, r + dy))^2 for the region's columns x (RW
// of them, from -max(dx, 0)) and its rows r = -dy - S + row, row < NR = kTH + dy + 2S.  A task is 8 consecutive columns of a
// row (the last task of a row starts at RW - 8 and overlaps its neighbour); lanes run down the rows.  mNR = magic(NR).
template <int S, int NA>
G1S_DN_HD void dn_hsum(int tid, const TileGeom &g, int LP, const uint16_t *L, uint32_t *Hb, int dx, int dy, int RW, int NR, uint32_t mNR) {
  const int ntasks = ((RW + 7) >> 3) * NR;
  const int ox = -imax(dx, 0);
  for (int i = tid; i < ntasks; i += kThreads) {
    const int seg = (int)(((uint32_t)i * mNR) >> 16), row = i - seg * NR;
    const int xs = imin(seg * 8, RW - 8);
    const uint16_t *a = L + (row + g.A - dy) * g.LS + (ox + xs - S + g.R);
    dn_slide8<S, NA>(a, a + dy * g.LS + dx, LP, Hb + row * g.HS + xs);
  }
}

// Hb(row, x) = sum over the arrays and |kx| <= S of (L(x + kx, r) - N(x + dx + kx, r + dy))^2 for the tile's columns x < kTW and
// the rows r = row - S, row < kTH + 2S; dx and dy of either sign.  Tasks as in dn_hsum, but none overlaps another: 8 divides kTW.
template <int S, int NA>
G1S_DN_HD void dn_hsum_t(int tid, const TileGeom &g, int LP, const uint16_t *L, const uint16_t *N, uint32_t *Hb, int dx, int dy) {
  constexpr int NR = kTH + 2 * S, ntasks = (kTW >> 3) * NR;
  const uint32_t mNR = magic(NR);
  for (int i = tid; i < ntasks; i += kThreads) {
    const int seg = (int)(((uint32_t)i * mNR) >> 16), row = i - seg * NR;
    const int xs = seg * 8;
    dn_slide8<S, NA>(L + (row + g.A) * g.LS + (xs + g.A), N + (row + g.A + dy) * g.LS + (xs + g.A + dx), LP, Hb + row * g.HS + xs);
  }
}

// o[j WS] = T[min(D >> q, 1023)] with D = the sum of Hb over the 2S + 1 rows from h + j HS, for 8 consecutive rows of a
// column; 0 where the pair takes no part, which is what ok(j) says.  Under a gain (rule 24) D is multiplied by the pair's
// mp <= 2^14 first: a 64-bit product below 2^46 (one v_mul_hi_u32 / v_mul_lo_u32 pair), shifted by q + 8.
template <int S, class Ok, class Gp = NoGain>
G1S_DN_HD void dn_weights8(const TileGeom &g, const uint32_t *h, uint16_t *o, const uint16_t *T, int q, Ok ok, Gp gp = Gp()) {
  uint32_t v[8 + 2 * S];
#pragma unroll
  for (int j = 0; j < 8 + 2 * S; ++j) v[j] = h[j * g.HS];
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j <= 2 * S; ++j) s += v[j];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j) s += v[j + 2 * S] - v[j - 1];
    uint32_t k;
    if constexpr (Gp::on) {
      const uint32_t mp = (dn_gain_at(gp.Mt, gp.ga[j * g.LS], gp.shift) + dn_gain_at(gp.Mt, gp.gb[j * g.LS], gp.shift) + 1u) >> 1;
      const uint64_t kk = ((uint64_t)s * mp) >> (q + 8);
      k = kk < (uint64_t)(kTable - 1) ? (uint32_t)kk : (uint32_t)(kTable - 1);
    } else {
      k = s >> q;
    }
    const uint16_t w = T[k < (uint32_t)(kTable - 1) ? k : (uint32_t)(kTable - 1)];
    o[j * g.WS] = ok(j) ? w : (uint16_t)0;
  }
}

// Wb(y, x) = the weight of the pair {p, p + d} for the region's RW x RH samples p = (x0 - max(dx, 0) + x, y0 - dy + y); 0
// where p or p + d lies outside the W x H grid (rule 2).  A task is 8 consecutive rows of a column (the last task of a
// column starts at RH - 8 and overlaps its neighbour); lanes run along the columns.
template <int S, class Gl = NoGain>
G1S_DN_HD void dn_weights(int tid, const TileGeom &g, const uint32_t *Hb, uint16_t *Wb, const uint16_t *T, int q, int dx, int dy, int RW,
                          int RH, uint32_t mRW, int x0, int y0, int W, int H, Gl gl = Gl()) {
  const int ntasks = ((RH + 7) >> 3) * RW;
  for (int i = tid; i < ntasks; i += kThreads) {
    const int seg = (int)(((uint32_t)i * mRW) >> 16), x = i - seg * RW;
    const int ys = imin(seg * 8, RH - 8);
    const int px = x0 - imax(dx, 0) + x, py = y0 - dy + ys;
    const bool col_ok = px >= 0 && px < W && px + dx >= 0 && px + dx < W;
    if constexpr (Gl::on) {
      // the guide at p and at p + d: both inside L, whose halo of R covers the region and the region moved by d
      const uint16_t *ga = gl.G + (ys - dy + g.R) * g.LS + (x - imax(dx, 0) + g.R);
      dn_weights8<S>(g, Hb + ys * g.HS + x, Wb + ys * g.WS + x, T, q, [=](int j) { return col_ok && py + j >= 0 && py + j + dy < H; },
                     GainPair{gl.Mt, ga, ga + dy * g.LS + dx, gl.shift});
    } else {
      dn_weights8<S>(g, Hb + ys * g.HS + x, Wb + ys * g.WS + x, T, q,
                     [=](int j) { return col_ok && py + j >= 0 && py + j + dy < H; });  // (dy >= 0: the other two row bounds follow)
    }
  }
}

// Wb(y, x) = the weight of the pair {(t, p), (t + k, p + d)} for the tile's samples p = (x0 + x, y0 + y); 0 where p or p + d
// lies outside the W x H grid (rule 6).  Tasks as in dn_weights, and no task overlaps another: 8 divides kTH.  Under motion
// (rule 19) the neighbour was staged from the tile moved by (mx, my), and it is p + m + d that has to lie inside.  Under a gain
// the neighbour's guide is read at p + d of N, which is G of frame t + k at p + m + d (rule 24).
template <int S, class Gl = NoGain>
G1S_DN_HD void dn_weights_t(int tid, const TileGeom &g, const uint32_t *Hb, uint16_t *Wb, const uint16_t *T, int q, int dx, int dy, int x0,
                            int y0, int W, int H, int mx = 0, int my = 0, Gl gl = Gl()) {
  constexpr int ntasks = (kTH >> 3) * kTW;
  const int ox = mx + dx, oy = my + dy;
  for (int i = tid; i < ntasks; i += kThreads) {
    const int x = i % kTW, ys = i / kTW * 8;
    const int px = x0 + x, py = y0 + ys;
    const bool col_ok = px < W && px + ox >= 0 && px + ox < W;
    if constexpr (Gl::on) {
      dn_weights8<S>(g, Hb + ys * g.HS + x, Wb + ys * g.WS + x, T, q, [=](int j) { return col_ok && py + j < H && py + j + oy >= 0 && py + j + oy < H; },
                     GainPair{gl.Mt, gl.G + (ys + g.R) * g.LS + (x + g.R), gl.GN + (ys + dy + g.R) * g.LS + (x + dx + g.R), gl.shift});
    } else {
      dn_weights8<S>(g, Hb + ys * g.HS + x, Wb + ys * g.WS + x, T, q,
                     [=](int j) { return col_ok && py + j < H && py + j + oy >= 0 && py + j + oy < H; });
    }
  }
}

// the two pairs of offset d at each sample the thread owns: {p, p + d}, weight at p, and {p - d, p}, weight at p - d
template <int NP>
G1S_DN_HD void dn_accumulate(int tid, const TileGeom &g, int LP, const uint16_t *L, const uint16_t *Wb, int dx, int dy, uint32_t *aw,
                             uint32_t *const (&au)[NP]) {
  const int x = tid & 63, yb = tid >> 6;
  const uint16_t *w1 = Wb + (yb + dy) * g.WS + x + imax(dx, 0);
  const uint16_t *w2 = Wb + yb * g.WS + x + imax(-dx, 0);
  const uint16_t *u1 = L + (yb + dy + g.R) * g.LS + x + dx + g.R;
  const uint16_t *u2 = L + (yb - dy + g.R) * g.LS + x - dx + g.R;
#pragma unroll
  for (int j = 0; j < kSPT; ++j) {
    const uint32_t a = w1[4 * j * g.WS], b = w2[4 * j * g.WS];
    aw[j] += a + b;
#pragma unroll
    for (int n = 0; n < NP; ++n) au[n][j] += a * u1[n * LP + 4 * j * g.LS] + b * u2[n * LP + 4 * j * g.LS];  // (the weights: read once)
  }
}

// the pair {(t, p), (t + k, p + d)} at each sample the thread owns: weight at p, sample from N
template <int NP>
G1S_DN_HD void dn_accumulate_t(int tid, const TileGeom &g, int LP, const uint16_t *N, const uint16_t *Wb, int dx, int dy, uint32_t *aw,
                               uint64_t *const (&au)[NP]) {
  const int x = tid & 63, yb = tid >> 6;
  const uint16_t *w = Wb + yb * g.WS + x;
  const uint16_t *u = N + (yb + dy + g.R) * g.LS + x + dx + g.R;
#pragma unroll
  for (int j = 0; j < kSPT; ++j) {
    const uint32_t a = w[4 * j * g.WS];
    aw[j] += a;
#pragma unroll
    for (int n = 0; n < NP; ++n) au[n][j] += (uint64_t)a * u[n * LP + 4 * j * g.LS];
  }
}

// d = 0: weight T[0] = 4096 on the sample itself
template <int NP>
G1S_DN_HD void dn_init(int tid, const TileGeom &g, int LP, const uint16_t *L, uint32_t *aw, uint32_t *const (&au)[NP]) {
  const uint16_t *u = L + ((tid >> 6) + g.R) * g.LS + (tid & 63) + g.R;
#pragma unroll
  for (int j = 0; j < kSPT; ++j) {
    aw[j] = 4096u;
#pragma unroll
    for (int n = 0; n < NP; ++n) au[n][j] = 4096u * u[n * LP + 4 * j * g.LS];
  }
}

// (n + (d >> 1)) / d for a quotient below 2^16 (a weighted mean of samples), d < 2^24: the float quotient is within one
// of the integer one (its relative error is a few 2^-24), and one step either way makes it exact
G1S_DN_HD uint32_t dn_rounded_mean(uint64_t n, uint32_t d) {
  n += d >> 1;
  uint32_t v = (uint32_t)((float)n * (1.0f / (float)d));
  const int64_t r = (int64_t)n - (int64_t)((uint64_t)v * d);
  if (r < 0) --v;
  else if (r >= (int64_t)d) ++v;
  return v;
}

// rules 4 and 7: one rounded division per sample; the numerator of rule 7 (Num = uint64_t) needs 64 bits
template <int BPS, class Num>
G1S_DN_HD void dn_store(int tid, uint8_t *out, uint32_t stride, int W, int H, int x0, int y0, const uint32_t *aw, const Num *au) {
  const int x = x0 + (tid & 63);
  if (x >= W) return;
#pragma unroll
  for (int j = 0; j < kSPT; ++j) {
    const int y = y0 + (tid >> 6) + 4 * j;
    if (y >= H) break;
    const uint32_t v = sizeof(Num) == 8 ? dn_rounded_mean(au[j], aw[j]) : (uint32_t)((au[j] + (aw[j] >> 1)) / aw[j]);
    uint8_t *row = out + (size_t)y * stride;
    if (BPS == 2) reinterpret_cast<uint16_t *>(row)[x] = (uint16_t)v;
    else row[x] = (uint8_t)v;
  }
}

// ---- the two drivers: a source `src`, LDS laid out by `o` (tile_geom for PlaneSrc, joint_geom for JointSrc) ------------
// the frame's own offsets (rules 1 - 3, 8 - 10) of one tile for thread `tid` of a workgroup whose barrier is `sync`: the
// sample arrays and T staged, the sums of rule 4 / 11 in aw and au.  gain: rule 24's table, staged beside T (JointSrc only).
template <int S, int BPS, class Src, class Layout, class Sync, class Gn = NoGain>
G1S_DN_HD void dn_spatial(int tid, const TileGeom &g, const Layout &o, uint8_t *lds, const uint16_t *table, int q, const Src &src, int x0, int y0,
                          Sync sync, uint32_t *aw, uint32_t *const (&au)[Src::NP], Gn gain = Gn()) {
  const int LP = dn_lp(o);
  uint32_t *Hb = reinterpret_cast<uint32_t *>(lds + o.offH);
  uint16_t *L = reinterpret_cast<uint16_t *>(lds + o.offL), *Wb = reinterpret_cast<uint16_t *>(lds + o.offW),
           *T = reinterpret_cast<uint16_t *>(lds + o.offT);
  src.template stage<BPS>(tid, g, LP, L, x0, y0);
  if constexpr (Gn::on) {
    static_assert(Src::NA == 3, "a gain reads the guide");
    uint16_t *Mt = reinterpret_cast<uint16_t *>(lds + o.offM);
    for (int i = tid; i < kTable / 2; i += kThreads) {  // (T's loop: the first kGain / 2 turns take a word of the gain along)
      reinterpret_cast<uint32_t *>(T)[i] = reinterpret_cast<const uint32_t *>(table)[i];
      if (i < kGain / 2) reinterpret_cast<uint32_t *>(Mt)[i] = reinterpret_cast<const uint32_t *>(gain.table)[i];
    }
  } else {
    for (int i = tid; i < kTable / 2; i += kThreads) reinterpret_cast<uint32_t *>(T)[i] = reinterpret_cast<const uint32_t *>(table)[i];
  }
  sync();
  dn_init<Src::NP>(tid, g, LP, L, aw, au);
  for (int dy = 0; dy <= g.A; ++dy) {
    const int NR = kTH + dy + 2 * S, RH = kTH + dy;
    const uint32_t mNR = magic(NR);
    for (int dx = dy ? -g.A : 1; dx <= g.A; ++dx) {
      const int RW = kTW + (dx < 0 ? -dx : dx);
      dn_hsum<S, Src::NA>(tid, g, LP, L, Hb, dx, dy, RW, NR, mNR);
      sync();
      if constexpr (Gn::on)
        dn_weights<S>(tid, g, Hb, Wb, T, q, dx, dy, RW, RH, magic(RW), x0, y0, src.grid_w(), src.grid_h(),
                      GainLds{reinterpret_cast<const uint16_t *>(lds + o.offM), L + 2 * LP, L + 2 * LP, gain.shift});
      else
        dn_weights<S>(tid, g, Hb, Wb, T, q, dx, dy, RW, RH, magic(RW), x0, y0, src.grid_w(), src.grid_h());
      sync();
      dn_accumulate<Src::NP>(tid, g, LP, L, Wb, dx, dy, aw, au);
    }
  }
}

// after dn_spatial, the 2 D frames around the frame in hand (rules 5 - 7, 11t): nb(k) is the source of the k-th, absent
// where the clip has no such frame -- the same for every thread of the workgroup.  The order of the neighbours does not
// show in the result: the sums are exact.  mv(k) is the tile's motion vector towards the k-th (rule 19), the same for every
// thread of the workgroup: the neighbour's tile is staged from the moved origin and one bounds test moves with it.
struct MotionVec {
  int x, y;
};
struct NoMotion {
  G1S_DN_HD MotionVec operator()(int) const { return MotionVec{0, 0}; }
};

template <int S, int BPS, int NP, class Layout, class Nb, class Sync, class Mv = NoMotion, class Gn = NoGain>
G1S_DN_HD void dn_temporal(int tid, const TileGeom &g, const Layout &o, uint8_t *lds, int q, Nb nb, int nnb, int x0, int y0, Sync sync, uint32_t *aw,
                           uint64_t *const (&au)[NP], Mv mv = Mv(), Gn gain = Gn()) {
  const int LP = dn_lp(o);
  uint32_t *Hb = reinterpret_cast<uint32_t *>(lds + o.offH);
  uint16_t *L = reinterpret_cast<uint16_t *>(lds + o.offL), *Wb = reinterpret_cast<uint16_t *>(lds + o.offW),
           *T = reinterpret_cast<uint16_t *>(lds + o.offT), *N = reinterpret_cast<uint16_t *>(lds + o.offN);
  for (int k = 0; k < nnb; ++k) {
    const auto n = nb(k);
    static_assert(decltype(n)::NP == NP, "a neighbour has the frame's planes");
    if (!n.present()) continue;
    sync();  // the last dn_accumulate_t has read N
    const MotionVec m = mv(k);
    n.template stage<BPS>(tid, g, LP, N, x0 + m.x, y0 + m.y);
    sync();
    for (int dy = -g.A; dy <= g.A; ++dy)
      for (int dx = -g.A; dx <= g.A; ++dx) {
        dn_hsum_t<S, decltype(n)::NA>(tid, g, LP, L, N, Hb, dx, dy);
        sync();
        if constexpr (Gn::on)  // (Mt: staged by dn_spatial)
          dn_weights_t<S>(tid, g, Hb, Wb, T, q, dx, dy, x0, y0, n.grid_w(), n.grid_h(), m.x, m.y,
                          GainLds{reinterpret_cast<const uint16_t *>(lds + o.offM), L + 2 * LP, N + 2 * LP, gain.shift});
        else
          dn_weights_t<S>(tid, g, Hb, Wb, T, q, dx, dy, x0, y0, n.grid_w(), n.grid_h(), m.x, m.y);
        sync();
        dn_accumulate_t<NP>(tid, g, LP, N, Wb, dx, dy, aw, au);
      }
  }
}

// the four tile functions, start to end (what kd_nlm and kd_nlm_j call in their forms kPlain and kTemporal); this one: one plane on its own
template <int S, int BPS, class Sync>
G1S_DN_HD void dn_tile(int tid, const TileGeom &g, uint8_t *lds, const uint16_t *table, int q, const uint8_t *in, uint32_t in_stride, uint8_t *out,
                       uint32_t out_stride, int W, int H, int x0, int y0, Sync sync) {
  uint32_t aw[kSPT], au[kSPT];
  dn_spatial<S, BPS>(tid, g, g, lds, table, q, PlaneSrc{in, in_stride, W, H}, x0, y0, sync, aw, {au});
  dn_store<BPS>(tid, out, out_stride, W, H, x0, y0, aw, au);
}

// the temporal filter: `nb` / `nb_stride` are the same plane of the 2 D frames around the frame in hand, a null pointer
// where the clip has no such frame (rule 5)
template <int S, int BPS, class Sync>
G1S_DN_HD void dn_tile_t(int tid, const TileGeom &g, uint8_t *lds, const uint16_t *table, int q, const uint8_t *in, uint32_t in_stride,
                         const uint8_t *const *nb, const uint32_t *nb_stride, int nnb, uint8_t *out, uint32_t out_stride, int W, int H, int x0, int y0,
                         Sync sync) {
  uint32_t aw[kSPT], au32[kSPT];
  dn_spatial<S, BPS>(tid, g, g, lds, table, q, PlaneSrc{in, in_stride, W, H}, x0, y0, sync, aw, {au32});  // (fits 32 bits, as in dn_tile)
  uint64_t au[kSPT];
#pragma unroll
  for (int j = 0; j < kSPT; ++j) au[j] = au32[j];
  dn_temporal<S, BPS>(tid, g, g, lds, q, [=](int k) { return PlaneSrc{nb[k], nb_stride[k], W, H}; }, nnb, x0, y0, sync, aw, {au});
  dn_store<BPS>(tid, out, out_stride, W, H, x0, y0, aw, au);
}

// one chroma tile of the joint filter
template <int S, int BPS, class Sync, class Gn = NoGain, class JG = JointGeom>
G1S_DN_HD void dn_tile_j(int tid, const TileGeom &g, const JG &jg, uint8_t *lds, const uint16_t *table, int q, const JointPlanes &p,
                         const JointShape &s, uint8_t *out_cb, uint32_t out_cb_stride, uint8_t *out_cr, uint32_t out_cr_stride, int x0, int y0,
                         Sync sync, Gn gain = Gn()) {
  uint32_t aw[kSPT], aub[kSPT], aur[kSPT];
  dn_spatial<S, BPS>(tid, g, jg, lds, table, q, JointSrc{p, s}, x0, y0, sync, aw, {aub, aur}, gain);
  dn_store<BPS>(tid, out_cb, out_cb_stride, s.cw, s.ch, x0, y0, aw, aub);
  dn_store<BPS>(tid, out_cr, out_cr_stride, s.cw, s.ch, x0, y0, aw, aur);
}

// one chroma tile of the temporal joint filter (rule 11t): nb(k) gives the planes of the k-th of the 2 D frames around the
// frame in hand, .luma a null pointer where the clip has no such frame -- the same for every thread of the workgroup
template <int S, int BPS, class Nb, class Sync, class Gn = NoGain, class JG = JointGeom>
G1S_DN_HD void dn_tile_jt(int tid, const TileGeom &g, const JG &jg, uint8_t *lds, const uint16_t *table, int q, const JointPlanes &p,
                          Nb nb, int nnb, const JointShape &s, uint8_t *out_cb, uint32_t out_cb_stride, uint8_t *out_cr,
                          uint32_t out_cr_stride, int x0, int y0, Sync sync, Gn gain = Gn()) {
  uint32_t aw[kSPT], aub32[kSPT], aur32[kSPT];
  dn_spatial<S, BPS>(tid, g, jg, lds, table, q, JointSrc{p, s}, x0, y0, sync, aw, {aub32, aur32}, gain);
  uint64_t aub[kSPT], aur[kSPT];
#pragma unroll
  for (int j = 0; j < kSPT; ++j) aub[j] = aub32[j], aur[j] = aur32[j];
  dn_temporal<S, BPS>(tid, g, jg, lds, q, [&](int k) { return JointSrc{nb(k), s}; }, nnb, x0, y0, sync, aw, {aub, aur}, NoMotion(), gain);
  dn_store<BPS>(tid, out_cb, out_cb_stride, s.cw, s.ch, x0, y0, aw, aub);
  dn_store<BPS>(tid, out_cr, out_cr_stride, s.cw, s.ch, x0, y0, aw, aur);
}

// ---- motion (rules 16 - 20): one vector per tile and neighbour frame ------------------------------------------------------
// The filter's tiles are the motion blocks.  kd_motion finds a block's vector towards one neighbour on the search plane (the
// rounded 2 x 2 box mean, rule 16: dn_stage_guide at xdec = ydec = 1), where a block is kMBW x kMBH samples.  In LDS
//
//   C   the block of u'_t, kMBW x kMBH u16 (what lies outside the search plane is staged clamped and never summed),
//   Wd  the (kMBW + 2M) x (kMBH + 2M) window of u'_{t+k} around it, the search plane's edges replicated,
//   K   a 64-bit key a thread, P one a group of 16 threads,
//
// C and Wd once per plane that takes part (NA = 2: Cb and Cr of a joint chroma tile, whose SADs add, rule 20).  The (2M + 1)^2
// candidates are dealt to the threads by `tid`; a thread keeps a row of C in registers and walks its candidates' rows of Wd.
// The minimum of rule 18's key is exact, so the order of the reduction cannot show.
constexpr int kMBW = kTW / 2, kMBH = kTH / 2;
constexpr int kMaxM = 32;  // on the search plane; the motion range is 2 M
constexpr int kMaxCand = ((2 * kMaxM + 1) * (2 * kMaxM + 1) + kThreads - 1) / kThreads;  // candidates a thread
constexpr int kKeyGroup = 16;

struct MotionGeom {
  int M, WW, WH, WS;  // the window: WH rows of WW samples, row stride WS (u16)
  int LPc, LPw;       // samples from one plane's C / Wd to the next
  int offC, offW, offK, offP, bytes;
};

G1S_DN_HD MotionGeom motion_geom(int M, int NA) {
  MotionGeom m;
  m.M = M, m.WW = kMBW + 2 * M, m.WH = kMBH + 2 * M;
  m.WS = m.WW | 1;
  m.LPc = kMBW * kMBH, m.LPw = (m.WS * m.WH + 7) & ~7;
  m.offC = 0;
  m.offW = m.offC + NA * m.LPc * 2;
  m.offK = (m.offW + NA * m.LPw * 2 + 15) & ~15;
  m.offP = m.offK + kThreads * 8;
  m.bytes = m.offP + kKeyGroup * 8;
  return m;
}

// what a motion block is searched on: the NA planes (W x H each) of frame t and of frame t + k
struct MotionPlanes {
  const uint8_t *p[2];
  uint32_t stride[2];
};

// rule 16 into `dst`: rows x cols samples of the search plane of a W x H plane from (x0, y0), coordinates clamped to it
template <int BPS>
G1S_DN_HD void dn_stage_half(int tid, uint16_t *dst, int rows, int cols, int stride, const uint8_t *in, uint32_t in_stride, int W, int H, int x0,
                             int y0) {
  TileGeom g{};
  g.R = 0, g.LH = rows, g.LW = cols, g.LS = stride;
  dn_stage_guide<BPS>(tid, g, dst, in, in_stride, W, H, 1, 1, (W + 1) >> 1, (H + 1) >> 1, x0, y0);
}

// SAD of rule 17 for the thread's candidates over the block's bw x bh samples; RAGGED: bw < kMBW.  sad[j] is candidate
// tid + j kThreads, whose window starts at base[j]; nj candidates a thread are looked at.
template <int NA, bool RAGGED>
G1S_DN_HD void dn_motion_sad(const MotionGeom &m, const uint16_t *C, const uint16_t *Wd, int bw, int bh, int nj, const int *base, uint32_t *sad) {
  for (int a = 0; a < NA; ++a)
    for (int r = 0; r < bh; ++r) {
      int c[kMBW];
#pragma unroll
      for (int x = 0; x < kMBW; ++x) c[x] = (int)C[a * m.LPc + r * kMBW + x];
#pragma unroll
      for (int j = 0; j < kMaxCand; ++j)
        if (j < nj) {  // (the same for the whole workgroup)
          const uint16_t *w = Wd + a * m.LPw + base[j] + r * m.WS;
          uint32_t s = 0;
#pragma unroll
          for (int x = 0; x < kMBW; ++x) {
            const int d = c[x] - (int)w[x];
            const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
            s += !RAGGED || x < bw ? ad : 0u;
          }
          sad[j] += s;
        }
    }
}

// rule 18's key of a candidate (cx, cy) = m' + (M, M)
G1S_DN_HD uint64_t dn_motion_key(uint32_t sad, int cx, int cy, int M) {
  const int ax = cx < M ? M - cx : cx - M, ay = cy < M ? M - cy : cy - M;
  return ((uint64_t)sad << 21) | ((uint64_t)(ax + ay) << 14) | ((uint64_t)cy << 7) | (uint64_t)cx;
}

// the vector of the block at (bx, by) (in blocks) of frame t towards frame t + k, for thread `tid` of a workgroup whose
// barrier is `sync`: mv[0], mv[1] = (mx, my) in full-resolution samples
template <int BPS, int NA, class Sync>
G1S_DN_HD void dn_motion_tile(int tid, const MotionGeom &m, uint8_t *lds, const MotionPlanes &cur, const MotionPlanes &ref, int W, int H, int bx,
                              int by, Sync sync, int8_t *mv) {
  uint16_t *C = reinterpret_cast<uint16_t *>(lds + m.offC), *Wd = reinterpret_cast<uint16_t *>(lds + m.offW);
  uint64_t *K = reinterpret_cast<uint64_t *>(lds + m.offK), *P = reinterpret_cast<uint64_t *>(lds + m.offP);
  const int x0 = bx * kMBW, y0 = by * kMBH;
  const int bw = imin(kMBW, ((W + 1) >> 1) - x0), bh = imin(kMBH, ((H + 1) >> 1) - y0);
  for (int a = 0; a < NA; ++a) {
    dn_stage_half<BPS>(tid, C + a * m.LPc, kMBH, kMBW, kMBW, cur.p[a], cur.stride[a], W, H, x0, y0);
    dn_stage_half<BPS>(tid, Wd + a * m.LPw, m.WH, m.WW, m.WS, ref.p[a], ref.stride[a], W, H, x0 - m.M, y0 - m.M);
  }
  sync();
  const int n1 = 2 * m.M + 1, ncand = n1 * n1, nj = (ncand + kThreads - 1) / kThreads;
  uint32_t sad[kMaxCand];
  int base[kMaxCand];
#pragma unroll
  for (int j = 0; j < kMaxCand; ++j) {
    const int i = tid + j * kThreads, ii = i < ncand ? i : 0, cy = ii / n1;  // (a thread without a j-th candidate walks the first)
    base[j] = cy * m.WS + (ii - cy * n1), sad[j] = 0;
  }
  if (bw < kMBW) dn_motion_sad<NA, true>(m, C, Wd, bw, bh, nj, base, sad);
  else dn_motion_sad<NA, false>(m, C, Wd, bw, bh, nj, base, sad);
  uint64_t best = ~(uint64_t)0;
#pragma unroll
  for (int j = 0; j < kMaxCand; ++j) {
    const int i = tid + j * kThreads;
    if (i < ncand) {
      const int cy = i / n1;
      const uint64_t key = dn_motion_key(sad[j], i - cy * n1, cy, m.M);
      best = key < best ? key : best;
    }
  }
  K[tid] = best;
  sync();
  if (tid < kKeyGroup) {
    uint64_t b = K[tid * (kThreads / kKeyGroup)];
    for (int i = 1; i < kThreads / kKeyGroup; ++i) {
      const uint64_t k = K[tid * (kThreads / kKeyGroup) + i];
      b = k < b ? k : b;
    }
    P[tid] = b;
  }
  sync();
  if (tid == 0) {
    uint64_t b = P[0];
    for (int i = 1; i < kKeyGroup; ++i) b = P[i] < b ? P[i] : b;
    mv[0] = (int8_t)(2 * ((int)(b & 127) - m.M)), mv[1] = (int8_t)(2 * ((int)((b >> 7) & 127) - m.M));
  }
}

// the temporal tile functions under motion (what kd_nlm<kMotion> and kd_nlm_j<kMotion> call): `mv` is the tile's vectors, a pair of
// int8 for each of the nnb neighbours, `mv_stride` bytes from one neighbour's to the next
struct TileVectors {
  const int8_t *mv;
  int stride;
  G1S_DN_HD MotionVec operator()(int k) const { return MotionVec{(int)mv[k * stride], (int)mv[k * stride + 1]}; }
};

template <int S, int BPS, class Sync>
G1S_DN_HD void dn_tile_tm(int tid, const TileGeom &g, uint8_t *lds, const uint16_t *table, int q, const uint8_t *in, uint32_t in_stride,
                          const uint8_t *const *nb, const uint32_t *nb_stride, int nnb, const int8_t *mv, int mv_stride, uint8_t *out,
                          uint32_t out_stride, int W, int H, int x0, int y0, Sync sync) {
  uint32_t aw[kSPT], au32[kSPT];
  dn_spatial<S, BPS>(tid, g, g, lds, table, q, PlaneSrc{in, in_stride, W, H}, x0, y0, sync, aw, {au32});
  uint64_t au[kSPT];
#pragma unroll
  for (int j = 0; j < kSPT; ++j) au[j] = au32[j];
  dn_temporal<S, BPS>(tid, g, g, lds, q, [=](int k) { return PlaneSrc{nb[k], nb_stride[k], W, H}; }, nnb, x0, y0, sync, aw, {au},
                      TileVectors{mv, mv_stride});
  dn_store<BPS>(tid, out, out_stride, W, H, x0, y0, aw, au);
}

template <int S, int BPS, class Nb, class Sync, class Gn = NoGain, class JG = JointGeom>
G1S_DN_HD void dn_tile_jtm(int tid, const TileGeom &g, const JG &jg, uint8_t *lds, const uint16_t *table, int q, const JointPlanes &p,
                           Nb nb, int nnb, const int8_t *mv, int mv_stride, const JointShape &s, uint8_t *out_cb, uint32_t out_cb_stride,
                           uint8_t *out_cr, uint32_t out_cr_stride, int x0, int y0, Sync sync, Gn gain = Gn()) {
  uint32_t aw[kSPT], aub32[kSPT], aur32[kSPT];
  dn_spatial<S, BPS>(tid, g, jg, lds, table, q, JointSrc{p, s}, x0, y0, sync, aw, {aub32, aur32}, gain);
  uint64_t aub[kSPT], aur[kSPT];
#pragma unroll
  for (int j = 0; j < kSPT; ++j) aub[j] = aub32[j], aur[j] = aur32[j];
  dn_temporal<S, BPS>(tid, g, jg, lds, q, [&](int k) { return JointSrc{nb(k), s}; }, nnb, x0, y0, sync, aw, {aub, aur}, TileVectors{mv, mv_stride}, gain);
  dn_store<BPS>(tid, out_cb, out_cb_stride, s.cw, s.ch, x0, y0, aw, aub);
  dn_store<BPS>(tid, out_cr, out_cr_stride, s.cw, s.ch, x0, y0, aw, aur);
}

}  // namespace g1s_dn
