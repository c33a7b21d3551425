// grain.hip -- `render`: the film grain synthesis process of the AV1 specification (clause 7.18.3) on the device.
//
// Written from the standard: random number process (7.18.3.2), generate grain process (7.18.3.3), scaling lookup
// initialisation (7.18.3.4), add noise synthesis process (7.18.3.5).  Everything is integer and exact; the only table is
// the standard's Gaussian_Sequence (av1_gaussian_sequence.h).  Two kernels per batch of frames:
//
//   kg_template  one workgroup per frame: the frame's grain templates (the LFSR draws split over the lanes by a
//                precomputed jump, the AR filter as a skewed wavefront with one lane per row), the frame's block offsets
//                (one byte per 32 x 32 luma block) -- and one workgroup per distinct segment for its three scaling tables.
//   kg_apply     one workgroup per (frame, 32-row luma stripe): templates, tables and two rows of block offsets in LDS,
//                every sample of the stripe's luma and chroma rows read once and written once, 8 samples a lane and turn.
//
// kg_apply reads `in` and writes `out`, which must not overlap: chroma is scaled by the co-located input luma.
// The file command (`render`) stands above the per-frame calls in grain_file.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "av1_gaussian_sequence.h"
#include "frame_op.h"

namespace {

const int16_t kGaussHost[2048] = {G1S_GAUSSIAN_SEQUENCE_VALUES};
__device__ const int16_t kGaussDev[2048] = {G1S_GAUSSIAN_SEQUENCE_VALUES};

constexpr int kThreads = 256;
constexpr int kLumaW = 82, kLumaH = 73;
constexpr int kTplSlot = 5992;      // int16 entries per template in the per-frame buffer (73 * 82 = 5986, rounded up to 16 bytes)
constexpr int kDrawsPerLane = 24;   // 256 lanes x 24 draws >= 5986
constexpr int kMaxBlocksX = 512;    // 32-column blocks across a frame: widths up to 16384
constexpr uint32_t kNoSegment = 0xffffffffu;

// one distinct parameter set of a batch (everything of g1s_segment_t but its times and its seed)
struct GrainSeg {
  int8_t cy[24], ccb[25], ccr[25];
  uint8_t py[14][2], pcb[10][2], pcr[10][2];
  uint8_t lag, ar_shift, grain_scale_shift, scaling_shift;
  uint8_t num_y, num_cb, num_cr, csfl, overlap;
  int16_t cb_mult, cb_luma_mult, cb_offset, cr_mult, cr_luma_mult, cr_offset;  // 128 / 128 / 256 already subtracted
};

struct GrainJob {
  const uint8_t *in[3];
  uint8_t *out[3];
  uint32_t in_stride[3], out_stride[3];  // bytes
  uint32_t seg;                          // index into the batch's GrainSeg list, kNoSegment: copy the frame
  uint32_t seed;
};

struct GrainGeom {
  int W, H, subx, suby, nplanes, bit_depth;
  int nbx, nstripes;  // 32 x 32 luma blocks across, 32-row luma stripes down (0 stripes: templates only)
  int cw, ch;         // chroma template size
};

struct TemplateParams {
  const GrainJob *jobs;
  const GrainSeg *segs;
  const uint16_t *jump;  // [kThreads][16]: column b of the LFSR's transition matrix to the power 24 * lane
  int16_t *tpl;          // [frames][3][kTplSlot]
  uint8_t *offs;         // [frames][nstripes * nbx]
  uint8_t *luts;         // [segs][3][256]
  int nframes, nsegs;
  GrainGeom g;
};

struct ApplyParams {
  const GrainJob *jobs;
  const GrainSeg *segs;
  const int16_t *tpl;
  const uint8_t *offs;
  const uint8_t *luts;
  GrainGeom g;
  int min_value, max_luma, max_chroma;
};

__host__ __device__ inline uint32_t lfsr_step(uint32_t r) {
  const uint32_t bit = ((r >> 0) ^ (r >> 1) ^ (r >> 3) ^ (r >> 12)) & 1u;
  return (r >> 1) | (bit << 15);
}

__device__ __forceinline__ int round2(int x, int n) { return n ? (x + (1 << (n - 1))) >> n : x; }
__device__ __forceinline__ int clip3(int lo, int hi, int x) { return min(hi, max(lo, x)); }

// ---------------------------------------------------------------------------------------------------------------
// kg_template
// ---------------------------------------------------------------------------------------------------------------
// The draws of a template: lane l owns draws [24 l, 24 l + 24).  The LFSR is linear over GF(2), so the register after
// 24 l steps is the XOR of the jump matrix's columns selected by the bits of the seed.
__device__ void tpl_draw(int16_t *dst, int n, uint32_t seed, bool active, int shift, const uint16_t *jump, int tid) {
  const int first = tid * kDrawsPerLane;
  if (first >= n) return;
  uint32_t r = 0;
  for (int b = 0; b < 16; ++b)
    if ((seed >> b) & 1u) r ^= jump[tid * 16 + b];
  for (int k = 0; k < kDrawsPerLane && first + k < n; ++k) {
    r = lfsr_step(r);
    const int g = active ? (int)kGaussDev[(r >> 5) & 2047u] : 0;
    dst[first + k] = (int16_t)round2(g, shift);
  }
}

// The scaling table of one plane at x: flat before the first and from the last point on, the standard's fixed-point line between.
__device__ int lut_entry(const uint8_t (*pts)[2], int n, int x) {
  if (n == 0) return 0;
  if (x < pts[0][0]) return pts[0][1];
  if (x >= pts[n - 1][0]) return pts[n - 1][1];
  int i = 0;
  while (i + 2 < n && x >= pts[i + 1][0]) ++i;
  const int dy = (int)pts[i + 1][1] - (int)pts[i][1], dx = (int)pts[i + 1][0] - (int)pts[i][0];
  const int delta = dy * ((65536 + (dx >> 1)) / dx);  // (dx > 0: checked on the host)
  return (int)pts[i][1] + (((x - (int)pts[i][0]) * delta + 32768) >> 16);
}

__global__ __launch_bounds__(kThreads) void kg_template(TemplateParams p) {
  __shared__ int16_t sL[kLumaW * kLumaH], sC[2][kLumaW * kLumaH];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= p.nframes) {  // the scaling tables of one distinct segment
    const int si = (int)blockIdx.x - p.nframes;
    const GrainSeg &sg = p.segs[si];
    uint8_t *lut = p.luts + (size_t)si * 768;
    lut[tid] = (uint8_t)lut_entry(sg.py, sg.num_y, tid);
    lut[256 + tid] = (uint8_t)(sg.csfl ? lut_entry(sg.py, sg.num_y, tid) : lut_entry(sg.pcb, sg.num_cb, tid));
    lut[512 + tid] = (uint8_t)(sg.csfl ? lut_entry(sg.py, sg.num_y, tid) : lut_entry(sg.pcr, sg.num_cr, tid));
    return;
  }
  const int frame = blockIdx.x;
  const GrainJob &job = p.jobs[frame];
  if (job.seg == kNoSegment) return;  // (uniform: the whole workgroup)
  const GrainSeg &sg = p.segs[job.seg];
  const GrainGeom &g = p.g;
  const int lag = sg.lag, ar_shift = sg.ar_shift;
  const int gc = 128 << (g.bit_depth - 8), gmin = -gc, gmax = (256 << (g.bit_depth - 8)) - 1 - gc;
  const int draw_shift = 12 - g.bit_depth + sg.grain_scale_shift;
  const uint32_t seed = job.seed & 0xffffu;
  const bool chroma = g.nplanes > 1;
  const int cw = g.cw, ch = g.ch;

  tpl_draw(sL, kLumaW * kLumaH, seed, sg.num_y > 0, draw_shift, p.jump, tid);
  if (chroma) {
    tpl_draw(sC[0], cw * ch, seed ^ 0xb524u, sg.num_cb > 0 || sg.csfl, draw_shift, p.jump, tid);
    tpl_draw(sC[1], cw * ch, seed ^ 0x49d8u, sg.num_cr > 0 || sg.csfl, draw_shift, p.jump, tid);
  }
  __syncthreads();

  // Luma AR filter, raster order in the standard.  (y, x) needs its own row up to x - 1 and the rows above up to x + lag:
  // row y may trail row y - 1 by lag + 1 columns.  Lane r owns row 3 + r and is at column 3 + t - r (lag + 1) in step t.
  if (lag > 0 && sg.num_y > 0) {
    const int rows = kLumaH - 3, cols = kLumaW - 6, skew = lag + 1;
    const int steps = cols + (rows - 1) * skew;
    for (int t = 0; t < steps; ++t) {
      const int xx = t - tid * skew;
      if (tid < rows && xx >= 0 && xx < cols) {
        const int y = 3 + tid, x = 3 + xx;
        int s = 0, pos = 0;
        for (int dr = -lag; dr <= 0; ++dr)
          for (int dc = -lag; dc <= lag; ++dc) {
            if (dr == 0 && dc == 0) break;
            s += (int)sL[(y + dr) * kLumaW + x + dc] * (int)sg.cy[pos++];
          }
        sL[y * kLumaW + x] = (int16_t)clip3(gmin, gmax, (int)sL[y * kLumaW + x] + round2(s, ar_shift));
      }
      __syncthreads();
    }
  }
  // Chroma AR filters: Cb on lanes 0 .. 127, Cr on lanes 128 .. 255, the same wavefront; the last tap takes the
  // co-located luma grain averaged over the subsampled footprint, so this waits for the luma template above.
  if (chroma) {
    const int pl = tid >> 7, r = tid & 127;
    const int rows = ch - 3, cols = cw - 6, skew = lag + 1;
    const int steps = cols + (rows - 1) * skew;
    int16_t *sP = sC[pl];
    const int8_t *coef = pl ? sg.ccr : sg.ccb;
    for (int t = 0; t < steps; ++t) {
      const int xx = t - r * skew;
      if (r < rows && xx >= 0 && xx < cols) {
        const int y = 3 + r, x = 3 + xx;
        int s = 0, pos = 0;
        for (int dr = -lag; dr <= 0; ++dr)
          for (int dc = -lag; dc <= lag; ++dc) {
            if (dr == 0 && dc == 0) break;
            s += (int)sP[(y + dr) * cw + x + dc] * (int)coef[pos++];
          }
        if (sg.num_y > 0) {
          const int lx = ((x - 3) << g.subx) + 3, ly = ((y - 3) << g.suby) + 3;
          int lu = 0;
          for (int i = 0; i <= g.suby; ++i)
            for (int j = 0; j <= g.subx; ++j) lu += (int)sL[(ly + i) * kLumaW + lx + j];
          s += round2(lu, g.subx + g.suby) * (int)coef[pos];
        }
        sP[y * cw + x] = (int16_t)clip3(gmin, gmax, (int)sP[y * cw + x] + round2(s, ar_shift));
      }
      __syncthreads();
    }
  }
  __syncthreads();
  int16_t *out = p.tpl + (size_t)frame * 3 * kTplSlot;
  for (int i = tid; i < kLumaW * kLumaH; i += kThreads) out[i] = sL[i];
  if (chroma)
    for (int i = tid; i < cw * ch; i += kThreads) {
      out[kTplSlot + i] = sC[0][i];
      out[2 * kTplSlot + i] = sC[1][i];
    }
  // Block offsets: the register is re-seeded per 32-row luma stripe, then one 8-bit draw per 32-column block.
  uint8_t *offs = p.offs + (size_t)frame * g.nstripes * g.nbx;
  for (int s = tid; s < g.nstripes; s += kThreads) {
    uint32_t r = seed;
    r ^= (uint32_t)((s * 37 + 178) & 255) << 8;
    r ^= (uint32_t)((s * 173 + 105) & 255);
    for (int b = 0; b < g.nbx; ++b) {
      r = lfsr_step(r);
      offs[s * g.nbx + b] = (uint8_t)(r >> 8);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// kg_apply
// ---------------------------------------------------------------------------------------------------------------
template <int BPS>
__device__ __forceinline__ void load8(const uint8_t *a, int (&v)[8]) {
  if (BPS == 2) {
    const uint4 w = *reinterpret_cast<const uint4 *>(a);
    v[0] = w.x & 0xffff, v[1] = w.x >> 16, v[2] = w.y & 0xffff, v[3] = w.y >> 16;
    v[4] = w.z & 0xffff, v[5] = w.z >> 16, v[6] = w.w & 0xffff, v[7] = w.w >> 16;
  } else {
    const uint2 w = *reinterpret_cast<const uint2 *>(a);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (w.x >> (8 * k)) & 0xff, v[4 + k] = (w.y >> (8 * k)) & 0xff;
  }
}
template <int BPS>
__device__ __forceinline__ void store8(uint8_t *a, const int (&v)[8]) {
  if (BPS == 2) {
    uint4 w;
    w.x = (uint32_t)v[0] | ((uint32_t)v[1] << 16), w.y = (uint32_t)v[2] | ((uint32_t)v[3] << 16);
    w.z = (uint32_t)v[4] | ((uint32_t)v[5] << 16), w.w = (uint32_t)v[6] | ((uint32_t)v[7] << 16);
    *reinterpret_cast<uint4 *>(a) = w;
  } else {
    uint2 w;
    w.x = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    w.y = (uint32_t)v[4] | ((uint32_t)v[5] << 8) | ((uint32_t)v[6] << 16) | ((uint32_t)v[7] << 24);
    *reinterpret_cast<uint2 *>(a) = w;
  }
}
template <int BPS>
__device__ __forceinline__ int load1(const uint8_t *row, int x) {
  return BPS == 2 ? (int)reinterpret_cast<const uint16_t *>(row)[x] : (int)row[x];
}
template <int BPS>
__device__ __forceinline__ void store1(uint8_t *row, int x, int v) {
  if (BPS == 2) reinterpret_cast<uint16_t *>(row)[x] = (uint16_t)v;
  else row[x] = (uint8_t)v;
}

// The noise stripe of one plane at row i (0 .. 33, or 0 .. 16 in a subsampled direction) and columns j0 .. j0 + 7 of block b:
// the block's window of the template and, under overlap_flag, the blend of its first columns with the columns the block to
// its left leaves beyond its 32 (27/17, 17/27; 23/22 for a subsampled plane).  j0 + 7 stays inside the block.
__device__ __forceinline__ void stripe_grain8(const int16_t *T, int tw, const uint8_t *off, int b, int i, int j0, int psx, int psy,
                                              bool overlap, int gmin, int gmax, int (&g)[8]) {
  const int r = off[b];
  const int ox = psx ? 6 + (r >> 4) : 9 + 2 * (r >> 4), oy = psy ? 6 + (r & 15) : 9 + 2 * (r & 15);
  const int16_t *row = T + (oy + i) * tw + ox + j0;
#pragma unroll
  for (int k = 0; k < 8; ++k) g[k] = row[k];
  if (overlap && b > 0 && j0 == 0) {
    const int r2 = off[b - 1];
    const int ox2 = psx ? 6 + (r2 >> 4) : 9 + 2 * (r2 >> 4), oy2 = psy ? 6 + (r2 & 15) : 9 + 2 * (r2 & 15);
    const int16_t *old = T + (oy2 + i) * tw + ox2 + (32 >> psx);
    if (psx) {
      g[0] = clip3(gmin, gmax, round2(old[0] * 23 + g[0] * 22, 5));
    } else {
      g[0] = clip3(gmin, gmax, round2(old[0] * 27 + g[0] * 17, 5));
      g[1] = clip3(gmin, gmax, round2(old[1] * 17 + g[1] * 27, 5));
    }
  }
}

// One plane's rows of the stripe.  `active`: the plane takes noise (otherwise its samples are copied).
template <int BPS>
__device__ void apply_plane(const ApplyParams &p, const GrainJob &job, const GrainSeg *sg, int pl, int stripe, const int16_t *T,
                            int tw, const uint16_t *lut, const uint8_t *off_prev, const uint8_t *off_cur, bool active) {
  const GrainGeom &g = p.g;
  const int psx = pl ? g.subx : 0, psy = pl ? g.suby : 0;
  const int pw = (g.W + psx) >> psx, ph = (g.H + psy) >> psy;
  const int row0 = stripe << (5 - psy), nrows = min(32 >> psy, ph - row0), nch = (pw + 7) >> 3;
  if (nrows <= 0) return;
  const uint8_t *in = job.in[pl];
  uint8_t *out = job.out[pl];
  const uint32_t is = job.in_stride[pl], os = job.out_stride[pl];
  // (uniform) whole words where every row of the plane starts on a word boundary
  const bool vec = ((((uintptr_t)in | (uintptr_t)out | is | os) & (8 * BPS - 1)) == 0);
  const bool vec_luma = pl && ((((uintptr_t)job.in[0] | job.in_stride[0]) & (psx ? 15 : 8 * BPS - 1)) == 0);
  const int sh = g.bit_depth - 8, top = (256 << sh) - 1;
  const int gc = 128 << sh, gmin = -gc, gmax = top - gc;
  int shift = 8, mult = 0, luma_mult = 0, offset = 0, maxv = p.max_luma;
  bool overlap = false, csfl = false;
  if (active) {
    shift = sg->scaling_shift, overlap = sg->overlap != 0, csfl = sg->csfl != 0;
    if (pl) {
      maxv = p.max_chroma;
      mult = pl == 1 ? sg->cb_mult : sg->cr_mult;
      luma_mult = pl == 1 ? sg->cb_luma_mult : sg->cr_luma_mult;
      offset = (pl == 1 ? sg->cb_offset : sg->cr_offset) * (1 << sh);
    }
  }
  const int vrows = psy ? 1 : 2;  // rows of a stripe that blend with the stripe above
  for (int id = threadIdx.x; id < nrows * nch; id += kThreads) {
    const int i = id / nch, c = id - i * nch, x0 = c * 8, y = row0 + i;
    const int nvalid = min(8, pw - x0);
    const bool whole = vec && nvalid == 8;
    const uint8_t *irow = in + (size_t)y * is;
    uint8_t *orow = out + (size_t)y * os;
    int v[8];
    if (whole) {
      load8<BPS>(irow + (size_t)x0 * BPS, v);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = k < nvalid ? load1<BPS>(irow, x0 + k) : 0;
    }
    if (active) {
      // the noise image at (y, x0 ..): this stripe's row, blended with the rows the stripe above leaves below its 32
      const int b = x0 >> (5 - psx), j0 = x0 & ((32 >> psx) - 1);
      int gr[8];
      stripe_grain8(T, tw, off_cur, b, i, j0, psx, psy, overlap, gmin, gmax, gr);
      if (overlap && stripe > 0 && i < vrows) {
        int old[8];
        stripe_grain8(T, tw, off_prev, b, i + (32 >> psy), j0, psx, psy, overlap, gmin, gmax, old);
        const int wo = psy ? 23 : (i == 0 ? 27 : 17), wg = psy ? 22 : (i == 0 ? 17 : 27);
#pragma unroll
        for (int k = 0; k < 8; ++k) gr[k] = clip3(gmin, gmax, round2(old[k] * wo + gr[k] * wg, 5));
      }
      // the index into the scaling function: the sample itself (luma), or the standard's combination of the co-located
      // input luma -- averaged over the two columns of a horizontally subsampled sample -- and the chroma sample
      int idx[8];
      if (pl == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) idx[k] = v[k];
      } else {
        const uint8_t *lrow = job.in[0] + (size_t)(y << psy) * job.in_stride[0];
        int lu[8];
        if (psx) {
          if (vec_luma && 2 * x0 + 16 <= g.W) {
            int a[8], bq[8];
            load8<BPS>(lrow + (size_t)(2 * x0) * BPS, a);
            load8<BPS>(lrow + (size_t)(2 * x0 + 8) * BPS, bq);
#pragma unroll
            for (int k = 0; k < 4; ++k) lu[k] = (a[2 * k] + a[2 * k + 1] + 1) >> 1, lu[4 + k] = (bq[2 * k] + bq[2 * k + 1] + 1) >> 1;
          } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const int lx = min(2 * (x0 + k), g.W - 1), ln = min(lx + 1, g.W - 1);
              lu[k] = (load1<BPS>(lrow, lx) + load1<BPS>(lrow, ln) + 1) >> 1;
            }
          }
        } else {
          if (vec_luma && x0 + 8 <= g.W) {
            load8<BPS>(lrow + (size_t)x0 * BPS, lu);
          } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) lu[k] = load1<BPS>(lrow, min(x0 + k, g.W - 1));
          }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
          idx[k] = csfl ? lu[k] : clip3(0, top, ((lu[k] * luma_mult + v[k] * mult) >> 6) + offset);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        // scale_lut: the table at idx >> sh, interpolated towards the next entry by the low bits
        const int e = lut[min(idx[k] >> sh, 255)], start = e & 255, end = e >> 8;
        const int sc = start + round2((end - start) * (idx[k] & ((1 << sh) - 1)), sh);
        v[k] = clip3(p.min_value, maxv, v[k] + round2(sc * gr[k], shift));
      }
    }
    if (whole) {
      store8<BPS>(orow + (size_t)x0 * BPS, v);
    } else {
      for (int k = 0; k < nvalid; ++k) store1<BPS>(orow, x0 + k, v[k]);
    }
  }
}

template <int BPS>
__global__ __launch_bounds__(kThreads) void kg_apply(ApplyParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const GrainGeom &g = p.g;
  const int frame = blockIdx.y, stripe = blockIdx.x, tid = threadIdx.x;
  const GrainJob &job = p.jobs[frame];
  const bool has_seg = job.seg != kNoSegment;  // (uniform)
  const int ctpl = g.nplanes > 1 ? g.cw * g.ch : 0;
  // LDS: luma template | cb | cr (int16) | three tables of (entry, next entry) pairs | block offsets of the stripe above and of this one
  int16_t *sT = reinterpret_cast<int16_t *>(smem);
  uint16_t *sLut = reinterpret_cast<uint16_t *>(sT + ((kLumaW * kLumaH + 2 * ctpl + 7) & ~7));
  uint8_t *sOff = reinterpret_cast<uint8_t *>(sLut + 768);
  const GrainSeg *sg = has_seg ? &p.segs[job.seg] : nullptr;
  if (has_seg) {
    const int16_t *tpl = p.tpl + (size_t)frame * 3 * kTplSlot;
    for (int i = tid; i < kLumaW * kLumaH; i += kThreads) sT[i] = tpl[i];
    for (int i = tid; i < ctpl; i += kThreads) {
      sT[kLumaW * kLumaH + i] = tpl[kTplSlot + i];
      sT[kLumaW * kLumaH + ctpl + i] = tpl[2 * kTplSlot + i];
    }
    const uint8_t *lut = p.luts + (size_t)job.seg * 768;
    for (int i = tid; i < 768; i += kThreads) {
      const int x = i & 255;
      sLut[i] = (uint16_t)(lut[i] | (lut[(i - x) + min(x + 1, 255)] << 8));
    }
    const uint8_t *offs = p.offs + (size_t)frame * g.nstripes * g.nbx;
    for (int i = tid; i < g.nbx; i += kThreads) {
      sOff[i] = stripe > 0 ? offs[(stripe - 1) * g.nbx + i] : 0;
      sOff[kMaxBlocksX + i] = offs[stripe * g.nbx + i];
    }
  }
  __syncthreads();
  const bool csfl = has_seg && sg->csfl;
  apply_plane<BPS>(p, job, sg, 0, stripe, sT, kLumaW, sLut, sOff, sOff + kMaxBlocksX, has_seg && sg->num_y > 0);
  if (g.nplanes > 1) {
    apply_plane<BPS>(p, job, sg, 1, stripe, sT + kLumaW * kLumaH, g.cw, sLut + 256, sOff, sOff + kMaxBlocksX,
                     has_seg && (sg->num_cb > 0 || csfl));
    apply_plane<BPS>(p, job, sg, 2, stripe, sT + kLumaW * kLumaH + ctpl, g.cw, sLut + 512, sOff, sOff + kMaxBlocksX,
                     has_seg && (sg->num_cr > 0 || csfl));
  }
}

size_t apply_lds_bytes(const GrainGeom &g) {
  const int ctpl = g.nplanes > 1 ? g.cw * g.ch : 0;
  return (size_t)((kLumaW * kLumaH + 2 * ctpl + 7) & ~7) * 2 + 768 * 2 + 2 * kMaxBlocksX;
}

}  // namespace

using namespace g1s_op;

// =============================================================== host engine =====
// (the stream, the sticky error, the parameter sets' turn and the staging of host frames: BatchedOp, frame_op.h)
struct g1s_grain : BatchedOp {
  bool clip_restricted = false, mc_identity = false;
  Event ev[3];
  GrainGeom geom_k{};  // what the kernels take: BatchedOp::geom and the block counts, the template sizes
  // the batch being filled
  std::vector<GrainJob> jobs;
  std::vector<GrainSeg> segs;
  struct HostOut {
    uint32_t slot;
    HostPlanes planes;
  };
  std::vector<HostOut> host_outs;  // frames whose out planes are host memory: copied back behind the kernels
  // device buffers
  ParamSets<GrainJob> p_jobs;
  ParamSets<GrainSeg> p_segs;
  DevBuf<uint16_t> d_jump;
  DevBuf<int16_t> d_tpl;
  DevBuf<uint8_t> d_offs, d_luts;
  size_t offs_cap = 0;
  double ms_template = 0, ms_apply = 0;
  uint64_t frames_timed = 0;

  int set_geometry(const g1s_frame_t &f);
  int flush();
  int launch_templates(int set, uint32_t nframes, uint32_t nsegs, const GrainGeom &g);
};

namespace {

// g1s_segment_t -> GrainSeg, with the checks the kernels rely on.  "" when fine.
std::string make_seg(const g1s_segment_t &s, GrainSeg &o) {
  std::memset(&o, 0, sizeof o);
  if (s.ar_coeff_lag > 3) return "ar_coeff_lag must be 0..3";
  if (s.ar_coeff_shift < 6 || s.ar_coeff_shift > 9) return "ar_coeff_shift must be 6..9";
  if (s.scaling_shift < 8 || s.scaling_shift > 11) return "scaling_shift must be 8..11";
  if (s.grain_scale_shift > 3) return "grain_scale_shift must be 0..3";
  if (s.num_y_points > G1S_NUM_Y_POINTS || s.num_cb_points > G1S_NUM_UV_POINTS || s.num_cr_points > G1S_NUM_UV_POINTS)
    return "too many scaling points";
  const int ny = 2 * s.ar_coeff_lag * (s.ar_coeff_lag + 1);
  if (s.num_y_coeffs < ny || s.num_uv_coeffs < ny + 1) return "fewer AR coefficients than ar_coeff_lag needs";
  auto increasing = [](const uint8_t (*p)[2], int n) {
    for (int i = 1; i < n; ++i)
      if (p[i][0] <= p[i - 1][0]) return false;
    return true;
  };
  if (!increasing(s.scaling_points_y, s.num_y_points) || !increasing(s.scaling_points_cb, s.num_cb_points) ||
      !increasing(s.scaling_points_cr, s.num_cr_points))
    return "scaling point values must be strictly increasing";
  std::memcpy(o.cy, s.ar_coeffs_y, ny);
  std::memcpy(o.ccb, s.ar_coeffs_cb, ny + 1);
  std::memcpy(o.ccr, s.ar_coeffs_cr, ny + 1);
  std::memcpy(o.py, s.scaling_points_y, 2 * s.num_y_points);
  std::memcpy(o.pcb, s.scaling_points_cb, 2 * s.num_cb_points);
  std::memcpy(o.pcr, s.scaling_points_cr, 2 * s.num_cr_points);
  o.lag = s.ar_coeff_lag, o.ar_shift = s.ar_coeff_shift, o.grain_scale_shift = s.grain_scale_shift, o.scaling_shift = s.scaling_shift;
  o.num_y = s.num_y_points, o.num_cb = s.num_cb_points, o.num_cr = s.num_cr_points;
  o.csfl = s.chroma_scaling_from_luma != 0, o.overlap = s.overlap_flag != 0;
  o.cb_mult = (int16_t)((int)s.cb_mult - 128), o.cb_luma_mult = (int16_t)((int)s.cb_luma_mult - 128), o.cb_offset = (int16_t)((int)s.cb_offset - 256);
  o.cr_mult = (int16_t)((int)s.cr_mult - 128), o.cr_luma_mult = (int16_t)((int)s.cr_luma_mult - 128), o.cr_offset = (int16_t)((int)s.cr_offset - 256);
  return "";
}

GrainGeom template_geom(uint32_t bit_depth, int subx, int suby, int nplanes) {
  GrainGeom g{};
  g.bit_depth = (int)bit_depth, g.subx = subx, g.suby = suby, g.nplanes = nplanes;
  g.cw = subx ? 44 : kLumaW, g.ch = suby ? 38 : kLumaH;
  return g;
}

}  // namespace

int g1s_grain::set_geometry(const g1s_frame_t &f) {
  GrainGeom g = template_geom(bit_depth, f.xdec, f.ydec, f.nplanes);
  g.W = (int)f.width, g.H = (int)f.height;
  g.nbx = (((g.W + 1) >> 1) + 15) / 16, g.nstripes = (((g.H + 1) >> 1) + 15) / 16;
  geom_k = g;
  set_frame_geometry(f);
  const size_t need = (size_t)g.nstripes * g.nbx * batch;
  if (need > offs_cap) {
    d_offs = DevBuf<uint8_t>();
    G1S_OP_TRY(hipMalloc((void **)&d_offs.p, need));
    offs_cap = need;
  }
  return G1S_OK;
}

int g1s_grain::launch_templates(int set, uint32_t nframes, uint32_t nsegs, const GrainGeom &g) {
  TemplateParams tp{};
  tp.jobs = p_jobs.d[set], tp.segs = p_segs.d[set], tp.jump = d_jump, tp.tpl = d_tpl, tp.offs = d_offs, tp.luts = d_luts;
  tp.nframes = (int)nframes, tp.nsegs = (int)nsegs, tp.g = g;
  hipLaunchKernelGGL(kg_template, dim3(nframes + nsegs), dim3(kThreads), 0, stream, tp);
  G1S_OP_TRY(hipGetLastError());
  return G1S_OK;
}

int g1s_grain::flush() {
  const uint32_t B = (uint32_t)jobs.size();
  if (!B) return G1S_OK;
  int set, rc = next_set(&set);
  if (rc) return rc;
  std::memcpy(p_jobs.h[set], jobs.data(), sizeof(GrainJob) * B);
  G1S_OP_TRY(p_jobs.upload(set, B, stream));
  if (!segs.empty()) {
    std::memcpy(p_segs.h[set], segs.data(), sizeof(GrainSeg) * segs.size());
    G1S_OP_TRY(p_segs.upload(set, segs.size(), stream));
  }
  if (timing) G1S_OP_TRY(hipEventRecord(ev[0], stream));
  if (!segs.empty() && (rc = launch_templates(set, B, (uint32_t)segs.size(), geom_k)) != 0) return rc;
  if (timing) G1S_OP_TRY(hipEventRecord(ev[1], stream));
  ApplyParams ap{};
  ap.jobs = p_jobs.d[set], ap.segs = p_segs.d[set], ap.tpl = d_tpl, ap.offs = d_offs, ap.luts = d_luts, ap.g = geom_k;
  const int sh = (int)bit_depth - 8;
  ap.min_value = clip_restricted ? 16 << sh : 0;
  ap.max_luma = clip_restricted ? 235 << sh : (256 << sh) - 1;
  ap.max_chroma = clip_restricted ? (mc_identity ? 235 << sh : 240 << sh) : (256 << sh) - 1;
  const dim3 grid((unsigned)geom_k.nstripes, B);
  const size_t lds = apply_lds_bytes(geom_k);
  if (bps == 2) hipLaunchKernelGGL(kg_apply<2>, grid, dim3(kThreads), lds, stream, ap);
  else hipLaunchKernelGGL(kg_apply<1>, grid, dim3(kThreads), lds, stream, ap);
  G1S_OP_TRY(hipGetLastError());
  if (timing) G1S_OP_TRY(hipEventRecord(ev[2], stream));
  if ((rc = set_done(set)) != 0) return rc;
  for (const HostOut &h : host_outs)
    if ((rc = copy_back(h.slot, h.planes)) != 0) return rc;
  if (timing) {
    G1S_OP_TRY(hipStreamSynchronize(stream));
    float a = 0, b = 0;
    G1S_OP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    G1S_OP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
    ms_template += a, ms_apply += b, frames_timed += B;
  }
  jobs.clear();
  segs.clear();
  host_outs.clear();
  return G1S_OK;
}

extern "C" {

const int16_t *g1s_grain_gaussian_sequence(void) { return kGaussHost; }

g1s_grain_t *g1s_grain_new(uint32_t bit_depth, const g1s_grain_opts_t *opts) {
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return refuse_new("film grain synthesis is defined for bit depths 8, 10 and 12");
  return new_op<g1s_grain>("film grain synthesis", opts, "g1s_grain_opts_t", bit_depth, [&](g1s_grain &g, std::string &) {
    g.clip_restricted = opts && opts->clip_to_restricted_range;
    g.mc_identity = opts && opts->mc_identity;
    // the jump table: column b of M^(24 l) is the register 24 l steps after the seed 1 << b
    std::vector<uint16_t> jump((size_t)kThreads * 16);
    for (int b = 0; b < 16; ++b) {
      uint32_t r = 1u << b;
      for (int l = 0; l < kThreads; ++l) {
        jump[(size_t)l * 16 + b] = (uint16_t)r;
        for (int k = 0; k < kDrawsPerLane; ++k) r = lfsr_step(r);
      }
    }
    const uint32_t B = g.batch;
    bool ok = true;
    for (Event &e : g.ev) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    return ok && g.p_jobs.alloc(B) && g.p_segs.alloc(B) && hipMalloc((void **)&g.d_jump.p, jump.size() * 2) == hipSuccess &&
           hipMalloc((void **)&g.d_tpl.p, sizeof(int16_t) * 3 * kTplSlot * B) == hipSuccess && hipMalloc((void **)&g.d_luts.p, (size_t)768 * B) == hipSuccess &&
           hipMemcpy(g.d_jump, jump.data(), jump.size() * 2, hipMemcpyHostToDevice) == hipSuccess;
  });
}

int g1s_grain_frame(g1s_grain_t *g, const g1s_segment_t *params, const g1s_frame_t *in, g1s_frame_t *out) {
  if (!g || !in || !out) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  const Refusal no = check_frame_pair(*in, *out, g->bps, 32u * kMaxBlocksX, "g1s_grain_new",
                                      "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, width up to 16384)");
  if (no.code) return g->fail(no.code, no.text);
  int rc;
  if (g->have_geom && !g->geom.same_shape(*in)) {
    // a new geometry: what is queued goes out and finishes first, the staging buffers are sized again
    if ((rc = g->flush()) != 0) return rc;
    if (hipStreamSynchronize(g->stream) != hipSuccess) return g->fail(G1S_ERR_HIP, "hipStreamSynchronize failed");
    g->have_geom = false;
  }
  if (!g->have_geom && (rc = g->set_geometry(*in)) != 0) return rc;
  GrainJob job{};
  job.seg = kNoSegment;
  if (params) {
    GrainSeg sg;
    const std::string why = make_seg(*params, sg);
    if (!why.empty()) return g->fail(G1S_ERR_INVALID, why);
    size_t k = 0;
    while (k < g->segs.size() && std::memcmp(&g->segs[k], &sg, sizeof sg) != 0) ++k;
    if (k == g->segs.size()) g->segs.push_back(sg);
    job.seg = (uint32_t)k;
    job.seed = params->random_seed;
  }
  // input and output staging are `batch` slots each; a frame's slot is its place in the batch being filled
  const uint32_t slot = (uint32_t)g->jobs.size();
  if ((rc = g->stage_in(*in, slot, g->batch, job.in, job.in_stride)) != 0) return rc;
  const bool host_out = out->on_device != 1;
  if (host_out && (rc = g->need_stage_out(g->batch)) != 0) return rc;
  for (int c = 0; c < g->geom.nplanes; ++c) {
    job.out[c] = host_out ? g->stage_out(slot, c) : static_cast<uint8_t *>(const_cast<void *>(out->data[c]));
    job.out_stride[c] = host_out ? (uint32_t)g->stage.row[c] : (uint32_t)out->stride_bytes[c];
    // in != out: a plane of the output must not overlap the same plane of the input or its luma
    if (planes_overlap(g->geom, job.out[c], job.out_stride[c], c, job.in[0], job.in_stride[0], 0) ||
        planes_overlap(g->geom, job.out[c], job.out_stride[c], c, job.in[c], job.in_stride[c], c))
      return g->fail(G1S_ERR_INVALID, "input and output planes overlap: g1s_grain_frame needs distinct buffers");
  }
  if ((rc = g->wait_host_input(*in)) != 0) return rc;
  if (host_out) g->host_outs.push_back({slot, host_planes(*out)});
  g->jobs.push_back(job);
  return g->jobs.size() >= g->batch ? g->flush() : G1S_OK;
}

int g1s_grain_sync(g1s_grain_t *g) {
  if (!g) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  const int rc = g->flush();
  return rc ? rc : g->wait();
}


int g1s_grain_templates(g1s_grain_t *g, const g1s_segment_t *params, uint32_t xdec, uint32_t ydec, int16_t *luma, int16_t *cb, int16_t *cr,
                        uint8_t lut[3][256]) {
  if (!g || !params || xdec > 1 || ydec > xdec) return G1S_ERR_INVALID;
  if (g->err_code) return g->err_code;
  (void)hipSetDevice(g->device);
  int rc = g->flush();  // (the batch buffers are about to be reused)
  if (rc) return rc;
  if (hipStreamSynchronize(g->stream) != hipSuccess) return g->fail(G1S_ERR_HIP, "hipStreamSynchronize failed");
  GrainSeg sg;
  const std::string why = make_seg(*params, sg);
  if (!why.empty()) return g->fail(G1S_ERR_INVALID, why);
  GrainJob job{};
  job.seg = 0, job.seed = params->random_seed;
  const GrainGeom tg = template_geom(g->bit_depth, (int)xdec, (int)ydec, 3);
  // (everything queued has finished: set 0 is free)
  *g->p_jobs.h[0] = job, *g->p_segs.h[0] = sg;
  if (g->p_jobs.upload(0, 1, g->stream) != hipSuccess || g->p_segs.upload(0, 1, g->stream) != hipSuccess)
    return g->fail(G1S_ERR_HIP, "upload of the template job failed");
  rc = g->launch_templates(0, 1, 1, tg);
  if (rc) return rc;
  const size_t nc = (size_t)tg.cw * tg.ch;
  bool ok = true;
  if (luma) ok = ok && hipMemcpyAsync(luma, g->d_tpl, sizeof(int16_t) * kLumaW * kLumaH, hipMemcpyDeviceToHost, g->stream) == hipSuccess;
  if (cb) ok = ok && hipMemcpyAsync(cb, g->d_tpl + kTplSlot, sizeof(int16_t) * nc, hipMemcpyDeviceToHost, g->stream) == hipSuccess;
  if (cr) ok = ok && hipMemcpyAsync(cr, g->d_tpl + 2 * kTplSlot, sizeof(int16_t) * nc, hipMemcpyDeviceToHost, g->stream) == hipSuccess;
  if (lut) ok = ok && hipMemcpyAsync(lut, g->d_luts, 768, hipMemcpyDeviceToHost, g->stream) == hipSuccess;
  ok = ok && hipStreamSynchronize(g->stream) == hipSuccess;
  if (!ok) return g->fail(G1S_ERR_HIP, std::string("reading the templates back failed: ") + hipGetErrorString(hipGetLastError()));
  return G1S_OK;
}

int g1s_grain_set_timing(g1s_grain_t *g, int enable, double *ms_template, double *ms_apply, uint64_t *frames) {
  if (!g) return G1S_ERR_INVALID;
  g->timing = enable != 0;
  if (ms_template) *ms_template = g->ms_template;
  if (ms_apply) *ms_apply = g->ms_apply;
  if (frames) *frames = g->frames_timed;
  return G1S_OK;
}

const char *g1s_grain_last_error(const g1s_grain_t *g) { return g ? g->err.c_str() : ""; }

void g1s_grain_free(g1s_grain_t *g) { free_op(g); }

}  // extern "C"
