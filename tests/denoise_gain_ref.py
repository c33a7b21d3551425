"""A chroma gain for the joint chroma filter (include/g1s_diff.h, "denoise", rules 21 - 24, and N9 of "noise levels")
restated in numpy and plain Python integers.

gain_from_s() is rule 21, s_from_segments() rule 22, chroma_sigma() rule 23 (N9), sums() rule 24 on top of the joint filter
of tests/denoise_joint_ref.py and, under motion, of tests/denoise_motion_ref.py: the same patches, the same parts that take
part, the weight looked up at (D_J mp) >> (q_J + 8).  int64 throughout: D_J < 2^32 and mp <= 2^14, so the product stays
below 2^46.  sums_pairs() is the same rule as a plain loop over pairs, for small planes.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import denoise_joint_ref as J
from tests import denoise_motion_ref as M
from tests import nlf_ref as NR

FLAT = np.full(256, 256, np.uint16)


# ------------------------------------------------------------------------------------------------------------ rule 21
def gain_from_s(s: Sequence[int], range_: int = 0) -> np.ndarray:
    """Rule 21: m[256] (uint16) from s(i), i = 0 .. 255, and a range R (0 = 4)."""
    if not 0 <= range_ <= 8:
        raise ValueError("chroma gain range must be 1..8 (0 = the default)")
    R = range_ or 4
    s = [int(v) for v in s]
    assert len(s) == 256 and all(0 <= v <= 255 for v in s)
    top = max(s)
    floor = max(1, -(-top // R))
    sp = [max(v, floor) for v in s]
    sbar = (sum(sp) + 128) >> 8
    return np.array([min(16384, max(1, (256 * sbar * sbar + ((v * v) >> 1)) // (v * v))) for v in sp], np.uint16)


# ------------------------------------------------------------------------------------------------------------ rule 22
def scaling_lut(points: Sequence[Tuple[int, int]]) -> List[int]:
    """7.18.3.4: 256 entries through the points, flat outside them, zero without points."""
    lut = [0] * 256
    if not points:
        return lut
    for k in range(len(points) - 1):
        if points[k + 1][0] <= points[k][0]:
            raise ValueError("scaling points must have increasing values")
    for x in range(points[0][0]):
        lut[x] = points[0][1]
    for (x0, y0), (x1, y1) in zip(points, points[1:]):
        dx, dy = x1 - x0, y1 - y0
        delta = dy * ((65536 + (dx >> 1)) // dx)
        for x in range(dx):
            lut[x0 + x] = y0 + ((x * delta + 32768) >> 16)  # (>> of a negative Python int floors: the arithmetic shift)
    for x in range(points[-1][0], 256):
        lut[x] = points[-1][1]
    return lut


def chroma_index(v: int, luma_mult: int, mult: int, offset: int) -> int:
    """idx(v) of rule 22 without chroma_scaling_from_luma: 7.18.3.5 at 8 bits with the chroma sample at mid-grey."""
    return min(255, max(0, ((v * (luma_mult - 128) + 128 * (mult - 128)) >> 6) + (offset - 256)))


def s_from_segments(segments: Sequence) -> np.ndarray:
    """Rule 22: s[256] (uint8), the rounded mean of the chroma scaling functions of both chroma planes of the segments
    (objects with the fields of GrainTableSegment) at the luma under them."""
    n = len(segments)
    if n < 1:
        raise ValueError("a grain prior needs at least one segment")
    total = [0] * 256
    for sg in segments:
        luma = scaling_lut(list(sg.scaling_points_y))
        for pts, lm, mu, off in ((sg.scaling_points_cb, sg.cb_luma_mult, sg.cb_mult, sg.cb_offset),
                                 (sg.scaling_points_cr, sg.cr_luma_mult, sg.cr_mult, sg.cr_offset)):
            lut = luma if sg.chroma_scaling_from_luma else scaling_lut(list(pts))
            for v in range(256):
                total[v] += lut[v if sg.chroma_scaling_from_luma else chroma_index(v, lm, mu, off)]
    return np.array([(t + n) // (2 * n) for t in total], np.uint8)


def chroma_gain(segments: Sequence, range_: int = 0) -> np.ndarray:
    """Rules 22 + 21."""
    return gain_from_s(s_from_segments(segments), range_)


# ------------------------------------------------------------------------------------------------------- rule 23 (N9)
def chroma_sigma(total: dict, min_count: int = 0) -> np.ndarray:
    """N9: s[256] (uint8) from the chroma bins of a record of tests/nlf_ref.py, planes 1 and 2 pooled; ValueError with the
    refusal's text where the rule refuses.  The same for every bit depth."""
    nmin = min_count or NR.DEFAULT_MIN_COUNT
    t = []
    for k in range(NR.BINS):
        n = int(total["n"][1, k]) + int(total["n"][2, k])
        q = int(total["q"][1, k]) + int(total["q"][2, k])
        t.append(math.isqrt((q << 16) // (36 * n)) if n >= nmin else None)
    valid = [k for k in range(NR.BINS) if t[k] is not None]
    if not valid:
        raise ValueError("no chroma bin has enough smooth samples for a prior")
    tmax = max(t[k] for k in valid)
    y = [max(1, 255 * t[k] // max(tmax, 1)) for k in valid]
    c = [8 * k + 4 for k in valid]
    s = np.zeros(256, np.uint8)
    for v in range(256):
        if v <= c[0]:
            s[v] = y[0]
        elif v >= c[-1]:
            s[v] = y[-1]
        else:
            i = max(j for j in range(len(c)) if c[j] <= v)
            s[v] = y[i] + ((y[i + 1] - y[i]) * (v - c[i]) * 2 + (c[i + 1] - c[i])) // (2 * (c[i + 1] - c[i]))  # (// floors)
    return s


# ------------------------------------------------------------------------------------------------------------ rule 24
def pair_gain(m: np.ndarray, ga: np.ndarray, gb: np.ndarray, shift: int) -> np.ndarray:
    """mp of rule 24 for guide samples ga at p and gb at p'."""
    return (m[np.minimum(ga >> shift, 255)] + m[np.minimum(gb >> shift, 255)] + 1) >> 1


def sums(us: Sequence[np.ndarray], vs: Optional[Sequence[np.ndarray]], mv: Optional[np.ndarray], A: int, S: int, tab: np.ndarray, q: int,
         gain: np.ndarray, shift: int, pair=pair_gain, wrap32: bool = False, unmoved_guide: bool = False):
    """([sum w Cb(p'), sum w Cr(p')], sum w) under a gain: us = (Cb, Cr, G) of the frame, vs the same of a neighbour frame
    (None: the frame itself, d = 0 carrying 4096), mv the field of vectors towards it (None: no motion), p' = p + m + d.
    `pair`, `wrap32` and `unmoved_guide` (the neighbour's guide read at p + d, not p + m + d) let a test restate the rule wrongly
    on purpose."""
    m = np.asarray(gain).astype(np.int64)
    tab = np.asarray(tab).astype(np.int64)
    h, w = us[0].shape
    if mv is None:
        mv = np.zeros((-(-h // M.BH), -(-w // M.BW), 2), np.int64)
    R = A + S
    pad = R + int(np.abs(mv).max(initial=0))
    pu = [np.pad(u, R, mode="edge") for u in us]
    pv = [np.pad(v, pad, mode="edge") for v in (us if vs is None else vs)]
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    nums, den = [np.zeros((h, w), np.int64) for _ in range(2)], np.zeros((h, w), np.int64)
    k = 2 * S + 1
    for mx, my in sorted({(int(a), int(b)) for a, b in mv.reshape(-1, 2)}):
        n1, d1 = [np.zeros((h, w), np.int64) for _ in range(2)], np.zeros((h, w), np.int64)
        for dy in range(-A, A + 1):
            for dx in range(-A, A + 1):
                if vs is None and dx == 0 and dy == 0:
                    n1[0] += 4096 * us[0]
                    n1[1] += 4096 * us[1]
                    d1 += 4096
                    continue
                oy, ox = pad + my + dy, pad + mx + dx
                e = np.zeros((h + 2 * S, w + 2 * S), np.int64)
                for a, b in zip(pu, pv):
                    e += (a[A:A + h + 2 * S, A:A + w + 2 * S] - b[oy - S:oy - S + h + 2 * S, ox - S:ox - S + w + 2 * S]) ** 2
                c = np.zeros((h + 2 * S + 1, w + 2 * S + 1), np.int64)
                c[1:, 1:] = np.cumsum(np.cumsum(e, 0), 1)
                D = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
                assert D.max() < 2 ** 32
                gy, gx = (oy - my, ox - mx) if unmoved_guide else (oy, ox)
                prod = D * pair(m, us[2], pv[2][gy:gy + h, gx:gx + w], shift)
                assert prod.max() < 2 ** 47
                if wrap32:
                    prod &= 0xFFFFFFFF
                wgt = tab[np.minimum(prod >> (q + 8), 1023)]
                part = (xs + mx + dx >= 0) & (xs + mx + dx < w) & (ys + my + dy >= 0) & (ys + my + dy < h)
                wgt = np.where(part, wgt, 0)
                for n in range(2):
                    n1[n] += wgt * pv[n][oy:oy + h, ox:ox + w]
                d1 += wgt
        mine = np.repeat(np.repeat((mv[:, :, 0] == mx) & (mv[:, :, 1] == my), M.BH, 0), M.BW, 1)[:h, :w]
        for n in range(2):
            nums[n] += np.where(mine, n1[n], 0)
        den += np.where(mine, d1, 0)
    return nums, den


def sums_pairs(us, vs, mv, A, S, tab, q, gain, shift):
    """sums() as a plain loop over the pairs (p, p'), one Python integer at a time: for small planes."""
    h, w = us[0].shape
    src = us if vs is None else vs
    cl = lambda v, n: min(max(v, 0), n - 1)  # noqa: E731
    nums, den = [np.zeros((h, w), np.int64) for _ in range(2)], np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            mx, my = (0, 0) if mv is None else (int(v) for v in mv[y // M.BH, x // M.BW])
            for dy in range(-A, A + 1):
                for dx in range(-A, A + 1):
                    if vs is None and dx == 0 and dy == 0:
                        wgt, py, px = 4096, y, x
                    else:
                        py, px = y + my + dy, x + mx + dx
                        if not (0 <= px < w and 0 <= py < h):
                            continue
                        D = 0
                        for ky in range(-S, S + 1):
                            for kx in range(-S, S + 1):
                                for a, b in zip(us, src):
                                    D += (int(a[cl(y + ky, h), cl(x + kx, w)]) - int(b[cl(py + ky, h), cl(px + kx, w)])) ** 2
                        ma, mb = int(gain[min(int(us[2][y, x]) >> shift, 255)]), int(gain[min(int(src[2][py, px]) >> shift, 255)])
                        wgt = int(tab[min((D * ((ma + mb + 1) >> 1)) >> (q + 8), 1023)])
                    nums[0][y, x] += wgt * int(src[0][py, px])
                    nums[1][y, x] += wgt * int(src[1][py, px])
                    den[y, x] += wgt
    return nums, den


def chroma_sums(frames, t, xdec, ydec, temporal_radius, search_radius, patch_radius, table, q, gain, bit_depth, mr=0, **wrong):
    """(numerator of Cb, numerator of Cr, denominator) of frame t of a clip of [Y, Cb, Cr] frames under a gain."""
    shift = bit_depth - 8
    us = J._triple(frames[t], xdec, ydec)
    (nb, nr), den = sums(us, None, None, search_radius, patch_radius, table, q, gain, shift, **wrong)
    for k in range(-temporal_radius, temporal_radius + 1):
        if k == 0 or not 0 <= t + k < len(frames):  # rule 5
            continue
        vs = J._triple(frames[t + k], xdec, ydec)
        mv = M.search(us[:2], vs[:2], mr) if mr else None
        (b, r), d = sums(us, vs, mv, search_radius, patch_radius, table, q, gain, shift, **wrong)
        nb, nr, den = nb + b, nr + r, den + d
    return nb, nr, den


def denoise_chroma_clip(frames, xdec, ydec, temporal_radius, search_radius, patch_radius, table, q, gain, bit_depth, mr=0, **wrong):
    """(out_Cb, out_Cr) of every frame of a clip under the joint flag and a gain."""
    out = []
    for t in range(len(frames)):
        nb, nr, den = chroma_sums(frames, t, xdec, ydec, temporal_radius, search_radius, patch_radius, table, q, gain, bit_depth, mr, **wrong)
        dt = np.asarray(frames[t][1]).dtype
        out.append((((nb + (den >> 1)) // den).astype(dt), ((nr + (den >> 1)) // den).astype(dt)))
    return out


def denoise_clip(frames, xdec, ydec, temporal_radius, search_radius, patch_radius, luma, joint, gain, bit_depth, mr=0, curve=None):
    """A clip under the joint flag and a gain: luma as tests/denoise_motion_ref.py has it (the gain never reaches it), chroma
    by rule 24 with `joint` = (T_J, q_J).  A luma-only frame is filtered as without the gain."""
    ys = M.denoise_clip([f[:1] for f in frames], xdec, ydec, temporal_radius, search_radius, patch_radius, luma, joint, mr, True, curve)
    if len(frames[0]) == 1:
        return ys
    cs = denoise_chroma_clip(frames, xdec, ydec, temporal_radius, search_radius, patch_radius, *joint, gain, bit_depth, mr)
    return [[y[0], cb, cr] for y, (cb, cr) in zip(ys, cs)]

