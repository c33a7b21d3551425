"""The luma-guided joint chroma filter (include/g1s_diff.h, "denoise", rules 8 - 11t) restated in numpy.

Cb and Cr share one weight, taken from both and the guide G: the frame's input luma at chroma resolution.  Integer
arithmetic only (int64 throughout), the weight table an argument as in tests/denoise_ref.py.  A clip is a list of frames,
a frame a list of three planes [Y, Cb, Cr]; luma goes through tests/denoise_temporal_ref.py unchanged.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import denoise_temporal_ref as TR


def joint_table_from_formula(bit_depth: int, patch_radius: int, strength: float) -> Tuple[np.ndarray, int]:
    """(T_J, q_J) of rule 10: rule 3 with n replaced by 3 n, the non-increasing clamp included."""
    n = 3 * (2 * patch_radius + 1) ** 2

    def entry(i: int, q: int) -> float:
        x = ((i + 0.5) * 2.0 ** q) / (n * strength * strength * 4.0 ** (bit_depth - 8))
        return 4096.0 * math.exp(-x) if x < 700 else 0.0

    q = 0
    while math.floor(entry(1023, q) + 0.5) != 0:
        q += 1
    t = [4096]
    for i in range(1, 1024):
        t.append(min(int(math.floor(entry(i, q) + 0.5)), t[-1]))
    return np.array(t, np.uint16), q


def guide(y: np.ndarray, xdec: int, ydec: int) -> np.ndarray:
    """Rule 8: the luma plane at chroma resolution, a rounded box mean, luma coordinates clamped to the plane."""
    y = np.asarray(y).astype(np.int64)
    H, W = y.shape
    cw, ch = (W + xdec) >> xdec, (H + ydec) >> ydec
    s = np.zeros((ch, cw), np.int64)
    for j in range(ydec + 1):
        rows = np.minimum((np.arange(ch) << ydec) + j, H - 1)
        for i in range(xdec + 1):
            cols = np.minimum((np.arange(cw) << xdec) + i, W - 1)
            s += y[rows[:, None], cols[None, :]]
    sh = xdec + ydec
    return (s + ((1 << sh) >> 1)) >> sh


def _sums(us: Sequence[np.ndarray], vs: Optional[Sequence[np.ndarray]], A: int, S: int, tab: np.ndarray, q: int):
    """(sum w Cb(p + d), sum w Cr(p + d), sum w) over the offsets that take part; us = (Cb, Cr, G) of the frame, vs the
    same of a neighbour frame (None: the frame itself, rules 8 - 10 with d = 0 carrying 4096)."""
    h, w = us[0].shape
    Rr = A + S
    pu = [np.pad(u, Rr, mode="edge") for u in us]
    pv = pu if vs is None else [np.pad(v, Rr, mode="edge") for v in vs]
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    nb, nr, den = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    k = 2 * S + 1
    for dy in range(-A, A + 1):
        for dx in range(-A, A + 1):
            if vs is None and dx == 0 and dy == 0:
                nb += 4096 * us[0]
                nr += 4096 * us[1]
                den += 4096
                continue
            e = np.zeros((h + 2 * S, w + 2 * S), np.int64)
            for a, b in zip(pu, pv):  # rule 9: the three planes' squared differences, summed
                e += (a[A:A + h + 2 * S, A:A + w + 2 * S] - b[A + dy:A + dy + h + 2 * S, A + dx:A + dx + w + 2 * S]) ** 2
            c = np.zeros((h + 2 * S + 1, w + 2 * S + 1), np.int64)
            c[1:, 1:] = np.cumsum(np.cumsum(e, 0), 1)
            D = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
            assert D.max() < 2 ** 32
            wgt = tab[np.minimum(D >> q, 1023)]
            part = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)
            wgt = np.where(part, wgt, 0)
            nb += wgt * pv[0][Rr + dy:Rr + dy + h, Rr + dx:Rr + dx + w]
            nr += wgt * pv[1][Rr + dy:Rr + dy + h, Rr + dx:Rr + dx + w]
            den += wgt
    return nb, nr, den


def _triple(frame: Sequence[np.ndarray], xdec: int, ydec: int):
    cb, cr = np.asarray(frame[1]).astype(np.int64), np.asarray(frame[2]).astype(np.int64)
    g = guide(frame[0], xdec, ydec)
    assert cb.shape == cr.shape == g.shape, (cb.shape, cr.shape, g.shape)
    return cb, cr, g


def max_distance(frame: Sequence[np.ndarray], xdec: int, ydec: int, A: int, S: int) -> int:
    """The largest D_J of the frame itself (for the test of the 32-bit ceiling)."""
    us = _triple(frame, xdec, ydec)
    h, w = us[0].shape
    pu = [np.pad(u, A + S, mode="edge") for u in us]
    k, best = 2 * S + 1, 0
    for dy in range(-A, A + 1):
        for dx in range(-A, A + 1):
            e = sum((a[A:A + h + 2 * S, A:A + w + 2 * S] - a[A + dy:A + dy + h + 2 * S, A + dx:A + dx + w + 2 * S]) ** 2 for a in pu)
            c = np.zeros((h + 2 * S + 1, w + 2 * S + 1), np.int64)
            c[1:, 1:] = np.cumsum(np.cumsum(e, 0), 1)
            best = max(best, int((c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]).max()))
    return best


def chroma_sums(frames: Sequence[Sequence[np.ndarray]], t: int, xdec: int, ydec: int, temporal_radius: int, search_radius: int,
                patch_radius: int, table: np.ndarray, q: int):
    """(numerator of Cb, numerator of Cr, denominator) of rule 11 / 11t for frame t of a clip, without the rounding term."""
    tab = np.asarray(table).astype(np.int64)
    assert tab.shape == (1024,)
    us = _triple(frames[t], xdec, ydec)
    nb, nr, den = _sums(us, None, search_radius, patch_radius, tab, q)
    for k in range(-temporal_radius, temporal_radius + 1):
        if k == 0 or not 0 <= t + k < len(frames):  # rule 5
            continue
        b, r, d = _sums(us, _triple(frames[t + k], xdec, ydec), search_radius, patch_radius, tab, q)
        nb += b
        nr += r
        den += d
    return nb, nr, den


def denoise_chroma_clip(frames: Sequence[Sequence[np.ndarray]], xdec: int, ydec: int, temporal_radius: int, search_radius: int,
                        patch_radius: int, table: np.ndarray, q: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """(out_Cb, out_Cr) of every frame of a clip."""
    out = []
    for t in range(len(frames)):
        nb, nr, den = chroma_sums(frames, t, xdec, ydec, temporal_radius, search_radius, patch_radius, table, q)
        dt = np.asarray(frames[t][1]).dtype
        out.append((((nb + (den >> 1)) // den).astype(dt), ((nr + (den >> 1)) // den).astype(dt)))
    return out


def denoise_clip(frames: Sequence[Sequence[np.ndarray]], xdec: int, ydec: int, temporal_radius: int, search_radius: int, patch_radius: int,
                 luma: Tuple[np.ndarray, int], joint: Tuple[np.ndarray, int]) -> List[List[np.ndarray]]:
    """A clip under the joint flag: luma by rules 1 - 7 with `luma` = (T, q), chroma by rules 8 - 11t with `joint` = (T_J, q_J).
    A luma-only frame is filtered as without the flag."""
    ys = TR.denoise_plane_clip([f[0] for f in frames], temporal_radius, search_radius, patch_radius, *luma)
    if len(frames[0]) == 1:
        return [[y] for y in ys]
    cs = denoise_chroma_clip(frames, xdec, ydec, temporal_radius, search_radius, patch_radius, *joint)
    return [[y, cb, cr] for y, (cb, cr) in zip(ys, cs)]


def denoise_frame(planes: Sequence[np.ndarray], xdec: int, ydec: int, search_radius: int, patch_radius: int, luma: Tuple[np.ndarray, int],
                  joint: Tuple[np.ndarray, int]) -> List[np.ndarray]:
    return denoise_clip([planes], xdec, ydec, 0, search_radius, patch_radius, luma, joint)[0]


def edge_content(seed: int = 5, step: int = 60, sigma: float = 16.0):
    """The 10-bit 4:2:0 frame of the property test: luma 128 x 96 in cells of 16 x 24 at 300 / 700, Cb and Cr 64 x 48 with
    co-located cells `step` code values apart, Gaussian grain of `sigma` on all three.  Returns (clean planes, noisy planes)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.arange(96)[:, None], np.arange(128)[None, :]
    cell = ((xx // 16) + (yy // 24)) & 1
    ccell = cell[::2, ::2]  # co-located: chroma cells of 8 x 12
    clean = [np.where(cell, 700, 300), 512 - step // 2 + step * ccell, 512 + step // 2 - step * ccell]
    noisy = [np.clip(np.rint(p + rng.normal(0.0, sigma, p.shape)), 0, 1023).astype(np.uint16) for p in clean]
    return [p.astype(np.uint16) for p in clean], noisy

