"""The temporal non-local-means filter (include/g1s_diff.h, "denoise", rules 1 - 7) restated in numpy.

Rules 1 - 4 are tests/denoise_ref.py's; this adds the frames around the one in hand (rules 5 - 7).  int64 throughout, the
weight table an argument as there.  A clip is a list of frames, a frame a list of planes.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np


def _sums(u: np.ndarray, v: Optional[np.ndarray], A: int, S: int, tab: np.ndarray, q: int) -> Tuple[np.ndarray, np.ndarray]:
    """(sum w v(p + d), sum w) over the offsets that take part, patches of u at p against patches of v at p + d.  v = None:
    the frame itself (rules 1 - 3: d = 0 carries 4096); else a neighbour (rule 6: every offset, d = 0 with its distance)."""
    h, w = u.shape
    R = A + S
    pu = np.pad(u, R, mode="edge")
    pv = pu if v is None else np.pad(v, R, mode="edge")
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    num, den = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    k = 2 * S + 1
    for dy in range(-A, A + 1):
        for dx in range(-A, A + 1):
            if v is None and dx == 0 and dy == 0:
                num += 4096 * u
                den += 4096
                continue
            a = pu[A:A + h + 2 * S, A:A + w + 2 * S]
            b = pv[A + dy:A + dy + h + 2 * S, A + dx:A + dx + w + 2 * S]
            c = np.zeros((h + 2 * S + 1, w + 2 * S + 1), np.int64)
            c[1:, 1:] = np.cumsum(np.cumsum((a - b) ** 2, 0), 1)
            D = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
            wgt = tab[np.minimum(D >> q, 1023)]
            part = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)
            wgt = np.where(part, wgt, 0)
            num += wgt * pv[R + dy:R + dy + h, R + dx:R + dx + w]
            den += wgt
    return num, den


def sums_plane(planes: Sequence[np.ndarray], t: int, temporal_radius: int, search_radius: int, patch_radius: int, table: np.ndarray,
               q: int) -> Tuple[np.ndarray, np.ndarray]:
    """(numerator without the rounding term, denominator) of rule 7 for frame t of a clip of planes."""
    tab = np.asarray(table).astype(np.int64)
    assert tab.shape == (1024,)
    u = np.asarray(planes[t]).astype(np.int64)
    num, den = _sums(u, None, search_radius, patch_radius, tab, q)
    for k in range(-temporal_radius, temporal_radius + 1):
        if k == 0 or not 0 <= t + k < len(planes):  # rule 5: skipped, not clamped
            continue
        v = np.asarray(planes[t + k]).astype(np.int64)
        assert v.shape == u.shape
        n, d = _sums(u, v, search_radius, patch_radius, tab, q)
        num += n
        den += d
    return num, den


def denoise_plane_clip(planes: Sequence[np.ndarray], temporal_radius: int, search_radius: int, patch_radius: int, table: np.ndarray,
                       q: int) -> List[np.ndarray]:
    """The same plane of every frame of a clip through rules 1 - 7."""
    out = []
    for t in range(len(planes)):
        num, den = sums_plane(planes, t, temporal_radius, search_radius, patch_radius, table, q)
        out.append(((num + (den >> 1)) // den).astype(np.asarray(planes[t]).dtype))
    return out


def denoise_clip(frames: Sequence[Sequence[np.ndarray]], temporal_radius: int, search_radius: int, patch_radius: int,
                 luma: Tuple[np.ndarray, int], chroma: Tuple[np.ndarray, int]) -> List[List[np.ndarray]]:
    """Every plane on its own grid; `luma` / `chroma` are the (T, q) of the two strengths.  Returns frames of planes."""
    nplanes = len(frames[0])
    per_plane = [denoise_plane_clip([f[c] for f in frames], temporal_radius, search_radius, patch_radius, *(luma if c == 0 else chroma))
                 for c in range(nplanes)]
    return [[per_plane[c][t] for c in range(nplanes)] for t in range(len(frames))]
