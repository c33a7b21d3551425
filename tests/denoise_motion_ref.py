"""Motion for the temporal radius (include/g1s_diff.h, "denoise", rules 16 - 20) restated in numpy.

half() is rule 16, search() rules 17 and 18, sums_plane() / denoise_plane_clip() rules 5 - 7 with rule 19 in the place of
rule 6: the neighbour is read block by block at p + m.  int64 throughout; `mr` is the motion range Mr in full-resolution
samples, M = mr // 2.  Vectors are arrays of shape (block rows, block columns, 2) holding (mx, my).  The joint forms (rule
20) take Cb and Cr together; a grain prior changes what luma plane goes in, nothing here.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import denoise_joint_ref as J
from tests import denoise_temporal_ref as TR

BW, BH = 64, 48  # a motion block: the filter's tile


def half(u: np.ndarray) -> np.ndarray:
    """Rule 16: the search plane of a plane."""
    u = np.asarray(u).astype(np.int64)
    H, W = u.shape
    ys, xs = np.arange((H + 1) >> 1), np.arange((W + 1) >> 1)
    y0, y1 = np.minimum(2 * ys, H - 1)[:, None], np.minimum(2 * ys + 1, H - 1)[:, None]
    x0, x1 = np.minimum(2 * xs, W - 1)[None, :], np.minimum(2 * xs + 1, W - 1)[None, :]
    return (u[y0, x0] + u[y0, x1] + u[y1, x0] + u[y1, x1] + 2) >> 2


def key(sad: int, mx: int, my: int, M: int) -> int:
    """Rule 18."""
    return (int(sad) << 21) + ((abs(mx) + abs(my)) << 14) + ((my + M) << 7) + (mx + M)


def search(cur: Sequence[np.ndarray], ref: Sequence[np.ndarray], mr: int) -> np.ndarray:
    """Rules 17 and 18 for the planes `cur` of frame t and `ref` of frame t + k -- one plane each, or (Cb, Cr) whose SADs add
    (rule 20): the vectors (mx, my) = 2 m' of every block, raster order."""
    if isinstance(cur, np.ndarray):
        cur, ref = [cur], [ref]
    M = mr // 2
    hc, hr = [half(p) for p in cur], [half(p) for p in ref]
    h, w = hc[0].shape
    pr = [np.pad(p, M, mode="edge") for p in hr]  # clamp(p' + m') to the search plane's edges
    by, bx = -(-h // (BH // 2)), -(-w // (BW // 2))
    n1 = 2 * M + 1
    cy, cx = np.arange(n1)[:, None], np.arange(n1)[None, :]
    tail = ((np.abs(cx - M) + np.abs(cy - M)) << 14) + (cy << 7) + cx
    out = np.zeros((by, bx, 2), np.int64)
    for j in range(by):
        for i in range(bx):
            ya, yb, xa, xb = j * (BH // 2), min((j + 1) * (BH // 2), h), i * (BW // 2), min((i + 1) * (BW // 2), w)
            sad = np.zeros((n1, n1), np.int64)
            for c, r in zip(hc, pr):
                win = np.lib.stride_tricks.sliding_window_view(r[ya:yb + 2 * M, xa:xb + 2 * M], (yb - ya, xb - xa))
                sad += np.abs(win - c[ya:yb, xa:xb]).sum((2, 3))
            k = int(((sad << 21) + tail).min())
            out[j, i] = 2 * ((k & 127) - M), 2 * (((k >> 7) & 127) - M)
    return out


def _sums_m(us: Sequence[np.ndarray], vs: Sequence[np.ndarray], mv: np.ndarray, A: int, S: int, tab: np.ndarray, q: int, nout: int):
    """Rule 19 (and 11t under it): ([sum w v_n(p + m + d) for the first nout planes], sum w), patches of the planes `us` at p
    against patches of the planes `vs` at p + m + d, m the vector of p's block.  For every distinct vector the sums of the whole
    plane as denoise_temporal_ref._sums forms them, the neighbour read at p + m; a block takes its own vector's."""
    h, w = us[0].shape
    R = A + S
    pad = R + int(np.abs(mv).max(initial=0))
    pu = [np.pad(u, R, mode="edge") for u in us]
    pv = [np.pad(v, pad, mode="edge") for v in vs]
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    nums, den = [np.zeros((h, w), np.int64) for _ in range(nout)], np.zeros((h, w), np.int64)
    k = 2 * S + 1
    for mx, my in sorted({(int(a), int(b)) for a, b in mv.reshape(-1, 2)}):
        n1, d1 = [np.zeros((h, w), np.int64) for _ in range(nout)], np.zeros((h, w), np.int64)
        for dy in range(-A, A + 1):
            for dx in range(-A, A + 1):
                oy, ox = pad + my + dy, pad + mx + dx  # plane sample (0, 0) + m + d in pv
                e = np.zeros((h + 2 * S, w + 2 * S), np.int64)
                for a, b in zip(pu, pv):
                    e += (a[A:A + h + 2 * S, A:A + w + 2 * S] - b[oy - S:oy - S + h + 2 * S, ox - S:ox - S + w + 2 * S]) ** 2
                c = np.zeros((h + 2 * S + 1, w + 2 * S + 1), np.int64)
                c[1:, 1:] = np.cumsum(np.cumsum(e, 0), 1)
                D = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
                wgt = tab[np.minimum(D >> q, 1023)]
                part = (xs + mx + dx >= 0) & (xs + mx + dx < w) & (ys + my + dy >= 0) & (ys + my + dy < h)
                wgt = np.where(part, wgt, 0)
                for n in range(nout):
                    n1[n] += wgt * pv[n][oy:oy + h, ox:ox + w]
                d1 += wgt
        mine = np.repeat(np.repeat((mv[:, :, 0] == mx) & (mv[:, :, 1] == my), BH, 0), BW, 1)[:h, :w]
        for n in range(nout):
            nums[n] += np.where(mine, n1[n], 0)
        den += np.where(mine, d1, 0)
    return nums, den


def sums_plane(planes: Sequence[np.ndarray], t: int, temporal_radius: int, search_radius: int, patch_radius: int, table: np.ndarray, q: int,
               mr: int, vectors: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(numerator without the rounding term, denominator) of rule 7 under rule 19 for frame t of a clip of planes.  vectors:
    {k: the field towards frame t + k}, in the place of search()."""
    tab = np.asarray(table).astype(np.int64)
    u = np.asarray(planes[t]).astype(np.int64)
    num, den = TR._sums(u, None, search_radius, patch_radius, tab, q)
    for k in range(-temporal_radius, temporal_radius + 1):
        if k == 0 or not 0 <= t + k < len(planes):
            continue
        v = np.asarray(planes[t + k]).astype(np.int64)
        if mr == 0:
            n, d = TR._sums(u, v, search_radius, patch_radius, tab, q)
        else:
            mv = vectors[k] if vectors is not None else search(u, v, mr)
            (n,), d = _sums_m([u], [v], mv, search_radius, patch_radius, tab, q, 1)
        num += n
        den += d
    return num, den


def denoise_plane_clip(planes: Sequence[np.ndarray], temporal_radius: int, search_radius: int, patch_radius: int, table: np.ndarray, q: int,
                       mr: int) -> List[np.ndarray]:
    """The same plane of every frame of a clip through rules 1 - 7 with rules 16 - 19."""
    out = []
    for t in range(len(planes)):
        num, den = sums_plane(planes, t, temporal_radius, search_radius, patch_radius, table, q, mr)
        out.append(((num + (den >> 1)) // den).astype(np.asarray(planes[t]).dtype))
    return out


def denoise_chroma_clip(frames: Sequence[Sequence[np.ndarray]], xdec: int, ydec: int, temporal_radius: int, search_radius: int, patch_radius: int,
                        table: np.ndarray, q: int, mr: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """(out_Cb, out_Cr) of every frame under the joint flag (rules 8 - 11t with rules 16 - 20): one vector a chroma tile from
    Cb and Cr, the guide of frame t + k read at the moved place."""
    tab = np.asarray(table).astype(np.int64)
    out = []
    for t in range(len(frames)):
        us = J._triple(frames[t], xdec, ydec)
        nb, nr, den = J._sums(us, None, search_radius, patch_radius, tab, q)
        for k in range(-temporal_radius, temporal_radius + 1):
            if k == 0 or not 0 <= t + k < len(frames):
                continue
            vs = J._triple(frames[t + k], xdec, ydec)
            if mr == 0:
                b, r, d = J._sums(us, vs, search_radius, patch_radius, tab, q)
            else:
                (b, r), d = _sums_m(us, vs, search(us[:2], vs[:2], mr), search_radius, patch_radius, tab, q, 2)
            nb, nr, den = nb + b, nr + r, den + d
        dt = np.asarray(frames[t][1]).dtype
        out.append((((nb + (den >> 1)) // den).astype(dt), ((nr + (den >> 1)) // den).astype(dt)))
    return out


def denoise_clip(frames: Sequence[Sequence[np.ndarray]], xdec: int, ydec: int, temporal_radius: int, search_radius: int, patch_radius: int,
                 luma: Tuple[np.ndarray, int], chroma: Tuple[np.ndarray, int], mr: int, joint: bool = False,
                 curve: Optional[Tuple[np.ndarray, np.ndarray]] = None) -> List[List[np.ndarray]]:
    """A clip, every plane on its own grid.  `chroma` is the (T, q) of the chroma planes: the joint table under `joint`.
    curve = (fwd, inv): luma as rule 14 has it, `luma` then the 12-bit table."""
    ys = [np.asarray(f[0]) for f in frames]
    if curve is not None:
        fwd, inv = (np.asarray(a).astype(np.int64) for a in curve)
        ys = [fwd[np.minimum(y.astype(np.int64), len(fwd) - 1)] for y in ys]
    yo = denoise_plane_clip(ys, temporal_radius, search_radius, patch_radius, *luma, mr)
    if curve is not None:
        yo = [inv[y].astype(np.asarray(frames[0][0]).dtype) for y in yo]
    if len(frames[0]) == 1:
        return [[y] for y in yo]
    if joint:
        cs = denoise_chroma_clip(frames, xdec, ydec, temporal_radius, search_radius, patch_radius, *chroma, mr)
    else:
        cb, cr = (denoise_plane_clip([f[c] for f in frames], temporal_radius, search_radius, patch_radius, *chroma, mr) for c in (1, 2))
        cs = list(zip(cb, cr))
    return [[y, b, r] for y, (b, r) in zip(yo, cs)]
