"""Moving content for the motion tests: frames are windows of a seeded world plane that move by a given vector an interval,
with independent grain on each frame.

* pan():    a uniform pan with a (different) shift in every interval -- catches chained vectors and an off-by-one in k;
* split():  two halves that move in opposite directions, left / right or top / bottom -- catches swapped block indices and
            raster-order mistakes;
* ties():   content of period 4, or constant content, where many candidates have the same SAD.

A frame is a 2-D array; clip(...) makes frames of planes for a chroma format from one world a plane.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np


def dtype_of(bit_depth: int):
    return np.uint8 if bit_depth == 8 else np.uint16


def world(seed, w: int, h: int, bit_depth: int, kind: str = "noise") -> np.ndarray:
    """A plane larger than the frames cut from it.  noise: independent samples over the full range (a block matches at one
    place only); texture: edges, a sine and low-contrast texture of amplitude 6 around mid-grey (the property test's)."""
    rng = np.random.default_rng(seed)
    top = (1 << bit_depth) - 1
    if kind == "noise":
        return rng.integers(0, top + 1, (h, w)).astype(np.int64)
    assert kind == "texture"
    yy, xx = np.mgrid[0:h, 0:w]
    scale = 1 << (bit_depth - 8)
    p = 128.0 + 40.0 * (((xx // 37) + (yy // 29)) & 1) + 20.0 * np.sin(xx / 9.0 + yy / 23.0) + 6.0 * rng.standard_normal((h, w))
    return np.clip(np.rint(p * scale), 0, top).astype(np.int64)


def grain(rng, plane: np.ndarray, sigma: float, bit_depth: int) -> np.ndarray:
    top = (1 << bit_depth) - 1
    if sigma <= 0:
        return plane.astype(dtype_of(bit_depth))
    return np.clip(np.rint(plane + rng.normal(0.0, sigma, plane.shape)), 0, top).astype(dtype_of(bit_depth))


def positions(shifts: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """Where the window stands in each frame: (0, 0), then moved by one shift (sx, sy) an interval."""
    at, out = (0, 0), [(0, 0)]
    for sx, sy in shifts:
        at = (at[0] + sx, at[1] + sy)
        out.append(at)
    return out


def pan(seed, w: int, h: int, bit_depth: int, shifts: Sequence[Tuple[int, int]], sigma: float = 0.0, kind: str = "noise",
        margin: int = 0):
    """(clean frames, grainy frames) of len(shifts) + 1 frames: the window moves by shifts[t] from frame t to frame t + 1, so
    the content moves by -shifts[t]: u_{t+1}(p - shifts[t]) = u_t(p), the vector of frame t towards frame t + 1 is -shifts[t]
    and the one of frame t + 1 towards frame t is +shifts[t]."""
    pos = positions(shifts)
    xs, ys = [p[0] for p in pos], [p[1] for p in pos]
    ox, oy = margin - min(xs), margin - min(ys)
    wd = world(seed, w + max(xs) - min(xs) + 2 * margin, h + max(ys) - min(ys) + 2 * margin, bit_depth, kind)
    rng = np.random.default_rng([int(np.sum(np.asarray(seed))), 77])
    clean = [wd[oy + y:oy + y + h, ox + x:ox + x + w] for x, y in pos]
    return [c.astype(dtype_of(bit_depth)) for c in clean], [grain(rng, c, sigma, bit_depth) for c in clean]


def split(seed, w: int, h: int, bit_depth: int, shift: Tuple[int, int], frames: int = 2, axis: str = "x", sigma: float = 0.0):
    """Grainy frames whose two halves (left / right for axis x at column (w // 128) * 64, top / bottom for y at row
    (h // 96) * 48: a block boundary) move by +shift and -shift an interval."""
    a = pan([seed, 1], w, h, bit_depth, [shift] * (frames - 1), sigma)[1]
    b = pan([seed, 2], w, h, bit_depth, [(-shift[0], -shift[1])] * (frames - 1), sigma)[1]
    out = []
    for p, q in zip(a, b):
        f = p.copy()
        if axis == "x":
            f[:, max(w // 128, 1) * 64:] = q[:, max(w // 128, 1) * 64:]
        else:
            f[max(h // 96, 1) * 48:, :] = q[max(h // 96, 1) * 48:, :]
        out.append(f)
    return out


def ties(w: int, h: int, bit_depth: int, frames: int = 2, period: int = 4) -> List[np.ndarray]:
    """Frames of content with `period` in x and y (period 0: constant), every frame the same: every candidate that is a
    multiple of the period has SAD 0 in the interior, and rule 18 has to pick the zero vector."""
    top = (1 << bit_depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.full((h, w), top // 2) if period == 0 else ((xx % period) * 7 + (yy % period) * 13) * (top // 64)
    return [p.astype(dtype_of(bit_depth)) for _ in range(frames)]


def clip(planes_of_frames: Sequence[Sequence[np.ndarray]]) -> List[List[np.ndarray]]:
    """[plane][frame] -> [frame][plane]"""
    return [list(f) for f in zip(*planes_of_frames)]


def chroma_size(w: int, h: int, ss) -> Tuple[int, int]:
    xdec, ydec = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[ss]
    return (w + xdec) >> xdec, (h + ydec) >> ydec
