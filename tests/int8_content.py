"""Frame pairs whose RESIDUAL is designed sample by sample (test infrastructure): the int8 edge of the accumulation chains.

The accumulation kernels multiply a residual d = narrowed source - narrowed denoised on the matrix cores only if it lies in
-128 .. 127, and the chroma regressor L (the sum of the 1, 2 or 4 luma residuals under a chroma sample) likewise; everything else
goes to the exact kernel.  tests/content.py's noise is a few code values and its damage is far outside int8, so no sample of it sits
at -129, -128, 127 or 128.  Here the narrowed source is a constant (127: with it both -128 and 127 are reachable, the denoised
sample being 255 or 0) and the narrowed denoised sample is source - d for a field d the caller designs per plane; for a d of -129
or 128 the source of that one sample moves to 126 or 128.  A constant source is flat to the finder, block by block, whatever d is
(the finder reads the source alone) -- the oracle's mask is still the truth, tests/test_int8_content_cpu.py holds what it gives.

Above 8 bits both planes get independent random bits below their narrowing shift: the kernels mask them away and the oracle
truncates them, neither rounds.  Source and denoised may differ in depth.

Integer arithmetic on numpy only; deterministic from the arguments.  The planes come in tests.content.make_frames' layout: lists
of C-contiguous 2-D arrays, uint8 for 8-bit and uint16 above."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

SOURCE = 127
D_MIN, D_MAX = -129, 128  # what a field may hold: one past int8 on either side (a source of 126 / 128 reaches them)


def make_frames(residuals: Sequence[np.ndarray], src_bd: int, den_bd: int, frame: int, seed: int = 1,
                source: int = SOURCE) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """(source_planes, denoised_planes), one pair per array of `residuals` (1: luma only, 3: Y, Cb, Cr at their own sizes).  The
    narrowed planes are exactly source' and source' - d, source' = `source` moved into [d, 255 + d] where d asks for it."""
    src, den = [], []
    for c, d in enumerate(residuals):
        d = np.asarray(d, np.int64)
        if d.min() < -255 or d.max() > 255:
            raise ValueError(f"plane {c}: residuals of {d.min()} .. {d.max()} are not differences of 8-bit samples")
        s8 = np.clip(np.full(d.shape, source, np.int64), np.maximum(d, 0), 255 + np.minimum(d, 0))
        v8 = s8 - d
        assert v8.min() >= 0 and v8.max() <= 255
        for k, (p8, bd, out) in enumerate(((s8, src_bd, src), (v8, den_bd, den))):
            up = bd - 8
            low = np.random.default_rng([seed, frame, 16 + 2 * c + k]).integers(0, 1 << up, d.shape) if up else 0
            out.append(np.ascontiguousarray(((p8 << up) | low).astype(np.uint8 if bd == 8 else np.uint16)))
    return src, den


def narrowed_residuals(src: Sequence[np.ndarray], den: Sequence[np.ndarray], src_bd: int, den_bd: int) -> List[np.ndarray]:
    """The residual as the oracle forms it (truncating shifts), from the planes."""
    return [(s.astype(np.int64) >> (src_bd - 8)) - (v.astype(np.int64) >> (den_bd - 8)) for s, v in zip(src, den)]


def luma_sums(d: np.ndarray, xdec: int, ydec: int) -> np.ndarray:
    """L at chroma resolution: the sum of the luma residuals under each chroma sample ((h >> ydec) x (w >> xdec))."""
    h, w = d.shape[0] >> ydec, d.shape[1] >> xdec
    d = np.asarray(d, np.int64)[:h << ydec, :w << xdec]
    return d.reshape(h, 1 << ydec, w, 1 << xdec).sum(axis=(1, 3))


# ---- residual fields ----------------------------------------------------------------------------------------------------------

def benign(shape, rng) -> np.ndarray:
    """|d| <= 3, independent: what lies around a poke."""
    return rng.integers(-3, 4, shape).astype(np.int64)


def extremes(shape, rng) -> np.ndarray:
    """Every sample -128 or 127, drawn at random (a well-conditioned system; a constant field is singular)."""
    return np.where(rng.integers(0, 2, shape) != 0, 127, -128).astype(np.int64)


def quads_inside(shape, rng, xdec: int = 1, ydec: int = 1) -> np.ndarray:
    """Luma under a chroma plane at the bound: every group of samples under a chroma sample (2 x 2; a pair for 4:2:2; the sample
    itself for 4:4:4) holds as many 127 as -128 in a random arrangement (4:4:4: either), so L stays inside int8 -- -2, -1 -- while
    every luma residual is extreme.  Samples of a cut last row or column, under no chroma sample, are drawn like `extremes`."""
    h, w = shape
    n = (1 << xdec) * (1 << ydec)
    out = extremes(shape, rng)
    if n == 1:
        return out
    gh, gw = h >> ydec, w >> xdec
    order = np.argsort(rng.random((gh, gw, n)), axis=2)  # a random permutation a group: its first half takes 127
    vals = np.where(order < n // 2, 127, -128).astype(np.int64)
    out[:gh << ydec, :gw << xdec] = vals.reshape(gh, gw, 1 << ydec, 1 << xdec).transpose(0, 2, 1, 3).reshape(gh << ydec, gw << xdec)
    return out


def poke(d: np.ndarray, y: int, x: int, value: int) -> None:
    if not D_MIN <= value <= D_MAX:
        raise ValueError(f"a poke of {value}")
    d[y, x] = value


def fill_unit(d: np.ndarray, by: int, cell: int, value: int, unit_w: int = 128, block_h: int = 32) -> None:
    """One whole unit (`unit_w` samples of block row `by`, `block_h` rows) at `value`: the block statistics' packed sums at an end."""
    d[by * block_h:(by + 1) * block_h, cell * unit_w:(cell + 1) * unit_w] = value


# what the luma residuals under one chroma sample are set to, by the L asked for and the samples under it (row-major)
L_MEMBERS = {
    4: {127: (32, 32, 32, 31), 128: (32, 32, 32, 32), -128: (-32, -32, -32, -32), -129: (-32, -32, -32, -33)},
    2: {127: (64, 63), 128: (64, 64), -128: (-64, -64), -129: (-64, -65)},
    1: {127: (127,), 128: (128,), -128: (-128,), -129: (-129,)},
}


def set_L(d: np.ndarray, cy: int, cx: int, value: int, xdec: int, ydec: int) -> None:
    """The luma residuals under chroma sample (cy, cx) so that their sum is `value` (127, 128, -128 or -129), every one of them
    well inside int8 (but at 4:4:4, where L is the residual itself)."""
    m = np.array(L_MEMBERS[(1 << xdec) * (1 << ydec)][value], np.int64).reshape(1 << ydec, 1 << xdec)
    d[cy << ydec:(cy + 1) << ydec, cx << xdec:(cx + 1) << xdec] = m
