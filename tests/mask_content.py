"""Frame pairs whose flat-block mask is designed block by block (test infrastructure).

The accumulation kernels decide per flat block, from whether its left, right and upper neighbour is flat and from where it sits
in its unit (4 luma / 8 chroma blocks in the wide chain, 2 in the stream chain): the observation window, the fast path, where a
unit's halo words come from, what is deferred beside what.  tests/content.py's kinds give rectangles of flat blocks, in which
nearly every flat block has three flat neighbours.  Here the `flat` frame of tests/content.py -- its ramps, gain laws, taps,
luma-into-chroma weights and noise, by import -- gets the checker texture on exactly the samples of the blocks a design marks 0.
The finder works per block (gradient covariance, variance, a top-10 % rule over the frame's scores), so the mask it gives is the
design but for a few designed-flat blocks it rejects, and, where a design has fewer than a tenth of its blocks flat, for textured
blocks the percentile rule flags with value 1.  The oracle's mask is the truth, never the design; tests/test_mask_content_cpu.py
holds what the masks of the committed design lists reach.

Integer arithmetic on numpy only; deterministic from the arguments."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from tests import content

BLOCK = 32
DAMAGE_PERIOD = 3  # of every three 4-block cells along a block row one takes damage (see _confine)


def damaged_cells(nbh: int, nbw: int, frame: int) -> np.ndarray:
    """(nbh, nbw) bool: the luma blocks of the 4-block cells that keep their damage in frame `frame`.  Along a block row the
    cells left and right of such a cell never do, and the pattern moves a cell from row to row and from frame to frame."""
    by, bx = np.arange(nbh)[:, None], np.arange(nbw)[None, :]
    return ((bx >> 2) + by + frame) % DAMAGE_PERIOD == 0


def _confine(before: np.ndarray, after: np.ndarray, keep: np.ndarray, bw: int, bh: int) -> None:
    """Undo, in place, what `after` changed against `before` outside the blocks (bh x bw samples) marked in `keep`."""
    h, w = after.shape
    k = np.repeat(np.repeat(keep, bh, axis=0), bw, axis=1)[:h, :w]
    after[~k] = before[~k]


def make_frames(design: np.ndarray, width: int, height: int, bit_depth: int, xdec: int, ydec: int, frame: int, seed: int = 1,
                damage: bool = False) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """(source_planes, denoised_planes) in tests.content.make_frames' layout.  `design`: (nbh, nbw) of 0 / 1 over the 32 x 32
    luma block grid, 1 asks for a flat block; the texture lies on exactly the samples of the blocks marked 0.

    damage: content._damage on the denoised planes (|source - denoised| > 127: the block's unit is deferred), kept only inside
    damaged_cells -- all over the frame it leaves hardly a 4-block unit whole, and the point here is a deferred unit beside units
    that are still multiplied."""
    nbh, nbw = (height + BLOCK - 1) // BLOCK, (width + BLOCK - 1) // BLOCK
    design = np.asarray(design)
    if design.shape != (nbh, nbw) or not np.isin(design, (0, 1)).all():
        raise ValueError(f"design: want 0 / 1 of shape {(nbh, nbw)}, got shape {design.shape}")
    tex = np.repeat(np.repeat(design == 0, BLOCK, axis=0), BLOCK, axis=1)[:height, :width]
    src, den = content.textured_frames(tex, width, height, bit_depth, xdec, ydec, frame, seed)
    if damage:
        keep = damaged_cells(nbh, nbw, frame)
        for c in range(3):
            before = den[c].copy()
            content._damage(np.random.default_rng([seed, frame, 8 + c]), src[c], den[c], bit_depth - 8)
            _confine(before, den[c], keep, BLOCK >> (xdec if c else 0), BLOCK >> (ydec if c else 0))
    return src, den


def _straddle(by, bx, unit: int):
    """Pairs of flat blocks across the boundaries between units of `unit` blocks, nothing else in either unit: a block row takes
    every second boundary, the next row the others."""
    cell = bx // unit
    last = (bx % unit == unit - 1) & ((cell + by) % 2 == 0) & ((cell + 1) * unit < bx.max() + 1)
    first = (bx % unit == 0) & ((cell - 1 + by) % 2 == 0) & (cell > 0)
    return last | first


def designs(nbh: int, nbw: int) -> Dict[str, np.ndarray]:
    """name -> (nbh, nbw) uint8 design, in a fixed order; the random ones are seeded by the grid's size."""
    by, bx = np.arange(nbh)[:, None], np.arange(nbw)[None, :]

    def rand(p, s):
        return np.random.default_rng([nbh, nbw, s]).random((nbh, nbw)) < p

    out = {
        # every flat block isolated: left, right and up not flat
        "checker0": (bx + by) % 2 == 0,
        "checker1": (bx + by) % 2 == 1,
        # up flat, left and right not
        "cols2": (bx % 2 == 1) | (by < 0),
        "cols3": (bx % 3 == 0) | (by < 0),
        # left and right flat, up not
        "rows2": (by % 2 == 1) | (bx < 0),
        # a list neighbour that is a spatial neighbour through one block only
        "straddle4": _straddle(by, bx, 4),
        # (every fourth row flat: with the pairs alone under a tenth of the blocks are flat, and the percentile rule then flags
        #  textured blocks inside the pairs' units)
        "straddle8": _straddle(by, bx, 8) | (by % 4 == 3),
        # one flat block a unit, at each position in turn down the rows
        "single4": bx % 4 == by % 4,
        "single8": bx % 8 == by % 8,
        "stairs": (bx - by) % 3 == 0,
        # whole 8-block units, every second one: full units beside empty ones, a list neighbour two units away
        "cells8": ((bx >> 3) + by) % 2 == 0,
        # columns in pairs: up flat, and one of left and right
        "colpairs": (bx % 3 != 2) | (by < 0),
        # pairs along every second row, a block further on each time: up not flat, and one of left and right, in every column
        "rowpairs": (by % 2 == 1) & ((bx + by // 2) % 3 != 2),
        "rand25": rand(0.25, 25),
        "rand50a": rand(0.5, 50),
        "rand50b": rand(0.5, 51),
        "rand85": rand(0.85, 85),    # holes in a flat field
        "sparse": rand(0.06, 6),     # under a tenth flat: the percentile rule flags textured blocks (mask value 1)
    }
    return {k: np.ascontiguousarray(np.broadcast_to(v, (nbh, nbw)).astype(np.uint8)) for k, v in out.items()}
