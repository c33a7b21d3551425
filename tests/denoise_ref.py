"""The project's non-local-means filter (include/g1s_diff.h, "denoise", rules 1 - 4) restated in numpy.

Integer arithmetic only, so the device's output can be compared byte for byte.  The weight table is an argument: the
tests take it from the library (`grav1synth_amd.denoise.weight_table`), so two `exp` implementations can never show up
as a sample mismatch; `table_from_formula` is the formula itself, for the test of the table.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np


def table_entry(i: int, q: int, bit_depth: int, patch_radius: int, strength: float) -> float:
    """4096 exp(-((i + 1/2) 2^q) / (n h^2 4^(B - 8))), unrounded."""
    n = (2 * patch_radius + 1) ** 2
    x = ((i + 0.5) * 2.0 ** q) / (n * strength * strength * 4.0 ** (bit_depth - 8))
    return 4096.0 * math.exp(-x) if x < 700 else 0.0


def table_from_formula(bit_depth: int, patch_radius: int, strength: float) -> Tuple[np.ndarray, int]:
    """(T, q) of rule 3: T[0] = 4096, T[i] = round(table_entry(i)), q the smallest shift with T[1023] = 0."""
    q = 0
    while math.floor(table_entry(1023, q, bit_depth, patch_radius, strength) + 0.5) != 0:
        q += 1
    t = [4096] + [int(math.floor(table_entry(i, q, bit_depth, patch_radius, strength) + 0.5)) for i in range(1, 1024)]
    return np.array(t, np.uint16), q


def denoise_plane(u: np.ndarray, search_radius: int, patch_radius: int, table: np.ndarray, q: int) -> np.ndarray:
    """One plane through rules 1 - 4 (vectorised: one pass over the plane per offset)."""
    A, S = search_radius, patch_radius
    src = np.asarray(u)
    h, w = src.shape
    u64 = src.astype(np.int64)
    R = A + S
    pad = np.pad(u64, R, mode="edge")  # pad[i, j] = u(clamp(j - R, i - R))
    tab = np.asarray(table).astype(np.int64)
    assert tab.shape == (1024,)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    num = 4096 * u64
    den = np.full((h, w), 4096, np.int64)
    for dy in range(-A, A + 1):
        for dx in range(-A, A + 1):
            if dx == 0 and dy == 0:
                continue
            # squared differences at the coordinates -S .. w + S - 1 (x), -S .. h + S - 1 (y)
            a = pad[A:A + h + 2 * S, A:A + w + 2 * S]
            b = pad[A + dy:A + dy + h + 2 * S, A + dx:A + dx + w + 2 * S]
            e = (a - b) ** 2
            c = np.zeros((h + 2 * S + 1, w + 2 * S + 1), np.int64)
            c[1:, 1:] = np.cumsum(np.cumsum(e, 0), 1)
            k = 2 * S + 1
            D = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]  # (h, w): the patch sum around every sample
            wgt = tab[np.minimum(D >> q, 1023)]
            part = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)  # rule 2: skipped, not clamped
            wgt = np.where(part, wgt, 0)
            num += wgt * pad[R + dy:R + dy + h, R + dx:R + dx + w]
            den += wgt
    assert num.max() + (den.max() >> 1) < 2 ** 32
    return ((num + (den >> 1)) // den).astype(src.dtype)


def denoise_frame(planes: Sequence[np.ndarray], search_radius: int, patch_radius: int, luma: Tuple[np.ndarray, int],
                  chroma: Tuple[np.ndarray, int]) -> List[np.ndarray]:
    """Every plane on its own grid; `luma` / `chroma` are the (T, q) of the two strengths."""
    return [denoise_plane(p, search_radius, patch_radius, *(luma if c == 0 else chroma)) for c, p in enumerate(planes)]
