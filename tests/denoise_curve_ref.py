"""The grain prior of `denoise` (include/g1s_diff.h, rules 12 - 14) restated in numpy: the curve of a table's luma scaling
function, its inverse, and luma through both around the existing restatements (denoise_ref, denoise_temporal_ref,
denoise_joint_ref).  Slow and plain: what the library and the kernels are compared with."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import denoise_joint_ref as J
from tests import denoise_ref as R
from tests import denoise_temporal_ref as TR
from tests import grain_ref as G

STAB_BITS = 12
STAB_TOP = (1 << STAB_BITS) - 1


def max_range(bit_depth: int) -> int:
    return 1 << (STAB_BITS - bit_depth)


def scaling(points_per_segment: Sequence[Sequence[Tuple[int, int]]], bit_depth: int) -> np.ndarray:
    """Rule 12's s(v), v = 0 .. M: the rounded unweighted mean of the segments' scale_lut over their luma ScalingLut."""
    n = len(points_per_segment)
    v = np.arange(1 << bit_depth, dtype=np.int64)
    total = np.zeros(1 << bit_depth, np.int64)
    for pts in points_per_segment:
        total += G.scale_lut(G.scaling_lut([tuple(p) for p in pts]), v, bit_depth)
    return (total + (n >> 1)) // n


def curve(points_per_segment: Sequence[Sequence[Tuple[int, int]]], bit_depth: int, rng: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(f, g) of rules 12 and 13 in Python integers."""
    assert bit_depth in (8, 10) and len(points_per_segment) >= 1 and 0 <= rng <= max_range(bit_depth)
    M = (1 << bit_depth) - 1
    R_ = rng if rng else min(4, max_range(bit_depth))
    s = [int(x) for x in scaling(points_per_segment, bit_depth)]
    floor = max(1, -(-max(s) // R_))
    C = [0]
    for v in range(M + 1):
        C.append(C[-1] + (1 << 24) // max(s[v], floor))
    CM = C[M]
    f = [(STAB_TOP * C[x] + (CM >> 1)) // CM for x in range(M + 1)]
    g = []
    for y in range(STAB_TOP + 1):
        if bit_depth == 8:
            g.append(min(range(M + 1), key=lambda x: (abs(f[x] - y), x)))
            continue
        # (the same without the search over every x: f increases, so the nearest is one of the two around y)
        hi = int(np.searchsorted(f, y, side="left"))  # first x with f(x) >= y
        g.append(min((x for x in (hi - 1, hi) if 0 <= x <= M), key=lambda x: (abs(f[x] - y), x)))
    return np.array(f, np.uint16), np.array(g, np.uint16)


def forward(u: np.ndarray, fwd: np.ndarray) -> np.ndarray:
    """Rule 14's u' = f[min(u, M)] as a 12-bit u16 plane."""
    return fwd[np.minimum(u.astype(np.int64), len(fwd) - 1)].astype(np.uint16)


def luma_table(patch_radius: int, strength: float) -> Tuple[np.ndarray, int]:
    """Rule 14's table: rule 3 at B = 12 with the luma strength."""
    return R.table_from_formula(STAB_BITS, patch_radius, strength)


def denoise_luma(u: np.ndarray, fwd: np.ndarray, inv: np.ndarray, search_radius: int, patch_radius: int, strength: float) -> np.ndarray:
    """One luma plane through rule 14 (rules 1 - 4 in the stabilised domain)."""
    T, q = luma_table(patch_radius, strength)
    v = R.denoise_plane(forward(u, fwd), search_radius, patch_radius, T, q)
    return inv[v].astype(u.dtype)


def denoise_luma_clip(planes: Sequence[np.ndarray], fwd: np.ndarray, inv: np.ndarray, temporal_radius: int, search_radius: int, patch_radius: int,
                      strength: float) -> List[np.ndarray]:
    """The luma planes of a clip through rule 14 (rules 1 - 7 in the stabilised domain)."""
    T, q = luma_table(patch_radius, strength)
    vs = TR.denoise_plane_clip([forward(u, fwd) for u in planes], temporal_radius, search_radius, patch_radius, T, q)
    return [inv[v].astype(u.dtype) for v, u in zip(vs, planes)]


def denoise_clip(frames: Sequence[Sequence[np.ndarray]], bit_depth: int, fwd: np.ndarray, inv: np.ndarray, xdec: int, ydec: int, temporal_radius: int,
                 search_radius: int, patch_radius: int, strength: float, chroma_strength: Optional[float] = None, joint: bool = False) -> List[List[np.ndarray]]:
    """A clip under a curve: luma by rule 14, chroma (rule 15) as the restatements without a curve make it -- independently
    with rule 3's table, or jointly with rule 10's and the unstabilised input luma as the guide."""
    hc = strength if chroma_strength is None else chroma_strength
    luma = denoise_luma_clip([f[0] for f in frames], fwd, inv, temporal_radius, search_radius, patch_radius, strength)
    if len(frames[0]) == 1:
        return [[y] for y in luma]
    tl, tc = R.table_from_formula(bit_depth, patch_radius, strength), R.table_from_formula(bit_depth, patch_radius, hc)
    if joint:
        plain = J.denoise_clip(frames, xdec, ydec, temporal_radius, search_radius, patch_radius, tl, J.joint_table_from_formula(bit_depth, patch_radius, hc))
    else:
        plain = TR.denoise_clip(frames, temporal_radius, search_radius, patch_radius, tl, tc)
    return [[y, p[1], p[2]] for y, p in zip(luma, plain)]


# ---------------------------------------------------------------------------------------------- the demonstration's content
def band_content(seed: int = 5):
    """10-bit, 192 x 96: three 64-column bands at 140 / 480 / 860 with the texture 10 sin(0.9 x) sin(0.7 y) + 14 ((y // 12) % 2),
    and Gaussian grain of sigma(v) = s(v) / 5, s(v) = round(20 + 60 v / 1023).  Returns (clean, noisy, the prior's points)."""
    h, w = 96, 192
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    level = np.repeat(np.array([140.0, 480.0, 860.0]), 64)[None, :]
    clean = level + 10.0 * np.sin(0.9 * x) * np.sin(0.7 * y) + 14.0 * ((y // 12) % 2)
    sigma = np.round(20.0 + 60.0 * clean / 1023.0) / 5.0
    noisy = clean + np.random.default_rng(seed).normal(0.0, 1.0, (h, w)) * sigma
    to_u16 = lambda p: np.clip(np.round(p), 0, 1023).astype(np.uint16)
    return to_u16(clean), to_u16(noisy), [(0, 20), (255, 80)]
