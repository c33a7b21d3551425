"""Coarse levels (include/g1s_diff.h, "denoise", rules 25 - 29) restated in numpy.

coarse_frame() is rule 25, merge() rule 27, denoise_clip() rule 26: the filter of rules 1 - 24 as tests/denoise_motion_ref.py
and tests/denoise_gain_ref.py restate it (imported, not copied), on the frames and on their coarse frames, with the tables
g1s_denoise_weights gives for the strengths of each level (level l's are rho times level l - 1's, a double product level by
level).  int64 throughout.  `wrong`: names of rules restated wrongly on purpose, for the tests that show a pass on the device
means something.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import denoise_gain_ref as G
from tests import denoise_joint_ref as J
from tests import denoise_motion_ref as M

WRONG = ("nearest", "trunc", "mirror", "noclip", "coarse_from_output", "merge_before_inverse", "mr_not_halved", "no_rho", "fine_guide")


def coarse_frame(frame: Sequence[np.ndarray]) -> List[np.ndarray]:
    """Rule 25: every plane through rule 16's box."""
    return [M.half(p).astype(np.asarray(p).dtype) for p in frame]


def coarse_motion_range(mr: int) -> int:
    """Rule 26: Mr' = 2 ceil(Mr / 4)."""
    return 2 * ((mr + 3) // 4)


def strengths(h: float, hc: float, K: int, rho: float) -> List[Tuple[float, float]]:
    """(h, hc) of levels 0 .. K."""
    out = [(float(h), float(hc))]
    for _ in range(K):
        out.append((float(rho) * out[-1][0], float(rho) * out[-1][1]))
    return out


def merge(v: np.ndarray, c: np.ndarray, bit_depth: int, wrong: Sequence[str] = (), top: Optional[int] = None) -> np.ndarray:
    """Rule 27 for one plane: v the full-resolution output, c the coarse level's.  int64 out (the caller casts)."""
    v, c = np.asarray(v).astype(np.int64), np.asarray(c).astype(np.int64)
    H, W = v.shape
    d = c - M.half(v)
    Hc, Wc = d.shape
    assert (Hc, Wc) == ((H + 1) >> 1, (W + 1) >> 1)

    def pair(n, nc):
        x = np.arange(n)
        a = x >> 1
        b = a + np.where(x & 1, 1, -1)
        if "mirror" in wrong:
            b = np.where(b < 0, np.minimum(a + 1, nc - 1), np.where(b > nc - 1, np.maximum(a - 1, 0), b))
        return a, np.clip(b, 0, nc - 1)

    xa, xb = pair(W, Wc)
    ya, yb = pair(H, Hc)
    if "nearest" in wrong:
        U = d[ya[:, None], xa[None, :]]
    else:
        s = 9 * d[ya[:, None], xa[None, :]] + 3 * d[ya[:, None], xb[None, :]] + 3 * d[yb[:, None], xa[None, :]] + d[yb[:, None], xb[None, :]] + 8
        U = np.sign(s) * (np.abs(s) >> 4) if "trunc" in wrong else s >> 4
    out = v + U
    return out if "noclip" in wrong else np.clip(out, 0, ((1 << bit_depth) - 1) if top is None else top)


def merge_loop(v: np.ndarray, c: np.ndarray, bit_depth: int) -> np.ndarray:
    """Rule 27 as a plain double loop, one Python integer at a time."""
    H, W = v.shape
    Hc, Wc = (H + 1) >> 1, (W + 1) >> 1

    def box(x, y):
        x0, x1, y0, y1 = min(2 * x, W - 1), min(2 * x + 1, W - 1), min(2 * y, H - 1), min(2 * y + 1, H - 1)
        return (int(v[y0, x0]) + int(v[y0, x1]) + int(v[y1, x0]) + int(v[y1, x1]) + 2) >> 2

    d = [[int(c[y, x]) - box(x, y) for x in range(Wc)] for y in range(Hc)]
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            xa, ya = x >> 1, y >> 1
            xb = min(max(xa + (1 if x & 1 else -1), 0), Wc - 1)
            yb = min(max(ya + (1 if y & 1 else -1), 0), Hc - 1)
            U = (9 * d[ya][xa] + 3 * d[ya][xb] + 3 * d[yb][xa] + d[yb][xb] + 8) >> 4  # (>> of a negative Python int floors)
            out[y, x] = min(max(int(v[y, x]) + U, 0), (1 << bit_depth) - 1)
    return out


def _tables(bit_depth: int, S: int, h: float, hc: float, joint: bool, curve):
    from grav1synth_amd.denoise import weight_table

    return weight_table(12 if curve is not None else bit_depth, S, h), weight_table(bit_depth, S, hc, joint_chroma=joint)


def level0(frames, xdec, ydec, bit_depth, h, hc, A, S, D, mr, joint, gain, curve, guide_of=None):
    """F_0: rules 1 - 24.  guide_of (a wrong restatement): the frames whose guide, through the box, the chroma filter is to take
    in the place of the guide of `frames`."""
    luma, chroma = _tables(bit_depth, S, h, hc, joint, curve)
    if gain is not None:
        assert guide_of is None
        return G.denoise_clip(frames, xdec, ydec, D, A, S, luma, chroma, gain, bit_depth, mr, curve)
    out = M.denoise_clip(frames, xdec, ydec, D, A, S, luma, chroma, mr, joint, curve)
    if guide_of is not None and joint and len(frames[0]) == 3:
        fake = [[M.half(J.guide(g[0], xdec, ydec)), f[1], f[2]] for f, g in zip(frames, guide_of)]  # (read at 4:4:4: the guide as given)
        cs = M.denoise_chroma_clip(fake, 0, 0, D, A, S, *chroma, mr)
        out = [[o[0], cb, cr] for o, (cb, cr) in zip(out, cs)]
    return out


def denoise_clip(frames: Sequence[Sequence[np.ndarray]], xdec: int, ydec: int, bit_depth: int, *, K: int = 0, rho: float = 1.0, h: float = 4.0,
                 hc: Optional[float] = None, A: int = 3, S: int = 2, D: int = 0, mr: int = 0, joint: bool = False, gain=None, curve=None,
                 wrong: Sequence[str] = (), _guide_of=None) -> List[List[np.ndarray]]:
    """F_K of rule 26 on a clip of frames (lists of planes)."""
    assert all(w in WRONG for w in wrong), wrong
    hc = h if hc is None else hc
    frames = [[np.asarray(p) for p in f] for f in frames]
    if K and "merge_before_inverse" in wrong:
        return _merge_before_inverse(frames, bit_depth, K, rho, h, A, S, D, mr, curve)
    fine = level0(frames, xdec, ydec, bit_depth, h, hc, A, S, D, mr, joint, gain, curve, _guide_of)
    if K == 0:
        return fine
    r = 1.0 if "no_rho" in wrong else float(rho)
    cf = [coarse_frame(f) for f in (fine if "coarse_from_output" in wrong else frames)]
    coarse = denoise_clip(cf, xdec, ydec, bit_depth, K=K - 1, rho=rho, h=r * h, hc=r * hc, A=A, S=S, D=D,
                          mr=mr if "mr_not_halved" in wrong else coarse_motion_range(mr), joint=joint, gain=gain, curve=curve, wrong=wrong,
                          _guide_of=frames if "fine_guide" in wrong else None)
    return [[merge(v, c, bit_depth, wrong).astype(v.dtype if "noclip" not in wrong else np.int64) for v, c in zip(fv, fc)] for fv, fc in zip(fine, coarse)]


def _merge_before_inverse(frames, bit_depth, K, rho, h, A, S, D, mr, curve):
    """A wrong restatement for luma-only clips with a curve and K = 1: the merge in the stabilised domain, the inverse after it."""
    from grav1synth_amd.denoise import weight_table

    assert K == 1 and curve is not None and len(frames[0]) == 1
    fwd, inv = (np.asarray(a).astype(np.int64) for a in curve)
    stab = lambda ys: [fwd[np.minimum(y.astype(np.int64), len(fwd) - 1)] for y in ys]  # noqa: E731
    ys = [f[0] for f in frames]
    fine = M.denoise_plane_clip(stab(ys), D, A, S, *weight_table(12, S, h), mr)
    coarse = M.denoise_plane_clip(stab([M.half(y) for y in ys]), D, A, S, *weight_table(12, S, float(rho) * h), coarse_motion_range(mr))
    return [[inv[merge(v, c, 12)].astype(ys[0].dtype)] for v, c in zip(fine, coarse)]
