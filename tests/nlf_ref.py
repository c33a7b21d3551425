"""Noise levels restated in numpy (test infrastructure): rules N1 - N8 of include/g1s_diff.h, the curve of rules 12 - 13
from a given scaling function, and the report text.

Imports nothing from the product package.  Records are dicts of numpy arrays: n, a, q, each (3, 32) uint64.  Everything
that could leave 64 bits is formed in Python integers."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

BINS = 32
EDGE_THRESHOLD = 50
SQRT_PI_BY_2 = 1.2533141373155003
DEFAULT_MIN_COUNT = 4096
NAMES = ("n", "a", "q")


def empty_record() -> dict:
    return {name: np.zeros((3, BINS), np.uint64) for name in NAMES}


def stencil(plane: np.ndarray):
    """N1 on the interior of a plane: (Gx, Gy, L, S9), each (ph - 2, pw - 2) int64; None when the interior is empty."""
    u = np.asarray(plane).astype(np.int64)
    ph, pw = u.shape
    if ph < 3 or pw < 3:
        return None
    m = [[u[i:ph - 2 + i, j:pw - 2 + j] for j in range(3)] for i in range(3)]
    gx = (m[0][0] - m[0][2]) + (m[2][0] - m[2][2]) + 2 * (m[1][0] - m[1][2])
    gy = (m[0][0] - m[2][0]) + (m[0][2] - m[2][2]) + 2 * (m[0][1] - m[2][1])
    lap = 4 * m[1][1] - 2 * (m[0][1] + m[2][1] + m[1][0] + m[1][2]) + (m[0][0] + m[0][2] + m[2][0] + m[2][2])
    s9 = sum(m[i][j] for i in range(3) for j in range(3))
    return gx, gy, lap, s9


def chroma_bins(luma: np.ndarray, ph: int, pw: int, bit_depth: int, xdec: int, ydec: int) -> np.ndarray:
    """N2 for chroma: `measure`'s rule 2 on the frame's own luma, for every sample of a ph x pw chroma plane."""
    y = np.asarray(luma).astype(np.int64)
    _h, w = y.shape
    ys = (np.arange(ph) << ydec)[:, None]
    xs = (np.arange(pw) << xdec)[None, :]
    I = (y[ys, xs] + y[ys, np.minimum(xs + 1, w - 1)] + 1) >> 1 if xdec else y[ys, xs]
    return I >> (bit_depth - 5)


def nlf_frame(planes: Sequence[np.ndarray], bit_depth: int, xdec: int = 1, ydec: int = 1) -> dict:
    """N1 - N4 on one frame: planes = [Y] or [Y, U, V]."""
    sh = bit_depth - 8
    half = (1 << (sh - 1)) if sh else 0
    rec = empty_record()
    for c, plane in enumerate(planes):
        st = stencil(plane)
        if st is None:
            continue
        gx, gy, lap, s9 = st
        counts = ((np.abs(gx) + np.abs(gy) + half) >> sh) < EDGE_THRESHOLD
        if c == 0:
            k = s9 // (9 << (bit_depth - 5))
        else:
            ph, pw = np.asarray(plane).shape
            k = chroma_bins(planes[0], ph, pw, bit_depth, xdec, ydec)[1:-1, 1:-1]
        k, al = k[counts], np.abs(lap[counts])
        rec["n"][c] = np.bincount(k, minlength=BINS).astype(np.uint64)
        a = np.zeros(BINS, np.int64)
        np.add.at(a, k, (al + half) >> sh)
        rec["a"][c] = a.astype(np.uint64)
        # L^2 < 2^32 and a plane has fewer than 2^31 samples here: the sum of a bin stays inside uint64
        q = np.zeros(BINS, np.uint64)
        np.add.at(q, k, (al * al).astype(np.uint64))
        rec["q"][c] = q
    return rec


def sum_records(records: Sequence[dict]) -> dict:
    """N4; an overflow of 64 bits raises OverflowError."""
    total = empty_record()
    for name in NAMES:
        flat = [sum(int(rec[name].ravel()[j]) for rec in records) for j in range(total[name].size)]
        if any(v > 2 ** 64 - 1 for v in flat):
            raise OverflowError(name)
        total[name] = np.array(flat, np.uint64).reshape(3, BINS)
    return total


def levels(total: dict, min_count: int = 0) -> List[Optional[int]]:
    """N5: t[k] for the luma bins, None where n < Nmin."""
    nmin = min_count or DEFAULT_MIN_COUNT
    out: List[Optional[int]] = []
    for k in range(BINS):
        n, q = int(total["n"][0, k]), int(total["q"][0, k])
        out.append(math.isqrt((q << 16) // (36 * n)) if n >= nmin else None)
    return out


def sigma(total: dict, bit_depth: int, min_count: int = 0) -> np.ndarray:
    """N6: s[1 << B] (uint8); ValueError with the refusal's text where the rule refuses."""
    if bit_depth == 12:
        raise ValueError("a grain prior needs headroom above the clip's bit depth: the stabilised domain is 12 bits, so a 12-bit clip is refused")
    if bit_depth not in (8, 10):
        raise ValueError("a grain prior is defined for bit depths 8 and 10")
    t = levels(total, min_count)
    valid = [k for k in range(BINS) if t[k] is not None]
    if not valid:
        raise ValueError("no luma bin has enough smooth samples for a prior")
    tmax = max(t[k] for k in valid)
    y = [max(1, 255 * t[k] // max(tmax, 1)) for k in valid]
    c = [(k << (bit_depth - 5)) + (1 << (bit_depth - 6)) for k in valid]
    s = np.zeros(1 << bit_depth, np.uint8)
    for v in range(1 << bit_depth):
        if v <= c[0]:
            s[v] = y[0]
        elif v >= c[-1]:
            s[v] = y[-1]
        else:
            i = max(j for j in range(len(c)) if c[j] <= v)
            s[v] = y[i] + ((y[i + 1] - y[i]) * (v - c[i]) * 2 + (c[i + 1] - c[i])) // (2 * (c[i + 1] - c[i]))  # (// floors)
    return s


def curve_from_s(s: Sequence[int], bit_depth: int, range_: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Rule 12 from "floor = ..." onwards and rule 13 of `denoise`, on s[1 << B]: (fwd, inv) as uint16."""
    rmax = 1 << (12 - bit_depth)
    R = range_ or min(4, rmax)
    M = (1 << bit_depth) - 1
    s = [int(v) for v in s]
    top = max(s)
    floor = max(1, -(-top // R))
    C = [0]
    for v in range(M + 1):
        C.append(C[-1] + (1 << 24) // max(s[v], floor))
    CM = C[M]
    fwd = [(4095 * C[x] + (CM >> 1)) // CM for x in range(M + 1)]
    # rule 13: the smallest x with |f(x) - y| minimal; f is strictly increasing from 0, so it is one of the two around y
    f = np.array(fwd)
    assert f[0] == 0 and f[M] == 4095 and (np.diff(f) > 0).all()
    inv = []
    for yv in range(4096):
        j = int(np.searchsorted(f, yv, side="right")) - 1  # f[j] <= yv < f[j + 1], or j = M
        inv.append(j + 1 if j < M and f[j + 1] - yv < yv - f[j] else j)
    return np.array(fwd, np.uint16), np.array(inv, np.uint16)


def strength(total: dict, bit_depth: int, min_count: int = 0, plane_class: int = 0) -> Optional[float]:
    """N7 for a plane class (0 luma, 1 the chroma planes pooled): h, or None where the rule refuses."""
    planes = (1, 2) if plane_class else (0,)
    Q = sum(int(total["q"][c, k]) for c in planes for k in range(BINS))
    N = sum(int(total["n"][c, k]) for c in planes for k in range(BINS))
    if N < (min_count or DEFAULT_MIN_COUNT):
        return None
    h = math.sqrt((2.0 * float(Q)) / (36.0 * float(N))) / float(1 << (bit_depth - 8))
    return h if 0.0 < h <= 1000.0 else None


def _fmt(defined: bool, v: float) -> str:
    return "%.4f" % v if defined else "-"


def format_noise_levels(total: dict, frames: int, bit_depth: int, nplanes: int = 3, min_count: int = 0) -> bytes:
    """N8 (the grammar is in include/g1s_diff.h): every value one f64 operation after the other, as the library."""
    out = ["noiselevels1", f"frames {frames} bit_depth {bit_depth} planes {nplanes}"]
    scale = float(1 << (bit_depth - 8))
    for c in range(nplanes):
        out.append(f"plane {c}")
        Q = N = 0
        for k in range(BINS):
            n, a, q = (int(total[name][c, k]) for name in NAMES)
            if not n:
                continue
            Q, N = Q + q, N + n
            sq = math.sqrt(float(q) / float(36 * n))
            sa = float(a) / float(6 * n) * SQRT_PI_BY_2 * scale
            out.append(f"bin {k} {n} {_fmt(True, sq)} {_fmt(True, sa)}")
        out.append("plane_sigma " + _fmt(N != 0, math.sqrt(float(Q) / float(36 * N)) if N else 0.0))
    hl, hc = strength(total, bit_depth, min_count, 0), strength(total, bit_depth, min_count, 1)
    out.append(f"auto_strength {_fmt(hl is not None, hl or 0.0)} {_fmt(hc is not None, hc or 0.0)}")
    return ("\n".join(out) + "\n").encode()


def to_struct(rec: dict, dtype) -> np.ndarray:
    """The record as an entry of the library's structured dtype (handed in by the caller: this module does not know it)."""
    out = np.zeros((), dtype)
    for name in NAMES:
        out[name] = rec[name]
    return out


def mismatches(got, want: dict, what: str) -> List[str]:
    """Field-by-field comparison of a library record (structured array entry) with a reference record."""
    bad = []
    for name in NAMES:
        g, w = np.asarray(got[name]), want[name]
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append(f"{what}: {name} is {g.dtype} {g.shape}, want {w.dtype} {w.shape}")
            continue
        if not np.array_equal(g, w):
            for c, i in np.argwhere(g != w)[:4]:
                bad.append(f"{what}: {name}[{c}][{i}] = {g[c, i]}, want {w[c, i]}")
    return bad
