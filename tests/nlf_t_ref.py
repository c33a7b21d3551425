"""Temporal noise levels restated in numpy (test infrastructure): rules T1 - T8 of include/g1s_diff.h, on top of
tests/nlf_ref.py (N1's stencil, N2's averageLuma, N6's interpolation).

Imports nothing from the product package.  Temporal records are dicts of numpy arrays: n and q (3, 32) uint64, s (3, 32)
int64.  Everything that could leave 64 bits is formed in Python integers."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from tests import nlf_ref as R

BINS = R.BINS
BOX_GATE = 144
NAMES = ("n", "s", "q")
DTYPES = {"n": np.uint64, "s": np.int64, "q": np.uint64}
SUMS_LEAVE_64 = "the clip's sums leave 64 bits"


def empty_record() -> dict:
    return {name: np.zeros((3, BINS), DTYPES[name]) for name in NAMES}


def average_luma(luma: np.ndarray, ph: int, pw: int, xdec: int, ydec: int) -> np.ndarray:
    """N2's averageLuma for every sample of a ph x pw chroma plane (before the shift to a bin)."""
    y = np.asarray(luma).astype(np.int64)
    _h, w = y.shape
    ys = (np.arange(ph) << ydec)[:, None]
    xs = (np.arange(pw) << xdec)[None, :]
    return (y[ys, xs] + y[ys, np.minimum(xs + 1, w - 1)] + 1) >> 1 if xdec else y[ys, xs] + 0 * xs


def gate_parts(cur: np.ndarray, before: np.ndarray, bit_depth: int):
    """T2's three conditions on the interior of a plane pair and the two box sums: (gate_t, gate_before, box, S9_t, S9_before);
    None when the interior is empty."""
    sh = bit_depth - 8
    half = (1 << (sh - 1)) if sh else 0
    st, sb = R.stencil(cur), R.stencil(before)
    if st is None:
        return None
    gate_t = ((np.abs(st[0]) + np.abs(st[1]) + half) >> sh) < R.EDGE_THRESHOLD
    gate_b = ((np.abs(sb[0]) + np.abs(sb[1]) + half) >> sh) < R.EDGE_THRESHOLD
    box = np.abs(st[3] - sb[3]) < (BOX_GATE << sh)
    return gate_t, gate_b, box, st[3], sb[3]


def nlf_pair(cur: Sequence[np.ndarray], before: Sequence[np.ndarray], bit_depth: int, xdec: int = 1, ydec: int = 1, *, gate="both", bins="both",
             box_strict=True) -> dict:
    """T1 - T5 on one pair: frame t (`cur`) against frame t - 1 (`before`).  The keyword arguments make the wrong
    restatements the tests tell apart: gate = "t" (N1's gate on frame t only), bins = "t" (bins from frame t alone),
    box_strict = False (<= in T2's third condition)."""
    rec = empty_record()
    for c, (pc, pb) in enumerate(zip(cur, before)):
        parts = gate_parts(pc, pb, bit_depth)
        if parts is None:
            continue
        gate_t, gate_b, box, s9t, s9b = parts
        if not box_strict:
            box = np.abs(s9t - s9b) <= (BOX_GATE << (bit_depth - 8))
        counts = gate_t & box & (gate_b if gate == "both" else True)
        ph, pw = np.asarray(pc).shape
        if c == 0:
            k = (s9t + s9b) // (18 << (bit_depth - 5)) if bins == "both" else s9t // (9 << (bit_depth - 5))
        else:
            at = average_luma(cur[0], ph, pw, xdec, ydec)[1:-1, 1:-1]
            ab = average_luma(before[0], ph, pw, xdec, ydec)[1:-1, 1:-1]
            k = (at + ab) >> (bit_depth - 4) if bins == "both" else at >> (bit_depth - 5)
        e = (np.asarray(pc).astype(np.int64) - np.asarray(pb).astype(np.int64))[1:-1, 1:-1]
        k, e = k[counts], e[counts]
        rec["n"][c] = np.bincount(k, minlength=BINS).astype(np.uint64)
        s = np.zeros(BINS, np.int64)
        np.add.at(s, k, e)
        rec["s"][c] = s
        q = np.zeros(BINS, np.int64)  # (e^2 < 2^24 and a plane has fewer than 2^31 samples here)
        np.add.at(q, k, e * e)
        rec["q"][c] = q.astype(np.uint64)
    return rec


def nlf_pair_loop(cur: Sequence[np.ndarray], before: Sequence[np.ndarray], bit_depth: int, xdec: int = 1, ydec: int = 1) -> dict:
    """T1 - T5 as a plain loop over samples in Python integers: what nlf_pair is checked against."""
    sh = bit_depth - 8
    half = (1 << (sh - 1)) if sh else 0
    n = [[0] * BINS for _ in range(3)]
    s = [[0] * BINS for _ in range(3)]
    q = [[0] * BINS for _ in range(3)]
    W = int(np.asarray(cur[0]).shape[1])

    def gate_and_box(u, y, x):
        m = [[int(u[y - 1 + i][x - 1 + j]) for j in range(3)] for i in range(3)]
        gx = (m[0][0] - m[0][2]) + (m[2][0] - m[2][2]) + 2 * (m[1][0] - m[1][2])
        gy = (m[0][0] - m[2][0]) + (m[0][2] - m[2][2]) + 2 * (m[0][1] - m[2][1])
        return ((abs(gx) + abs(gy) + half) >> sh) < 50, sum(sum(r) for r in m)

    def avg_luma(luma, y, x):
        ys, xs = y << ydec, x << xdec
        if not xdec:
            return int(luma[ys][xs])
        return (int(luma[ys][xs]) + int(luma[ys][min(xs + 1, W - 1)]) + 1) >> 1

    for c in range(len(cur)):
        ut, ub = np.asarray(cur[c]).tolist(), np.asarray(before[c]).tolist()
        ph, pw = len(ut), len(ut[0])
        lt, lb = np.asarray(cur[0]).tolist(), np.asarray(before[0]).tolist()
        for y in range(1, ph - 1):
            for x in range(1, pw - 1):
                gt, s9t = gate_and_box(ut, y, x)
                gb, s9b = gate_and_box(ub, y, x)
                if not (gt and gb and abs(s9t - s9b) < 144 * (1 << sh)):
                    continue
                if c == 0:
                    k = (s9t + s9b) // (18 * (1 << (bit_depth - 5)))
                else:
                    k = (avg_luma(lt, y, x) + avg_luma(lb, y, x)) >> (bit_depth - 4)
                e = ut[y][x] - ub[y][x]
                n[c][k] += 1
                s[c][k] += e
                q[c][k] += e * e
    return {"n": np.array(n, np.uint64), "s": np.array(s, np.int64), "q": np.array(q, np.uint64)}


def run_records(frames: Sequence[Sequence[np.ndarray]], bit_depth: int, xdec: int = 1, ydec: int = 1) -> List[dict]:
    """The temporal records of one run: one per frame but the first."""
    return [nlf_pair(frames[t], frames[t - 1], bit_depth, xdec, ydec) for t in range(1, len(frames))]


def sum_records(records: Sequence[dict]) -> dict:
    """T5; an overflow of 64 bits raises OverflowError."""
    total = empty_record()
    for name in NAMES:
        flat = [sum(int(rec[name].ravel()[j]) for rec in records) for j in range(total[name].size)]
        lo, hi = (-(2 ** 63), 2 ** 63 - 1) if name == "s" else (0, 2 ** 64 - 1)
        if any(v < lo or v > hi for v in flat):
            raise OverflowError(name)
        total[name] = np.array(flat, DTYPES[name]).reshape(3, BINS)
    return total


def level(n: int, s: int, q: int, *, remove_mean=True, wrap_s2=False) -> int:
    """T6 for one bin with n > 0.  remove_mean = False and wrap_s2 = True (s^2 taken modulo 2^64) are wrong restatements."""
    s2 = s * s if remove_mean else 0
    if wrap_s2:
        s2 %= 1 << 64
    return math.isqrt(max((n * q - s2) << 16, 0) // (2 * n * n))


def class_bins(total: dict, plane_class: int):
    planes = (1, 2) if plane_class else (0,)
    out = []
    for k in range(BINS):
        n, s, q = (sum(int(total[name][c, k]) for c in planes) for name in NAMES)
        if n > 2 ** 64 - 1 or q > 2 ** 64 - 1 or not -(2 ** 63) <= s <= 2 ** 63 - 1:
            raise ValueError(SUMS_LEAVE_64)
        out.append((n, s, q))
    return out


def levels(total: dict, min_count: int = 0, plane_class: int = 0, **wrong) -> List[Optional[int]]:
    """T6: t_T[k] of a plane class, None where n < Nmin."""
    nmin = min_count or R.DEFAULT_MIN_COUNT
    return [level(n, s, q, **wrong) if n >= nmin else None for n, s, q in class_bins(total, plane_class)]


def sigma_from_levels(t: Sequence[Optional[int]], bit_depth: int, none_text: str) -> np.ndarray:
    """N6's y and interpolation on given levels."""
    valid = [k for k in range(BINS) if t[k] is not None]
    if not valid:
        raise ValueError(none_text)
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
            s[v] = y[i] + ((y[i + 1] - y[i]) * (v - c[i]) * 2 + (c[i + 1] - c[i])) // (2 * (c[i + 1] - c[i]))
    return s


def sigma(total: dict, bit_depth: int, min_count: int = 0, **wrong) -> np.ndarray:
    """T7's N6: s[1 << B]; ValueError with the refusal's text."""
    if bit_depth == 12:
        raise ValueError("a grain prior needs headroom above the clip's bit depth: the stabilised domain is 12 bits, so a 12-bit clip is refused")
    if bit_depth not in (8, 10):
        raise ValueError("a grain prior is defined for bit depths 8 and 10")
    return sigma_from_levels(levels(total, min_count, 0, **wrong), bit_depth, "no luma bin has enough smooth samples for a prior")


def chroma_sigma(total: dict, min_count: int = 0) -> np.ndarray:
    """T7's N9: s[256]."""
    return sigma_from_levels(levels(total, min_count, 1), 8, "no chroma bin has enough smooth samples for a prior")


def variance(N: int, S: int, Q: int) -> float:
    m2, m = float(Q) / float(N), float(S) / float(N)
    v = m2 - m * m
    return v if v > 0.0 else 0.0


def plane_sums(total: dict, planes):
    return tuple(sum(int(total[name][c, k]) for c in planes for k in range(BINS)) for name in NAMES)


def strength(total: dict, bit_depth: int, min_count: int = 0, plane_class: int = 0) -> Optional[float]:
    """T7's strength for a plane class: h, or None where N7 refuses."""
    N, S, Q = plane_sums(total, (1, 2) if plane_class else (0,))
    if N < (min_count or R.DEFAULT_MIN_COUNT):
        return None
    h = math.sqrt(variance(N, S, Q)) / float(1 << (bit_depth - 8))
    return h if 0.0 < h <= 1000.0 else None


def plane_sigma_t(total: dict, c: int) -> Optional[float]:
    N, S, Q = plane_sums(total, (c,))
    return math.sqrt(variance(N, S, Q) / 2.0) if N else None


def plane_sigma(ordinary: dict, c: int) -> Optional[float]:
    """N8's plane_sigma."""
    N, Q = (sum(int(ordinary[name][c, k]) for k in range(BINS)) for name in ("n", "q"))
    return math.sqrt(float(Q) / float(36 * N)) if N else None


def _fmt(defined: bool, v: float) -> str:
    return "%.4f" % v if defined else "-"


def format_noise_levels_temporal(total: dict, pairs: int, bit_depth: int, nplanes: int = 3, min_count: int = 0, ordinary: Optional[dict] = None) -> bytes:
    """T8 (the grammar is in include/g1s_diff.h)."""
    out = ["noiselevels_t1", f"pairs {pairs} bit_depth {bit_depth} planes {nplanes}"]
    for c in range(nplanes):
        out.append(f"plane {c}")
        for k in range(BINS):
            n, s, q = (int(total[name][c, k]) for name in NAMES)
            if n:
                out.append(f"bin {k} {n} {_fmt(True, math.sqrt(variance(n, s, q) / 2.0))}")
        st = plane_sigma_t(total, c)
        out.append("plane_sigma_t " + _fmt(st is not None, st or 0.0))
        so = plane_sigma(ordinary, c) if ordinary is not None else None
        ok = st is not None and so is not None and so > 0.0
        out.append("ratio " + _fmt(ok, st / so if ok else 0.0))
    hl, hc = strength(total, bit_depth, min_count, 0), strength(total, bit_depth, min_count, 1)
    out.append(f"auto_strength_t {_fmt(hl is not None, hl or 0.0)} {_fmt(hc is not None, hc or 0.0)}")
    return ("\n".join(out) + "\n").encode()


def to_struct(rec: dict, dtype) -> np.ndarray:
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
