"""The cross record of `measure` restated in numpy (test infrastructure): rules 12 - 17 of include/g1s_diff.h and the cross
report's text.

Imports nothing from the product package.  Records are dicts of numpy arrays with the PAIRING where the temporal record has
the plane (0: Cb against L, 1: Cr against L, 2: Cb against Cr): n (3, 32) uint64, x (3, 32) int64, u and v (3, 32) uint64,
c (3, 25) int64.  Sums are formed in Python integers where 64 bits could be left."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from tests.measure_ref import intensity

BINS, LAGS = 32, 25
# rule 15 = rule 8: dy = -2 .. 2, dx = -2 .. 2 in raster order, (0, 0) at index 12
OFFSETS = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3)]
assert len(OFFSETS) == LAGS and OFFSETS[12] == (0, 0) and OFFSETS[0] == (-2, -2) and OFFSETS[1] == (-1, -2)
FIELDS = (("n", np.uint64, BINS), ("x", np.int64, BINS), ("u", np.uint64, BINS), ("v", np.uint64, BINS), ("c", np.int64, LAGS))
PAIRINGS = ("cb_luma", "cr_luma", "cb_cr")


def empty_record() -> dict:
    return {name: np.zeros((3, size), dt) for name, dt, size in FIELDS}


def round2(v, s: int, truncate: bool = False):
    """Round2(v, s) = (v + ((1 << s) >> 1)) >> s with an arithmetic shift (numpy's >> on int64 is one): towards minus
    infinity.  truncate = True is the WRONG rounding (a division that truncates towards zero), there for the test that shows
    the difference."""
    v = np.asarray(v, np.int64) + ((1 << s) >> 1)
    if truncate:
        return np.where(v < 0, -((-v) >> s), v >> s)
    return v >> s


def luma_at_chroma(d_y: np.ndarray, cw: int, ch: int, xdec: int, ydec: int, truncate: bool = False) -> np.ndarray:
    """Rule 12: L on the cw x ch grid from the luma residual d_y (int64, H x W)."""
    d_y = np.asarray(d_y, np.int64)
    h, w = d_y.shape
    ys, xs = (np.arange(ch) << ydec)[:, None], (np.arange(cw) << xdec)[None, :]
    s = np.zeros((ch, cw), np.int64)
    for i in range(ydec + 1):
        for j in range(xdec + 1):
            s += d_y[np.minimum(ys + i, h - 1), np.minimum(xs + j, w - 1)]
    return round2(s, xdec + ydec, truncate)


def pairings(noisy: Sequence[np.ndarray], clean: Sequence[np.ndarray], xdec: int, ydec: int, truncate: bool = False):
    """Rule 13: [(a_0, b_0), (a_1, b_1), (a_2, b_2)] as int64 planes of the chroma grid."""
    d = [np.asarray(noisy[c]).astype(np.int64) - np.asarray(clean[c]).astype(np.int64) for c in range(3)]
    ch, cw = d[1].shape
    L = luma_at_chroma(d[0], cw, ch, xdec, ydec, truncate)
    return [(d[1], L), (d[2], L), (d[1], d[2])]


def cross_frame(noisy: Sequence[np.ndarray], clean: Sequence[np.ndarray], bit_depth: int, xdec: int = 1, ydec: int = 1,
                truncate: bool = False) -> dict:
    """Rules 12 - 16 on one pair: planes = [Y, U, V], or [Y] (all zeros)."""
    rec = empty_record()
    if len(clean) != 3:
        return rec
    k = (intensity(clean, 1, xdec, ydec) >> (bit_depth - 5)).ravel()
    for j, (a, b) in enumerate(pairings(noisy, clean, xdec, ydec, truncate)):
        ph, pw = a.shape
        rec["n"][j] = np.bincount(k, minlength=BINS).astype(np.uint64)
        for name, values in (("x", a * b), ("u", a * a), ("v", b * b)):
            s = np.zeros(BINS, np.int64)
            np.add.at(s, k, values.ravel())
            rec[name][j] = s.astype(rec[name].dtype)
        for i, (dx, dy) in enumerate(OFFSETS):
            if pw - abs(dx) <= 0 or ph - abs(dy) <= 0:
                continue
            # p = (x, y) and p + delta inside the chroma plane
            y0, y1, x0, x1 = max(0, -dy), ph - max(0, dy), max(0, -dx), pw - max(0, dx)
            rec["c"][j, i] = int((a[y0:y1, x0:x1] * b[y0 + dy:y1 + dy, x0 + dx:x1 + dx]).sum())
    return rec


def sum_records(records: Sequence[dict]) -> dict:
    """Rule 16's sum; an overflow of 64 bits raises OverflowError."""
    total = empty_record()
    for name, dt, _size in FIELDS:
        lo, hi = (0, 2 ** 64 - 1) if dt is np.uint64 else (-2 ** 63, 2 ** 63 - 1)
        flat = [sum(int(rec[name].ravel()[j]) for rec in records) for j in range(total[name].size)]
        if any(v < lo or v > hi for v in flat):
            raise OverflowError(name)
        total[name] = np.array(flat, dt).reshape(total[name].shape)
    return total


def _fmt(defined: bool, v: float) -> str:
    return "%.4f" % v if defined else "-"


def profile(t: dict, j: int, tm: List[float]) -> dict:
    """The printed values of pairing j: every value one f64 operation after the other, in the order of the grammar."""
    p = dict(has_rho=[False] * BINS, rho=[0.0] * BINS, has_slope=[False] * BINS, slope=[0.0] * BINS, has_lag=[False] * LAGS,
             lag=[0.0] * LAGS, peak=-1, has_beta=False, beta=0.0)
    U = V = 0
    for k in range(BINS):
        x, u, v = int(t["x"][j, k]), int(t["u"][j, k]), int(t["v"][j, k])
        U, V = (U + u) & (2 ** 64 - 1), (V + v) & (2 ** 64 - 1)  # (u64 sums)
        p["has_rho"][k] = u != 0 and v != 0
        if p["has_rho"][k]:
            p["rho"][k] = float(x) / math.sqrt(float(u) * float(v))
        p["has_slope"][k] = v != 0
        if v != 0:
            p["slope"][k] = float(x) / float(v)
    T = tm[12]
    for i in range(LAGS):
        p["has_lag"][i] = U != 0 and V != 0 and tm[i] > 0.0
        if not p["has_lag"][i]:
            continue
        p["lag"][i] = (float(int(t["c"][j, i])) / tm[i]) / math.sqrt((float(U) / T) * (float(V) / T))
        if p["peak"] < 0 or abs(p["lag"][i]) > abs(p["lag"][p["peak"]]):
            p["peak"] = i
    p["has_beta"] = V != 0
    if V != 0:
        p["beta"] = float(int(t["c"][j, 12])) / float(V)
    return p


def _peak(p: dict) -> str:
    if p["peak"] < 0:
        return "- - -"
    dx, dy = OFFSETS[p["peak"]]
    return f"{dx} {dy} {_fmt(True, p['lag'][p['peak']])}"


def partial_rho(ps: Sequence[dict]):
    """(defined, value) from the three pairings' zero_rho."""
    if not all(p["has_lag"][12] for p in ps):
        return False, 0.0
    r0, r1, r2 = (p["lag"][12] for p in ps)
    f0 = 1.0 - r0 * r0
    f1 = 1.0 - r1 * r1
    if f0 <= 0.0 or f1 <= 0.0:
        return False, 0.0
    return True, (r2 - r0 * r1) / math.sqrt(f0 * f1)


def terms_f64(frames: int, width: int, height: int, xdec: int, ydec: int) -> List[float]:
    cw, ch = (width + xdec) >> xdec, (height + ydec) >> ydec
    return [float(frames) * float(max(cw - abs(dx), 0)) * float(max(ch - abs(dy), 0)) for dx, dy in OFFSETS]


def format_cross(total: dict, frames: int, bit_depth: int, width: int, height: int, xdec: int = 1, ydec: int = 1,
                 synth: Optional[dict] = None) -> bytes:
    """Rule 17: the cross report (the grammar is in include/g1s_diff.h)."""
    out = ["graincross1", f"frames {frames} bit_depth {bit_depth}"]
    tm = terms_f64(frames, width, height, xdec, ydec)
    pa, pb = [], []
    for j, name in enumerate(PAIRINGS):
        out.append(f"pairing {name}")
        if not frames:
            continue
        a = profile(total, j, tm)
        b = profile(synth, j, tm) if synth is not None else None
        pa.append(a), pb.append(b)
        for k in range(BINS):
            if int(total["n"][j, k]) == 0:
                continue
            line = f"bin {k} {int(total['n'][j, k])} {_fmt(a['has_rho'][k], a['rho'][k])} {_fmt(a['has_slope'][k], a['slope'][k])}"
            if b is not None:
                line += f" {_fmt(b['has_rho'][k], b['rho'][k])} {_fmt(b['has_slope'][k], b['slope'][k])}"
            out.append(line)
        for i, (dx, dy) in enumerate(OFFSETS):
            line = f"lag {dx} {dy} {_fmt(a['has_lag'][i], a['lag'][i])}"
            if b is not None:
                line += f" {_fmt(b['has_lag'][i], b['lag'][i])}"
            out.append(line)
        out.append("zero_rho " + _fmt(a["has_lag"][12], a["lag"][12]) + ("" if b is None else " " + _fmt(b["has_lag"][12], b["lag"][12])))
        out.append("peak_rho " + _peak(a) + ("" if b is None else " " + _peak(b)))
        out.append("beta " + _fmt(a["has_beta"], a["beta"]) + ("" if b is None else " " + _fmt(b["has_beta"], b["beta"])))
        if j == 2:
            out.append("partial_rho " + _fmt(*partial_rho(pa)) + ("" if b is None else " " + _fmt(*partial_rho(pb))))
    return ("\n".join(out) + "\n").encode()


def to_struct(rec: dict, dtype) -> np.ndarray:
    """The record as an entry of the library's structured dtype (handed in by the caller: this module does not know it)."""
    out = np.zeros((), dtype)
    for name, _dt, _size in FIELDS:
        out[name] = rec[name]
    return out


def mismatches(got, want: dict, what: str) -> List[str]:
    """Field-by-field comparison of a library record (structured array entry) with a reference record."""
    bad = []
    for name, _dt, _size in FIELDS:
        g, w = np.asarray(got[name]), want[name]
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append(f"{what}: {name} is {g.dtype} {g.shape}, want {w.dtype} {w.shape}")
            continue
        if not np.array_equal(g, w):
            for c, i in np.argwhere(g != w)[:4]:
                bad.append(f"{what}: {name}[{c}][{i}] = {g[c, i]}, want {w[c, i]}")
    return bad
