"""`measure` restated in numpy (test infrastructure): rules 1 - 6 of include/g1s_diff.h and the report text.

Imports nothing from the product package.  Records are dicts of numpy arrays: n (3, 32) uint64, s1 (3, 32) int64,
s2 (3, 32) uint64, r (3, 25) int64.  Sums are formed in Python integers where 64 bits could be left."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

BINS, LAGS = 32, 25
# rule 4: the lag-3 causal neighbourhood in the table's coefficient order, (0, 0) last
OFFSETS = [(dx, dy) for dy in range(-3, 1) for dx in range(-3, 4) if (dy, dx) < (0, 0)] + [(0, 0)]
assert len(OFFSETS) == LAGS and OFFSETS[0] == (-3, -3) and OFFSETS[23] == (-1, 0)


def empty_record() -> dict:
    return dict(n=np.zeros((3, BINS), np.uint64), s1=np.zeros((3, BINS), np.int64), s2=np.zeros((3, BINS), np.uint64),
                r=np.zeros((3, LAGS), np.int64))


def intensity(clean: Sequence[np.ndarray], c: int, xdec: int, ydec: int) -> np.ndarray:
    """Rule 2: the clean luma for luma, the specification's averageLuma of the clean frame for chroma."""
    y = np.asarray(clean[0]).astype(np.int64)
    if c == 0:
        return y
    h, w = y.shape
    ph, pw = np.asarray(clean[c]).shape
    ys = (np.arange(ph) << ydec)[:, None]
    xs = (np.arange(pw) << xdec)[None, :]
    if xdec:
        return (y[ys, xs] + y[ys, np.minimum(xs + 1, w - 1)] + 1) >> 1
    return y[ys, xs]


def terms(pw: int, ph: int) -> List[int]:
    return [max(pw - abs(dx), 0) * max(ph - abs(dy), 0) for dx, dy in OFFSETS]


def measure_frame(noisy: Sequence[np.ndarray], clean: Sequence[np.ndarray], bit_depth: int, xdec: int = 1, ydec: int = 1) -> dict:
    """Rules 1 - 5 on one pair: planes = [Y] or [Y, U, V]."""
    rec = empty_record()
    for c in range(len(clean)):
        d = np.asarray(noisy[c]).astype(np.int64) - np.asarray(clean[c]).astype(np.int64)
        ph, pw = d.shape
        k = (intensity(clean, c, xdec, ydec) >> (bit_depth - 5)).ravel()
        rec["n"][c] = np.bincount(k, minlength=BINS).astype(np.uint64)
        s1 = np.zeros(BINS, np.int64)
        s2 = np.zeros(BINS, np.int64)
        np.add.at(s1, k, d.ravel())
        np.add.at(s2, k, (d * d).ravel())
        rec["s1"][c], rec["s2"][c] = s1, s2.astype(np.uint64)
        for i, (dx, dy) in enumerate(OFFSETS):
            if pw - abs(dx) <= 0 or ph - abs(dy) <= 0:
                continue
            # p = (x, y) and p + delta inside: y + dy >= 0, 0 <= x + dx < pw
            y0, x0, x1 = -dy, max(0, -dx), pw - max(0, dx)
            a = d[y0:, x0:x1]
            b = d[0:ph + dy, x0 + dx:x1 + dx]
            rec["r"][c, i] = int((a * b).sum())
    return rec


def sum_records(records: Sequence[dict]) -> dict:
    """Rule 6; an overflow of 64 bits raises OverflowError."""
    total = empty_record()
    for name, lo, hi in (("n", 0, 2 ** 64 - 1), ("s1", -2 ** 63, 2 ** 63 - 1), ("s2", 0, 2 ** 64 - 1), ("r", -2 ** 63, 2 ** 63 - 1)):
        flat = [sum(int(rec[name].ravel()[j]) for rec in records) for j in range(total[name].size)]
        if any(v < lo or v > hi for v in flat):
            raise OverflowError(name)
        total[name] = np.array(flat, total[name].dtype).reshape(total[name].shape)
    return total


def _fmt(defined: bool, v: float) -> str:
    return "%.4f" % v if defined else "-"


def _profile(t: dict, c: int, tm: List[float]):
    has, mean, sigma = [False] * BINS, [0.0] * BINS, [0.0] * BINS
    for k in range(BINS):
        has[k] = int(t["n"][c, k]) > 0
        if not has[k]:
            continue
        n = float(int(t["n"][c, k]))
        mean[k] = float(int(t["s1"][c, k])) / n
        var = float(int(t["s2"][c, k])) / n - mean[k] * mean[k]
        sigma[k] = math.sqrt(var if var > 0.0 else 0.0)
    has_rho, rho = [False] * 24, [0.0] * 24
    for i in range(24):
        has_rho[i] = int(t["r"][c, 24]) != 0 and tm[i] > 0.0
        if has_rho[i]:
            rho[i] = (float(int(t["r"][c, i])) / tm[i]) / (float(int(t["r"][c, 24])) / tm[24])
    return has, mean, sigma, has_rho, rho


def format_profile(total: dict, frames: int, bit_depth: int, width: int, height: int, xdec: int = 1, ydec: int = 1, nplanes: int = 3,
                   synth: Optional[dict] = None) -> bytes:
    """The report (the grammar is in include/g1s_diff.h): every value one f64 operation after the other, as the library."""
    out = ["grainprofile1", f"frames {frames} bit_depth {bit_depth} planes {nplanes}"]
    for c in range(nplanes):
        pw = (width + xdec) >> xdec if c else width
        ph = (height + ydec) >> ydec if c else height
        tm = [float(max(pw - abs(dx), 0)) * float(max(ph - abs(dy), 0)) * float(frames) for dx, dy in OFFSETS]
        out.append(f"plane {c}")
        a = _profile(total, c, tm)
        b = _profile(synth, c, tm) if synth is not None else None
        for k in range(BINS):
            if not a[0][k]:
                continue
            line = f"bin {k} {int(total['n'][c, k])} {_fmt(True, a[1][k])} {_fmt(True, a[2][k])}"
            if b is not None:
                line += f" {_fmt(b[0][k], b[1][k])} {_fmt(b[0][k], b[2][k])}"
            out.append(line)
        for i in range(24):
            dx, dy = OFFSETS[i]
            line = f"lag {dx} {dy} {_fmt(a[3][i], a[4][i])}"
            if b is not None:
                line += f" {_fmt(b[3][i], b[4][i])}"
            out.append(line)
        if b is not None:
            diffs = [abs(b[4][i] - a[4][i]) for i in range(24) if a[3][i] and b[3][i]]
            out.append("max_rho_diff " + _fmt(bool(diffs), max(diffs) if diffs else 0.0))
            num = den = 0.0
            for k in range(BINS):
                if a[0][k] and b[0][k] and a[2][k] > 0.0 and b[2][k] > 0.0:
                    n = float(int(total["n"][c, k]))
                    num += n * (b[2][k] / a[2][k])
                    den += n
            out.append("sigma_ratio " + _fmt(den > 0.0, num / den if den > 0.0 else 0.0))
    return ("\n".join(out) + "\n").encode()


def to_struct(rec: dict, dtype) -> np.ndarray:
    """The record as an entry of the library's structured dtype (handed in by the caller: this module does not know it)."""
    out = np.zeros((), dtype)
    for name in ("n", "s1", "s2", "r"):
        out[name] = rec[name]
    return out


def mismatches(got, want: dict, what: str) -> List[str]:
    """Field-by-field comparison of a library record (structured array entry) with a reference record."""
    bad = []
    for name in ("n", "s1", "s2", "r"):
        g, w = np.asarray(got[name]), want[name]
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append(f"{what}: {name} is {g.dtype} {g.shape}, want {w.dtype} {w.shape}")
            continue
        for c, i in np.argwhere(g != w)[:4]:
            bad.append(f"{what}: {name}[{c}][{i}] = {g[c, i]}, want {w[c, i]}")
    return bad
