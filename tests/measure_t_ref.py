"""The temporal record of `measure` restated in numpy (test infrastructure): rules 7 - 11 of include/g1s_diff.h and the
temporal report's text.

Imports nothing from the product package.  Records are dicts of numpy arrays: n (3, 32) uint64, x (3, 32) int64, u and v
(3, 32) uint64, c (3, 25) int64.  Sums are formed in Python integers where 64 bits could be left."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from tests.measure_ref import intensity

BINS, LAGS = 32, 25
# rule 8: dy = -2 .. 2, dx = -2 .. 2 in raster order, (0, 0) at index 12
OFFSETS = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3)]
assert len(OFFSETS) == LAGS and OFFSETS[12] == (0, 0) and OFFSETS[0] == (-2, -2) and OFFSETS[1] == (-1, -2)
FIELDS = (("n", np.uint64, BINS), ("x", np.int64, BINS), ("u", np.uint64, BINS), ("v", np.uint64, BINS), ("c", np.int64, LAGS))


def empty_record() -> dict:
    return {name: np.zeros((3, size), dt) for name, dt, size in FIELDS}


def terms(pw: int, ph: int) -> List[int]:
    return [max(pw - abs(dx), 0) * max(ph - abs(dy), 0) for dx, dy in OFFSETS]


def temporal_frame(noisy: Sequence[np.ndarray], clean: Sequence[np.ndarray], prev_noisy: Sequence[np.ndarray], prev_clean: Sequence[np.ndarray],
                   bit_depth: int, xdec: int = 1, ydec: int = 1) -> dict:
    """Rules 7 - 9: pair t = (noisy, clean) against pair t - 1 = (prev_noisy, prev_clean); planes = [Y] or [Y, U, V]."""
    rec = empty_record()
    for c in range(len(clean)):
        d = np.asarray(noisy[c]).astype(np.int64) - np.asarray(clean[c]).astype(np.int64)
        e = np.asarray(prev_noisy[c]).astype(np.int64) - np.asarray(prev_clean[c]).astype(np.int64)
        ph, pw = d.shape
        k = (intensity(clean, c, xdec, ydec) >> (bit_depth - 5)).ravel()
        rec["n"][c] = np.bincount(k, minlength=BINS).astype(np.uint64)
        for name, values in (("x", d * e), ("u", d * d), ("v", e * e)):
            s = np.zeros(BINS, np.int64)
            np.add.at(s, k, values.ravel())
            rec[name][c] = s.astype(rec[name].dtype)
        for i, (dx, dy) in enumerate(OFFSETS):
            if pw - abs(dx) <= 0 or ph - abs(dy) <= 0:
                continue
            # p = (x, y) and p + delta inside the plane
            y0, y1, x0, x1 = max(0, -dy), ph - max(0, dy), max(0, -dx), pw - max(0, dx)
            rec["c"][c, i] = int((d[y0:y1, x0:x1] * e[y0 + dy:y1 + dy, x0 + dx:x1 + dx]).sum())
    return rec


def run_records(pairs: Sequence, bit_depth: int, xdec: int = 1, ydec: int = 1) -> List[dict]:
    """The temporal records of one run: pairs = [(noisy, clean), ...]; one record for every pair but the first."""
    return [temporal_frame(pairs[t][0], pairs[t][1], pairs[t - 1][0], pairs[t - 1][1], bit_depth, xdec, ydec) for t in range(1, len(pairs))]


def sum_records(records: Sequence[dict]) -> dict:
    """Rule 10; an overflow of 64 bits raises OverflowError."""
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


def _profile(t: dict, c: int, tm: List[float]):
    """(has_bin, bin, has_lag, lag, peak): every value one f64 operation after the other, in the order of the grammar."""
    has_bin, rho_bin = [False] * BINS, [0.0] * BINS
    U = V = 0
    for k in range(BINS):
        u, v = int(t["u"][c, k]), int(t["v"][c, k])
        U, V = (U + u) & (2 ** 64 - 1), (V + v) & (2 ** 64 - 1)  # (u64 sums)
        has_bin[k] = u != 0 and v != 0
        if has_bin[k]:
            rho_bin[k] = float(int(t["x"][c, k])) / math.sqrt(float(u) * float(v))
    T = tm[12]
    has_lag, rho = [False] * LAGS, [0.0] * LAGS
    peak = -1
    for i in range(LAGS):
        has_lag[i] = U != 0 and V != 0 and tm[i] > 0.0
        if not has_lag[i]:
            continue
        rho[i] = (float(int(t["c"][c, i])) / tm[i]) / math.sqrt((float(U) / T) * (float(V) / T))
        if peak < 0 or abs(rho[i]) > abs(rho[peak]):
            peak = i
    return has_bin, rho_bin, has_lag, rho, peak


def _peak(p) -> str:
    if p[4] < 0:
        return "- - -"
    dx, dy = OFFSETS[p[4]]
    return f"{dx} {dy} {_fmt(True, p[3][p[4]])}"


def format_temporal(total: dict, pairs: int, bit_depth: int, width: int, height: int, xdec: int = 1, ydec: int = 1, nplanes: int = 3,
                    synth: Optional[dict] = None) -> bytes:
    """Rule 11: the temporal report (the grammar is in include/g1s_diff.h)."""
    out = ["graintemporal1", f"pairs {pairs} bit_depth {bit_depth} planes {nplanes}"]
    for c in range(nplanes):
        out.append(f"plane {c}")
        if not pairs:
            continue
        pw = (width + xdec) >> xdec if c else width
        ph = (height + ydec) >> ydec if c else height
        tm = [float(pairs) * float(max(pw - abs(dx), 0)) * float(max(ph - abs(dy), 0)) for dx, dy in OFFSETS]
        a = _profile(total, c, tm)
        b = _profile(synth, c, tm) if synth is not None else None
        for k in range(BINS):
            if int(total["n"][c, k]) == 0:
                continue
            line = f"bin {k} {int(total['n'][c, k])} {_fmt(a[0][k], a[1][k])}"
            if b is not None:
                line += f" {_fmt(b[0][k], b[1][k])}"
            out.append(line)
        for i, (dx, dy) in enumerate(OFFSETS):
            line = f"lag {dx} {dy} {_fmt(a[2][i], a[3][i])}"
            if b is not None:
                line += f" {_fmt(b[2][i], b[3][i])}"
            out.append(line)
        out.append("temporal_rho " + _fmt(a[2][12], a[3][12]) + ("" if b is None else " " + _fmt(b[2][12], b[3][12])))
        out.append("peak_rho " + _peak(a) + ("" if b is None else " " + _peak(b)))
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
