"""The scale record of `measure` restated in numpy (test infrastructure): rules 18 - 23 of include/g1s_diff.h and the scale
report's text.

Imports nothing from the product package.  Records are dicts of numpy arrays indexed [plane][k - 1][bin]: n (3, 5, 32) uint64,
s1 (3, 5, 32) int64, s2 (3, 5, 32) uint64.  Sums are formed in Python integers where 64 bits could be left.  The keyword
arguments of scale_frame are the WRONG restatements, one a rule, there for the tests that show each rule bites."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from tests.measure_ref import intensity

BINS, SCALES = 32, 5
FIELDS = (("n", np.uint64), ("s1", np.int64), ("s2", np.uint64))


def empty_record() -> dict:
    return {name: np.zeros((3, SCALES, BINS), dt) for name, dt in FIELDS}


def box_sums(v: np.ndarray, k: int) -> np.ndarray:
    """Rule 18: the sums of v over the whole boxes of side 2^k aligned at the origin, (ph >> k, pw >> k)."""
    L = 1 << k
    ph, pw = v.shape
    bh, bw = ph >> k, pw >> k
    return v[:bh * L, :bw * L].reshape(bh, L, bw, L).sum(axis=(1, 3))


def scale_frame(noisy: Sequence[np.ndarray], clean: Sequence[np.ndarray], bit_depth: int, xdec: int = 1, ydec: int = 1, *,
                bin_by_sample: bool = False, rounded_mean: bool = False, luma_sum: bool = False, square32: bool = False) -> dict:
    """Rules 18 - 21 on one pair: planes = [Y] or [Y, U, V]."""
    rec = empty_record()
    for c in range(len(clean)):
        d = np.asarray(noisy[c]).astype(np.int64) - np.asarray(clean[c]).astype(np.int64)
        I = intensity(clean, c, xdec, ydec)
        for k in range(1, SCALES + 1):
            B = box_sums(d, k)
            if not B.size:
                continue
            C = box_sums(I, k)
            shift = 2 * k + bit_depth - 5
            if bin_by_sample:  # WRONG: the box's first sample stands for the box
                K = I[::1 << k, ::1 << k][:B.shape[0], :B.shape[1]] >> (bit_depth - 5)
            elif rounded_mean:  # WRONG: the box mean rounded to nearest before it is binned
                K = ((C + (1 << (2 * k - 1))) >> (2 * k)) >> (bit_depth - 5)
            elif luma_sum and c and xdec:  # WRONG: chroma binned by the plain sum of the luma samples under the box's row
                y = np.asarray(clean[0]).astype(np.int64)
                h, w = y.shape
                ys, xs = (np.arange(I.shape[0]) << ydec)[:, None], (np.arange(I.shape[1]) << xdec)[None, :]
                K = box_sums(y[ys, xs] + y[ys, np.minimum(xs + 1, w - 1)], k) >> (shift + 1)
            else:
                K = C >> shift
            K = np.minimum(K, BINS - 1).ravel()
            sq = B * B
            if square32:  # WRONG: the square wrapped to 32 bits
                sq = sq & 0xffffffff
            rec["n"][c, k - 1] = np.bincount(K, minlength=BINS).astype(np.uint64)
            s1, s2 = np.zeros(BINS, np.int64), np.zeros(BINS, np.int64)
            np.add.at(s1, K, B.ravel())
            np.add.at(s2, K, sq.ravel())  # (below 2^63: rule 21's bound with the planes the tests use)
            rec["s1"][c, k - 1], rec["s2"][c, k - 1] = s1, s2.astype(np.uint64)
    return rec


def sum_records(records: Sequence[dict]) -> dict:
    """Rule 22; an overflow of 64 bits raises OverflowError."""
    total = empty_record()
    for name, dt in FIELDS:
        lo, hi = (0, 2 ** 64 - 1) if dt is np.uint64 else (-2 ** 63, 2 ** 63 - 1)
        flat = [sum(int(rec[name].ravel()[j]) for rec in records) for j in range(total[name].size)]
        if any(v < lo or v > hi for v in flat):
            raise OverflowError(name)
        total[name] = np.array(flat, dt).reshape(total[name].shape)
    return total


def _fmt(defined: bool, v: float) -> str:
    return "%.4f" % v if defined else "-"


def pooled_variance(n, s1, s2):
    """(m, V) of rule 23 over 32 bins; V is None when m = 0.  One f64 operation after the other, in the header's order."""
    m, S = 0, 0.0
    for j in range(BINS):
        nj = int(n[j])
        if not nj:
            continue
        m = (m + nj) & (2 ** 64 - 1)
        sq = float(int(s1[j])) * float(int(s1[j]))
        part = sq / float(nj)
        S = S + (float(int(s2[j])) - part)
    return m, (S / float(m) if m else None)


def column(plain: dict, scale: dict, c: int) -> dict:
    """The printed values of plane c of one column: sigma[k - 1], gain[k - 1] (None: "-")."""
    _m0, v0 = pooled_variance(plain["n"][c], plain["s1"][c], plain["s2"][c])
    sigma: List[Optional[float]] = [None] * SCALES
    gain: List[Optional[float]] = [None] * SCALES
    for k in range(SCALES):
        _m, v = pooled_variance(scale["n"][c, k], scale["s1"][c, k], scale["s2"][c, k])
        if v is None:
            continue
        L = float(2 << k)
        sigma[k] = math.sqrt(v if v > 0.0 else 0.0) / L
        if v0 is not None and v0 > 0.0:
            den = (L * L) * v0
            gain[k] = v / den
    return dict(sigma=sigma, gain=gain)


def _bin_sigma(rec: dict, c: int, k: int, j: int) -> float:
    n = float(int(rec["n"][c, k, j]))
    mean = float(int(rec["s1"][c, k, j])) / n
    var = float(int(rec["s2"][c, k, j])) / n - mean * mean
    return math.sqrt(var if var > 0.0 else 0.0) / float(2 << k)


def _opt(v: Optional[float]) -> str:
    return _fmt(v is not None, v if v is not None else 0.0)


def format_scales(total: dict, stotal: dict, frames: int, bit_depth: int, nplanes: int = 3, synth: Optional[dict] = None,
                  ssynth: Optional[dict] = None) -> bytes:
    """Rule 23: the scale report (the grammar is in include/g1s_diff.h)."""
    out = ["grainscales1", f"frames {frames} bit_depth {bit_depth} planes {nplanes}"]
    for c in range(nplanes):
        out.append(f"plane {c}")
        if not frames:
            continue
        a = column(total, stotal, c)
        b = column(synth, ssynth, c) if synth is not None else None
        for k in range(SCALES):
            m = sum(int(v) for v in stotal["n"][c, k]) & (2 ** 64 - 1)
            line = f"scale {k + 1} boxes {m} {_opt(a['sigma'][k])} {_opt(a['gain'][k])}"
            if b is not None:
                line += f" {_opt(b['sigma'][k])} {_opt(b['gain'][k])}"
            out.append(line)
        for k in range(SCALES):
            for j in range(BINS):
                if not int(stotal["n"][c, k, j]):
                    continue
                line = f"sbin {k + 1} {j} {int(stotal['n'][c, k, j])} {_fmt(True, _bin_sigma(stotal, c, k, j))}"
                if b is not None:
                    line += " " + (_fmt(True, _bin_sigma(ssynth, c, k, j)) if int(ssynth["n"][c, k, j]) else "-")
                out.append(line)
        if b is not None:
            for k in range(SCALES):
                ga, gb = a["gain"][k], b["gain"][k]
                both = ga is not None and gb is not None and ga > 0.0
                out.append(f"gain_ratio {k + 1} " + _fmt(both, gb / ga if both else 0.0))
    return ("\n".join(out) + "\n").encode()


def to_struct(rec: dict, dtype) -> np.ndarray:
    """The record as an entry of the library's structured dtype (handed in by the caller: this module does not know it)."""
    out = np.zeros((), dtype)
    for name, _dt in FIELDS:
        out[name] = rec[name]
    return out


def mismatches(got, want: dict, what: str) -> List[str]:
    """Field-by-field comparison of a library record (structured array entry) with a reference record."""
    bad = []
    for name, _dt in FIELDS:
        g, w = np.asarray(got[name]), want[name]
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append(f"{what}: {name} is {g.dtype} {g.shape}, want {w.dtype} {w.shape}")
            continue
        for c, k, j in np.argwhere(g != w)[:4]:
            bad.append(f"{what}: {name}[{c}][{k}][{j}] = {g[c, k, j]}, want {w[c, k, j]}")
    return bad
