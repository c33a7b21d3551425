"""Lagged noise levels restated in numpy (test infrastructure): rules L1 - L5 of include/g1s_diff.h, on tests/nlf_t_ref.py's
gate_parts (T2's gate), and rules L6 - L7 (the AR fit on a clip's record) with the library's order of operations.  L4's Lbar is `measure`'s rule 12 (a box with Round2), not N2's averageLuma, so it is formed here.

Imports nothing from the product package.  Lag records are dicts of numpy arrays: n (3, 46) uint64, r (3, 46) int64, s (3,)
int64, xn (2, 25) uint64, xr (2, 25) int64, ln uint64, ls int64, l2 uint64 (the last three 0-d arrays)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from tests import nlf_t_ref as T

# L2: (dx, dy) of lag i
LAGS = [(dx, 0) for dx in range(7)] + [(dx, dy) for dy in (1, 2, 3) for dx in range(-6, 7)]
# L4: rule 4 of `measure`: the 24 causal offsets in the table's coefficient order, (0, 0) at index 24
CROSS = [(dx, dy) for dy in (-3, -2, -1) for dx in range(-3, 4)] + [(dx, 0) for dx in (-3, -2, -1)] + [(0, 0)]
assert len(LAGS) == 46 and len(CROSS) == 25
NAMES = ("n", "r", "s", "xn", "xr", "ln", "ls", "l2")
SHAPES = {"n": (3, 46), "r": (3, 46), "s": (3,), "xn": (2, 25), "xr": (2, 25), "ln": (), "ls": (), "l2": ()}
DTYPES = {"n": np.uint64, "r": np.int64, "s": np.int64, "xn": np.uint64, "xr": np.int64, "ln": np.uint64, "ls": np.int64, "l2": np.uint64}
LRECORD = np.dtype([(name, "<u8" if DTYPES[name] is np.uint64 else "<i8", SHAPES[name]) for name in NAMES])


def empty_record() -> dict:
    return {name: np.zeros(SHAPES[name], DTYPES[name]) for name in NAMES}


def gate_and_difference(cur: np.ndarray, before: np.ndarray, bit_depth: int):
    """L1 and T1 on a whole plane: (g, e), each (ph, pw) int64; g is 0 off the interior."""
    u, v = np.asarray(cur).astype(np.int64), np.asarray(before).astype(np.int64)
    g = np.zeros(u.shape, np.int64)
    parts = T.gate_parts(u, v, bit_depth)
    if parts is not None:
        gate_t, gate_b, box = parts[:3]
        g[1:-1, 1:-1] = gate_t & box & gate_b
    return g, u - v


def overlap(a: np.ndarray, b: np.ndarray, dx: int, dy: int):
    """(a(p), b(p + d)) over every p for which p and p + d lie inside the plane (two views; empty where there is none)."""
    h, w = a.shape
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y1 <= y0 or x1 <= x0:
        return a[:0, :0], b[:0, :0]
    return a[y0:y1, x0:x1], b[y0 + dy:y1 + dy, x0 + dx:x1 + dx]


def luma_under(g0: np.ndarray, e0: np.ndarray, ph: int, pw: int, xdec: int, ydec: int, *, truncate=False, clamp=True, first_only=False):
    """L4: (gL, Lbar) on the ph x pw chroma grid.  The keyword arguments make wrong restatements: Lbar truncating towards
    zero, the box without the clamp (a sample past the edge taken as 0 and as counting), gL from the box's first sample."""
    H, W = e0.shape
    ys, xs = (np.arange(ph) << ydec)[:, None], (np.arange(pw) << xdec)[None, :]
    total = np.zeros((ph, pw), np.int64)
    gl = np.ones((ph, pw), np.int64)
    for i in range(ydec + 1):
        for j in range(xdec + 1):
            Y, X = ys + i, xs + j
            if clamp:
                Y, X = np.minimum(Y, H - 1), np.minimum(X, W - 1)
                total += e0[Y, X]
                gl &= g0[Y, X] if not (first_only and (i or j)) else 1
            else:
                inside = (Y < H) & (X < W)
                Yc, Xc = np.minimum(Y, H - 1), np.minimum(X, W - 1)
                total += np.where(inside, e0[Yc, Xc], 0)
                gl &= np.where(inside, g0[Yc, Xc], 1)
    s = xdec + ydec
    if truncate:
        lbar = np.sign(total) * (np.abs(total) >> s)
    else:
        lbar = (total + ((1 << s) >> 1)) >> s
    return gl, lbar


def lags_pair(cur: Sequence[np.ndarray], before: Sequence[np.ndarray], bit_depth: int, xdec: int = 1, ydec: int = 1, *, gate_at="both", mirror_dx=False,
              wrap32=False, **luma_kw) -> dict:
    """L1 - L5 on one pair: frame t (`cur`) against frame t - 1 (`before`).  Wrong restatements: gate_at = "p" (the gate at
    p only), mirror_dx (dx mirrored), wrap32 (the products summed in 32 bits), and luma_under's."""
    ge = [gate_and_difference(pc, pb, bit_depth) for pc, pb in zip(cur, before)]
    return lags_of_fields(ge, xdec, ydec, gate_at=gate_at, mirror_dx=mirror_dx, wrap32=wrap32, **luma_kw)


def lags_of_fields(ge, xdec: int = 1, ydec: int = 1, *, gate_at="both", mirror_dx=False, wrap32=False, **luma_kw) -> dict:
    """L3 - L5 on given (g, e) per plane: lags_pair behind the gate.  With g = 1 everywhere these are the ungated sums of any
    fields, which the estimation tests compare against."""
    rec = empty_record()
    for c, (g, e) in enumerate(ge):
        rec["s"][c] = int((e * g).sum())
        for i, (dx, dy) in enumerate(LAGS):
            dx = -dx if mirror_dx else dx
            ga, gb = overlap(g, g, dx, dy)
            ea, eb = overlap(e, e, dx, dy)
            both = ga * gb if gate_at == "both" else ga
            prod = ea * eb
            r = int((prod * both).sum())
            rec["n"][c, i] = int(both.sum())
            rec["r"][c, i] = (r + 2 ** 31) % 2 ** 32 - 2 ** 31 if wrap32 else r
    if len(ge) == 3:
        ph, pw = ge[1][1].shape
        gl, lbar = luma_under(ge[0][0], ge[0][1], ph, pw, xdec, ydec, **luma_kw)
        rec["ln"] = np.uint64(int(gl.sum()))
        rec["ls"] = np.int64(int((lbar * gl).sum()))
        rec["l2"] = np.uint64(int((lbar * lbar * gl).sum()))
        for c in (1, 2):
            g, e = ge[c]
            for j, (dx, dy) in enumerate(CROSS):
                ga, gb = overlap(gl, g, dx, dy)
                la, eb = overlap(lbar, e, dx, dy)
                rec["xn"][c - 1, j] = int((ga * gb).sum())
                rec["xr"][c - 1, j] = int((la * eb * ga * gb).sum())
    return rec


def lags_pair_loop(cur: Sequence[np.ndarray], before: Sequence[np.ndarray], bit_depth: int, xdec: int = 1, ydec: int = 1) -> dict:
    """L1 - L5 as a plain loop over samples and lags in Python integers: what lags_pair is checked against."""
    sh = bit_depth - 8
    half = (1 << (sh - 1)) if sh else 0

    def gate_and_box(u, y, x):
        m = [[u[y - 1 + i][x - 1 + j] for j in range(3)] for i in range(3)]
        gx = (m[0][0] - m[0][2]) + (m[2][0] - m[2][2]) + 2 * (m[1][0] - m[1][2])
        gy = (m[0][0] - m[2][0]) + (m[0][2] - m[2][2]) + 2 * (m[0][1] - m[2][1])
        return ((abs(gx) + abs(gy) + half) >> sh) < 50, sum(sum(r) for r in m)

    planes = []
    for pc, pb in zip(cur, before):
        ut, ub = np.asarray(pc).tolist(), np.asarray(pb).tolist()
        ph, pw = len(ut), len(ut[0])
        g = [[0] * pw for _ in range(ph)]
        e = [[ut[y][x] - ub[y][x] for x in range(pw)] for y in range(ph)]
        for y in range(1, ph - 1):
            for x in range(1, pw - 1):
                gt, s9t = gate_and_box(ut, y, x)
                gb, s9b = gate_and_box(ub, y, x)
                g[y][x] = int(gt and gb and abs(s9t - s9b) < 144 * (1 << sh))
        planes.append((g, e, ph, pw))
    rec = {name: np.zeros(SHAPES[name], object) for name in NAMES}
    for c, (g, e, ph, pw) in enumerate(planes):
        for y in range(ph):
            for x in range(pw):
                if not g[y][x]:
                    continue
                rec["s"][c] += e[y][x]
                for i, (dx, dy) in enumerate(LAGS):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < ph and 0 <= xx < pw and g[yy][xx]:
                        rec["n"][c, i] += 1
                        rec["r"][c, i] += e[y][x] * e[yy][xx]
    if len(planes) == 3:
        g0, e0, H, W = planes[0]
        _, _, ph, pw = planes[1]
        s = xdec + ydec
        gl = [[0] * pw for _ in range(ph)]
        lbar = [[0] * pw for _ in range(ph)]
        ln = ls = l2 = 0
        for y in range(ph):
            for x in range(pw):
                box = [(min((y << ydec) + i, H - 1), min((x << xdec) + j, W - 1)) for i in range(ydec + 1) for j in range(xdec + 1)]
                gl[y][x] = int(all(g0[Y][X] for Y, X in box))
                lbar[y][x] = (sum(e0[Y][X] for Y, X in box) + ((1 << s) >> 1)) >> s
                if gl[y][x]:
                    ln, ls, l2 = ln + 1, ls + lbar[y][x], l2 + lbar[y][x] ** 2
        rec["ln"], rec["ls"], rec["l2"] = np.array(ln, object), np.array(ls, object), np.array(l2, object)
        for c in (1, 2):
            g, e, _, _ = planes[c]
            for y in range(ph):
                for x in range(pw):
                    if not gl[y][x]:
                        continue
                    for j, (dx, dy) in enumerate(CROSS):
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < ph and 0 <= xx < pw and g[yy][xx]:
                            rec["xn"][c - 1, j] += 1
                            rec["xr"][c - 1, j] += lbar[y][x] * e[yy][xx]
    return {name: np.array(rec[name].tolist(), DTYPES[name]).reshape(SHAPES[name]) for name in NAMES}


def run_records(frames: Sequence[Sequence[np.ndarray]], bit_depth: int, xdec: int = 1, ydec: int = 1) -> List[dict]:
    """The lag records of one run: one per frame but the first."""
    return [lags_pair(frames[t], frames[t - 1], bit_depth, xdec, ydec) for t in range(1, len(frames))]


def sum_records(records: Sequence[dict]) -> dict:
    """L5; an overflow of 64 bits raises OverflowError."""
    total = empty_record()
    for name in NAMES:
        flat = [sum(int(np.asarray(rec[name]).ravel()[j]) for rec in records) for j in range(max(int(np.prod(SHAPES[name])), 1))]
        lo, hi = (0, 2 ** 64 - 1) if DTYPES[name] is np.uint64 else (-(2 ** 63), 2 ** 63 - 1)
        if any(v < lo or v > hi for v in flat):
            raise OverflowError(name)
        total[name] = np.array(flat, DTYPES[name]).reshape(SHAPES[name])
    return total


def to_struct(rec: dict, dtype=LRECORD) -> np.ndarray:
    out = np.zeros((), dtype)
    for name in NAMES:
        out[name] = rec[name]
    return out


def mismatches(got, want: dict, what: str) -> List[str]:
    """Field-by-field comparison of a library record (structured array entry) with a reference record."""
    bad = []
    for name in NAMES:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append(f"{what}: {name} is {g.dtype} {g.shape}, want {w.dtype} {w.shape}")
            continue
        if not np.array_equal(g, w):
            for at in np.argwhere(g != w)[:4]:
                at = tuple(int(v) for v in at)
                bad.append(f"{what}: {name}{list(at)} = {g[at]}, want {w[at]}")
    return bad


# ---- rules L6 - L7: the AR fit, with the operations in the library's order (Python floats are f64) ----
TOO_FEW = "too few static sample pairs for a table"
SINGULAR_LUMA = "Solving latest noise equation system failed 0!"
TINY = 1.0e-16


def lag_index(dx: int, dy: int) -> int:
    if dy < 0 or (dy == 0 and dx < 0):
        dx, dy = -dx, -dy
    return 7 + 13 * (dy - 1) + dx + 6 if dy else dx


def causal_offsets(lag: int):
    return [(dx, dy) for dy in range(-lag, 1) for dx in range(-lag, lag + 1) if dy < 0 or dx < 0]


def ar_system(total: dict, c: int, bit_depth: int, lag: int, min_count: int = 0, *, remove_mean=True):
    """L6 - L7 up to the solve: (A, b, N), A a list of rows; ValueError with L6's refusal.  remove_mean = False is a wrong
    restatement."""
    nmin = min_count or 4096
    o = causal_offsets(lag)
    m = len(o)
    nc = m + (1 if c else 0)
    n0 = int(total["n"][c, 0])
    if n0 < nmin:
        raise ValueError(TOO_FEW)
    mean = float(int(total["s"][c])) / float(n0) if remove_mean else 0.0

    def C(dx, dy):
        i = lag_index(dx, dy)
        n = int(total["n"][c, i])
        if n < nmin:
            raise ValueError(TOO_FEW)
        return float(int(total["r"][c, i])) / float(n) - mean * mean

    den = float(1 << (2 * (bit_depth - 8))) * (255.0 * 255.0)
    N = float(n0)
    A = [[0.0] * nc for _ in range(nc)]
    b = [0.0] * nc
    for i in range(m):
        for j in range(m):
            A[i][j] = N * C(o[i][0] - o[j][0], o[i][1] - o[j][1]) / den
        b[i] = N * C(*o[i]) / den
    if c:
        ln = int(total["ln"])
        if ln < nmin:
            raise ValueError(TOO_FEW)
        mean_l = float(int(total["ls"])) / float(ln)
        var_l = float(int(total["l2"])) / float(ln) - mean_l * mean_l

        def X(dx, dy):
            j = CROSS.index((dx, dy))
            n = int(total["xn"][c - 1, j])
            if n < nmin:
                raise ValueError(TOO_FEW)
            return float(int(total["xr"][c - 1, j])) / float(n) - mean_l * mean

        for i in range(m):
            A[i][m] = A[m][i] = N * X(*o[i]) / den
        A[m][m] = N * var_l / den
        b[m] = N * X(0, 0) / den
    return A, b, n0


def gauss_solve(A, b):
    """The fold's elimination (bubble the larger magnitude up one row at a time); None when singular."""
    n = len(b)
    R = [list(row) for row in A]
    b = list(b)
    x = [0.0] * n
    for k in range(n - 1):
        for i in range(n - 1, k, -1):
            if abs(R[i - 1][k]) < abs(R[i][k]):
                R[i - 1], R[i] = R[i], R[i - 1]
                b[i], b[i - 1] = b[i - 1], b[i]
        pivot = R[k]
        if abs(pivot[k]) < TINY:
            return None
        pk, bk = pivot[k], b[k]
        for i in range(k, n - 1):
            row = R[i + 1]
            cc = row[k] / pk
            for j in range(k + 1, n):
                row[j] -= cc * pivot[j]
            b[i + 1] -= cc * bk
    for i in range(n - 1, -1, -1):
        row = R[i]
        if abs(row[i]) < TINY:
            return None
        cc = 0.0
        for j in range(i + 1, n):
            cc += row[j] * x[j]
        x[i] = (b[i] - cc) / row[i]
    return x


def noise_ar(total: dict, c: int, bit_depth: int, lag: int = 3, min_count: int = 0, **wrong):
    """L6 - L7: (x, gain) as g1s_nlf_ar gives them; ValueError with the refusal's text."""
    import math

    A, b, n0 = ar_system(total, c, bit_depth, lag, min_count, **wrong)
    nc = len(b)
    m = nc - (1 if c else 0)
    x = gauss_solve(A, b)
    if x is None:
        if not c:
            raise ValueError(SINGULAR_LUMA)
        x = [0.0] * nc  # the fold's chroma fallback
        if abs(A[m][m]) > 1e-6:
            x[m] = b[m] / A[m][m]
        return np.array(x), 1.0
    var = 0.0
    for i in range(m):
        var += A[i][i] / n0
    var /= m
    sum_covar = 0.0
    for i in range(m):
        bi = b[i]
        if c:
            bi -= A[i][nc - 1] * x[nc - 1]
        sum_covar += (bi * x[i]) / n0
    t = var - sum_covar
    noise_var = t if t > 1e-6 else 1e-6
    q = var / noise_var
    g = math.sqrt(q if q > 1e-6 else 1e-6)
    return np.array(x), (1.0 if 1 > g else g)


def format_noise_lags(total: dict, pairs: int, bit_depth: int, nplanes: int = 3, lag: int = 3, min_count: int = 0) -> bytes:
    """L10 (the grammar is in include/g1s_diff.h)."""
    import math

    def fmt(defined, v):
        return "%.4f" % v if defined else "-"

    nmin = min_count or 4096
    o = causal_offsets(lag)
    out = ["noiselags1", f"pairs {pairs} bit_depth {bit_depth} planes {nplanes} lag {lag}"]
    for c in range(nplanes):
        out.append(f"plane {c}")
        n0 = int(total["n"][c, 0])
        have0 = n0 >= nmin
        mean = float(int(total["s"][c])) / float(n0) if have0 else 0.0
        c0 = float(int(total["r"][c, 0])) / float(n0) - mean * mean if have0 else 0.0
        try:
            x, gain = noise_ar(total, c, bit_depth, lag, min_count)
        except ValueError:
            x, gain = None, None
        out.append(f"n0 {n0} sigma_t {fmt(have0, math.sqrt((c0 if c0 > 0.0 else 0.0) / 2.0))} gain {fmt(x is not None, gain or 0.0)}")
        for i, (dx, dy) in enumerate(o):
            k = lag_index(dx, dy)
            n = int(total["n"][c, k])
            ok = have0 and c0 > 0.0 and n >= nmin
            ci = float(int(total["r"][c, k])) / float(n) - mean * mean if ok else 0.0
            out.append(f"rho {i} {dx} {dy} {fmt(ok, ci / c0 if ok else 0.0)}")
        for i in range(len(o)):
            out.append(f"coef {i} {fmt(x is not None, x[i] if x is not None else 0.0)}")
        if c:
            out.append(f"luma {fmt(x is not None, x[len(o)] if x is not None else 0.0)}")
    return ("\n".join(out) + "\n").encode()
