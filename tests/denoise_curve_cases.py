"""The seeded, edge-weighted case list of the grain prior's sweep (tests/test_gpu_denoise_curve_sweep.py), in the style of
tests/sweep.py and with its menus.  The edges are kd_curve's: a lane takes 16 samples a step, so the luma width is drawn
around multiples of 16 (and the first 1024 samples, a wave's step, are forced), the rows around the 32 of a workgroup's
strip; the row's alignment is drawn too -- a contiguous tensor, or a view with a pitch and a base offset (tests/views.py)
that takes the sample-by-sample path.  Clip lengths are drawn around the temporal window and the batch as denoise_t's are.
Plain records: a failing one prints whole and can be pasted back into run_cases."""
from __future__ import annotations

from typing import List

import numpy as np

from tests import sweep as S

SEED, CASES, CHUNKS = 15, 48, 3
OP_ID = 101  # (beside tests/sweep.py's operations and the joint sweep's 100)
POOL = 8

CURVES = ("flat", "step", "example", "ramp")


def curve_points(name: str):
    """The luma scaling points of each segment of a case's prior, and its range R (0 = the default)."""
    import os

    from grav1synth_amd.tbl import parse_tbl

    if name == "flat":
        return [[(0, 10), (127, 10), (128, 200), (255, 200)]], 1
    if name == "step":  # two levels, the largest range (the caller passes the depth's bound)
        return [[(0, 10), (127, 10), (128, 200), (255, 200)]], -1
    if name == "ramp":
        return [[(0, 20), (255, 80)], [(0, 24), (100, 40), (255, 90)]], 0
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference-example-table.tbl")
    return [s.scaling_points_y for s in parse_tbl(open(path, "rb").read())], 0


def _pool(rng) -> List[dict]:
    """POOL parameter sets, every entry of every menu among them (tests/sweep.py's _dn_pool, for the depths a prior takes)."""
    def column(menu):
        vals = [m[0] for m in menu]
        col = [vals[i] for i in rng.permutation(len(vals))][:POOL]
        return col + [S._pick(rng, menu) for _ in range(POOL - len(col))]

    A, S_ = column([(1, 2), (2, 2), (3, 2), (5, 1), (7, 1)]), column([(1, 2), (2, 2), (3, 1), (4, 1)])
    h, hc, bd = column(S.STRENGTHS), column(S.STRENGTHS), column([(8, 1), (10, 1)])
    D, batch = column([(0, 2), (1, 2), (2, 2), (3, 1)]), column([(1, 1), (2, 1), (3, 1), (4, 1), (5, 1)])
    joint, curve = column([(False, 2), (True, 1)]), column([(c, 1) for c in CURVES])
    return [dict(bd=int(bd[i]), A=int(A[i]), S=int(S_[i]), strength=float(h[i]), chroma_strength=float(hc[i]), D=int(D[i]), batch=int(batch[i]),
                 joint=bool(joint[i]), curve=str(curve[i])) for i in range(POOL)]


def _dc(w, h, bd, ss, A, S_, D, n, batch, nc, curve, joint=False, strength=4.0, chroma_strength=4.0, kind="grainy", split=-1, split_kind="none",
        view="none") -> dict:
    return dict(w=w, h=h, wc=S._cls(w, 16), hc=S._cls(h, 32), pool=-1, bd=bd, ss=ss, A=A, S=S_, strength=strength, chroma_strength=chroma_strength,
                kind=kind, cseed=w * 977 + h + D, D=D, nframes=n, nc=nc, batch=batch, split=split, split_kind=split_kind, curve=curve, joint=joint, view=view)


FORCED = [
    _dc(1025, 33, 10, "420", 1, 1, 0, 1, 2, "1", "step", kind="noise"), _dc(1024, 32, 8, "mono", 2, 2, 1, 3, 2, "2D+1", "example", kind="gradient"),
    _dc(1023, 31, 8, "444", 1, 4, 2, 3, 1, "D+1", "ramp", True, 0.05, 60.0), _dc(1, 1, 10, "420", 3, 2, 1, 2, 2, "2D", "flat", view="both"),
    _dc(17, 65, 10, "422", 7, 1, 0, 2, 3, "b-1", "step", True, 60.0, 1000.0, "noise", view="in"), _dc(2049, 3, 8, "mono", 1, 1, 3, 7, 3, "2D+1", "ramp", kind="const", view="out"),
    _dc(66, 50, 8, "420", 2, 2, 1, 4, 2, "2D+2", "example", True, split=2, split_kind="geometry"), _dc(15, 2, 10, "mono", 5, 3, 2, 5, 4, "2D+1", "step", split=3, split_kind="sync", view="both"),
]


def cases(seed: int = SEED, n: int = CASES) -> List[dict]:
    rng = np.random.default_rng([seed, OP_ID])
    pool = _pool(rng)
    out = []
    while len(out) < n:
        i = len(out)
        if i < len(FORCED):
            out.append({"op": "denoise_c", "i": i, **FORCED[i], "forced": True})
            continue
        w, wc = S._edge(rng, 16, 9, (4, 200))
        h, hc = S._edge(rng, 32, 2, (4, 100))
        k = int(rng.integers(0, len(pool)))
        p = pool[k]
        ss = S._pick(rng, [("420", 3), ("422", 1), ("444", 2), ("mono", 2)])
        D, batch = p["D"], p["batch"]
        nc = S._pick(rng, [("1", 1), ("D", 1), ("D+1", 1.5), ("2D", 1), ("2D+1", 1.5), ("2D+2", 1), ("b-1", 1), ("b+1", 1)])
        nfr = max({"1": 1, "D": D, "D+1": D + 1, "2D": 2 * D, "2D+1": 2 * D + 1, "2D+2": 2 * D + 2, "b-1": batch - 1, "b+1": batch + 1}[nc], 1)
        split, split_kind = -1, "none"
        if nfr >= 2:
            split_kind = S._pick(rng, [("none", 3), ("sync", 1), ("geometry", 1)])
            if split_kind != "none":
                split = int(rng.integers(1, nfr))
        c = _dc(w, h, p["bd"], ss, p["A"], p["S"], D, nfr, batch, nc, p["curve"], p["joint"], p["strength"], p["chroma_strength"], S._pick(rng, S.DN_KINDS),
                split, split_kind, S._pick(rng, [("none", 3), ("in", 1), ("out", 1), ("both", 1)]))
        c.update(wc=wc, hc=hc, pool=k, cseed=int(rng.integers(0, 1 << 30)))
        if S._dn_budget(c, nfr, min(2 * D + 1, nfr)) > 2.5e7:  # (what the numpy reference pays; drawn again)
            continue
        out.append({"op": "denoise_c", "i": i, **c, "forced": False})
    return out
