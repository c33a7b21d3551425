"""Shared helpers for the parity tests (test infrastructure)."""
from __future__ import annotations

from fractions import Fraction
from typing import List, Sequence

import numpy as np

from grav1synth_amd.synth import SynthSpec, make_pair
from tests.oracle_binding import OracleDiff, format_tbl as oracle_format_tbl


def np_pair(spec: SynthSpec, frame: int):
    s, d = make_pair(spec, frame)
    return [p.numpy() for p in s], [p.numpy() for p in d]


def oracle_run(spec: SynthSpec, frames: Sequence[int], lag=3, chroma=True, fps=Fraction(24, 1),
               specs_per_frame=None, collect=None):
    """Run the CPU oracle over synthetic frames; returns (.tbl bytes, segments).
    `collect(oracle, frame_index)` is called after each frame when given."""
    o = OracleDiff(fps.numerator, fps.denominator, spec.bit_depth, spec.bit_depth, lag, chroma)
    for k, f in enumerate(frames):
        sp = specs_per_frame[k] if specs_per_frame else spec
        s, d = np_pair(sp, f)
        if not chroma:
            s, d = s[:1], d[:1]
        o.diff_frame(s, d, sp.xdec, sp.ydec)
        if collect:
            collect(o, k)
    segs = o.finish()
    return oracle_format_tbl(segs), segs


def record_from_oracle(o: OracleDiff, spec, lag: int, nplanes: int):
    """Assemble a product record from the oracle's exact integer shadows.  `spec`: a SynthSpec, or the geometry alone as
    (width, height, xdec, ydec)."""
    from grav1synth_amd.diff import Record

    width, height, xdec, ydec = spec if isinstance(spec, tuple) else (spec.width, spec.height, spec.xdec, spec.ydec)
    r = Record.blank(width, height, xdec, ydec, nplanes, lag)
    for c in range(nplanes):
        v = r.views(c)
        S, Sb, nobs = o.ar_sums(c)
        v["S"][:] = S
        v["Sb_nobs"][:-1] = Sb
        v["Sb_nobs"][-1] = nobs
        ls, sd, sd2 = o.block_stats(c)
        if c == 0:
            v["luma_sum"][:] = ls
            v["mask"][:] = o.flat_mask().ravel()
            v["scores"][:] = o.scores().ravel()
        v["sum_d"][:] = sd
        v["sum_d2"][:] = sd2
    return r


def oracle_shadow(o: OracleDiff, nplanes: int) -> dict:
    """The oracle's integer shadows of the frame it has just taken, copied out: what a record is compared with."""
    return dict(mask=o.flat_mask(), scores=o.scores(), ar=[o.ar_sums(c) for c in range(nplanes)],
                stats=[o.block_stats(c) for c in range(nplanes)])


def record_mismatches(shadow: dict, r, where: str) -> List[str]:
    """Every field of record `r` against an oracle_shadow: mask bytes, f32 score bits, S, Sb and nobs of every plane, and
    luma_sum, sum_d, sum_d2 on the blocks the oracle measured.  Returns one line per field that differs, led by `where`."""
    out = []
    om, rm = shadow["mask"], r.flat_mask()
    if not np.array_equal(om, rm):
        out.append(f"{where}: flat mask differs at {np.argwhere(om != rm)[:5].tolist()}")
    osc, rsc = shadow["scores"], r.scores()
    if not np.array_equal(osc.view(np.uint32), rsc.view(np.uint32)):
        out.append(f"{where}: score bits differ ({(osc.view(np.uint32) != rsc.view(np.uint32)).sum()} blocks)")
    flat = om.ravel() != 0
    for c in range(len(shadow["ar"])):
        S, Sb, nobs = shadow["ar"][c]
        S2, Sb2, nobs2 = r.ar_sums(c)
        if nobs != nobs2 or not np.array_equal(S, S2) or not np.array_equal(Sb, Sb2):
            fields = [n for n, bad in (("nobs", nobs != nobs2), ("S", not np.array_equal(S, S2)), ("Sb", not np.array_equal(Sb, Sb2))) if bad]
            out.append(f"{where} plane {c}: AR sums differ: {', '.join(fields)} (nobs {nobs} vs {nobs2})")
        ls, sd, sd2 = shadow["stats"][c]
        ls2, sd_2, sd2_2 = r.block_stats(c)
        # the oracle records statistics only for blocks it measures (flat, > 32 samples)
        # (per plane: a chroma corner block of <= 32 samples is skipped while its luma block is measured)
        meas = flat & ((sd2 != 0) | (sd != 0) | ((ls != 0) if c == 0 else False))
        if c == 0 and not np.array_equal(ls[meas], ls2[meas]):
            out.append(f"{where}: luma block sums differ (luma_sum, first at block {int(np.flatnonzero(meas & (ls != ls2))[0])})")
        if not np.array_equal(sd[meas], sd_2[meas]) or not np.array_equal(sd2[meas], sd2_2[meas]):
            fields = [n for n, bad in (("sum_d", not np.array_equal(sd[meas], sd_2[meas])), ("sum_d2", not np.array_equal(sd2[meas], sd2_2[meas]))) if bad]
            bad = np.flatnonzero(meas & ((sd != sd_2) | (sd2 != sd2_2)))
            out.append(f"{where} plane {c}: block noise sums differ: {', '.join(fields)} ({bad.size} blocks, first {int(bad[0])})")
    return out
