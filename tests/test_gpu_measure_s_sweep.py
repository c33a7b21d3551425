"""A seeded, edge-weighted sweep of the scales meter in the manner of tests/test_gpu_measure_x_sweep.py (tests/sweep.py is not
edited).  The case list is drawn from numpy.random.default_rng([SEED, OP_ID]) as plain pasteable records, it is fixed, and its
SHA-256 is printed and pinned here; every scale record is compared field by field with tests/measure_s_ref.py, every ordinary
record with tests/measure_ref.py.  The sizes drawn are the CHROMA plane's (cw, ch), weighted to one below, on and one above 32,
km_measure's tile (64 x 128) and twice the tile; the luma size follows from the subsampling, even or odd (odd = 1: the luma
plane ends inside the last chroma sample, so that rule 2's clamp takes part)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import measure_ref as R
from tests import measure_s_ref as MS
from tests import sweep as S
from tests.test_gpu_grain import _to_dev

SEED, N, CHUNKS = 24, 60, 3
OP_ID = len(S.OPS) + 3  # (len(S.OPS) .. len(S.OPS) + 2 are the `measure`, the temporal and the cross sweep's)
TW, TH = 64, 128        # km_measure's tile: the unit of km_measure_s's bands and strips
DIGEST = "0cfb0a97e66339a0a0aa7288b04ce906cceda39e51a2dd6e35588409c637f046"

KINDS = [("noise", 3), ("small", 2), ("cells", 3), ("one_bin", 1.5), ("two_bins", 2), ("edge", 2), ("ramp", 1.5), ("extreme", 2)]
WHERE = [("device", 3), ("host", 2), ("mixed", 1)]
# the corner cases of tests/test_gpu_measure_s.py at the head
FORCED = [
    dict(cw=1, ch=1, odd=1, bd=8, ss="420", kind="noise", where="device", n=2, batch=1),
    dict(cw=TW, ch=TH, odd=0, bd=12, ss="444", kind="extreme", where="device", n=2, batch=2),
    dict(cw=TW + 1, ch=TH + 1, odd=1, bd=12, ss="420", kind="extreme", where="mixed", n=3, batch=2),
    dict(cw=31, ch=33, odd=1, bd=10, ss="422", kind="ramp", where="host", n=3, batch=2),
    dict(cw=2 * TW + 1, ch=2 * TH + 1, odd=1, bd=10, ss="420", kind="cells", where="device", n=5, batch=1),
    dict(cw=33, ch=31, odd=0, bd=8, ss="420", kind="two_bins", where="host", n=5, batch=4),
    dict(cw=32, ch=32, odd=1, bd=8, ss="422", kind="edge", where="host", n=2, batch=3),
    dict(cw=3, ch=2 * TH - 1, odd=0, bd=12, ss="444", kind="small", where="device", n=5, batch=5),
]
WIDTHS = [(31, 2), (32, 2), (33, 2), (TW - 1, 2), (TW, 2), (TW + 1, 2), (2 * TW - 1, 2), (2 * TW, 2), (2 * TW + 1, 2), ("uni", 4), (1, 0.5), (2, 0.5), (3, 0.5)]
HEIGHTS = [(31, 2), (32, 2), (33, 2), (TH - 1, 2), (TH, 2), (TH + 1, 2), (2 * TH - 1, 2), (2 * TH, 2), (2 * TH + 1, 2), ("uni", 4), (1, 0.5), (2, 0.5), (3, 0.5)]


def _size(rng, menu, hi):
    v = S._pick(rng, menu)
    return (int(rng.integers(4, hi + 1)), "uni") if v == "uni" else (int(v), "edge" if v > 3 else str(v))


def cases():
    rng = np.random.default_rng([SEED, OP_ID])
    out = []
    for i in range(N):
        if i < len(FORCED):
            c = dict(FORCED[i], wc="forced", hc="forced")
        else:
            cw, wc = _size(rng, WIDTHS, 2 * TW + 40)
            ch, hc = _size(rng, HEIGHTS, 2 * TH + 40)
            n = int(S._pick(rng, [(1, 2), (2, 3), (3, 2), (5, 1)]))
            c = dict(cw=cw, ch=ch, odd=int(rng.integers(0, 2)), bd=int(S._pick(rng, [(8, 1), (10, 1), (12, 1)])),
                     ss=S._pick(rng, [("420", 3), ("422", 1), ("444", 1)]), kind=S._pick(rng, KINDS), where=S._pick(rng, WHERE), n=n,
                     batch=int(S._pick(rng, [(1, 1), (2, 2), (4, 1), (n + 1, 1)])), wc=wc, hc=hc)
        out.append({"op": "measure_s", "i": i, **c, "forced": i < len(FORCED)})
    return out


def luma_size(c: dict):
    subx, suby = S.SUBSAMPLINGS[c["ss"]]
    return (c["cw"] << subx) - (subx and c["odd"]), (c["ch"] << suby) - (suby and c["odd"])


def pair_of(c: dict, k: int):
    """(noisy, clean) of frame k of a case (numpy only)."""
    rng = np.random.default_rng([SEED, c["i"], k])
    bd, top = c["bd"], (1 << c["bd"]) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    w, h = luma_size(c)
    shapes = [(h, w)] + [(c["ch"], c["cw"])] * 2
    step = 1 << (bd - 5)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    if c["kind"] == "one_bin":
        luma = np.full((h, w), (5 + k) * step + 1)
    elif c["kind"] == "two_bins":  # two distant bins sample by sample (k even) or chroma sample by chroma sample: boxes in a third
        sh = k & 1
        luma = np.where(((xs >> sh) + (ys >> sh)) & 1, 22 * step + 1, 6 * step + 1)
    elif c["kind"] == "edge":  # three samples on a bin's lower edge and one below it (k even); e - 1, e by columns (k odd)
        e = (9 + k) * step
        luma = np.where((xs & ys & 1) == 1, e - 1, e) if k % 2 == 0 else e - 1 + (xs & 1) + 0 * ys
    elif c["kind"] == "ramp":
        luma = (((xs >> 1) + 3 * (ys >> 1) + 7 * k) % 32) * step + ((ys + k) % step)
    else:
        luma = None
    noisy, clean = [], []
    for j, s in enumerate(shapes):
        py, px = np.arange(s[0])[:, None], np.arange(s[1])[None, :]
        if c["kind"] == "extreme":  # every residual +-top: one sign a plane (k even) or sign by cells of 4 / at random (k odd)
            if k % 2 == 0:
                b = np.full(s, top if (c["i"] + j + k // 2) & 1 else 0)
            elif j == 0:
                b = np.where((((px >> 2) + (py >> 2)) & 1) == 1, top, 0)
            else:
                b = np.where(rng.integers(0, 2, s) > 0, top, 0)
            a = top - b
        elif c["kind"] == "cells":  # +-amp on a checkerboard of 2^k x 2^k cells on a flat frame: scale k and below, nothing above
            b = np.full(s, top // 2)
            a = b + np.where(((px >> k) + (py >> k)) & 1, -(3 + j), 3 + j)
        else:
            b = luma if (j == 0 and luma is not None) else rng.integers(0, top + 1, s)
            amp = 12 if c["kind"] in ("small", "two_bins", "edge") else top
            a = np.clip(b + rng.integers(-amp, amp + 1, s), 0, top)
        noisy.append(np.ascontiguousarray(a.astype(dt)))
        clean.append(np.ascontiguousarray(b.astype(dt)))
    return noisy, clean


def test_the_case_list_is_fixed_and_covers_its_axes():
    cl = cases()
    print("measure_s sweep: %d cases, sha256 %s" % (len(cl), S.digest(cl)))
    assert len(cl) == N and cl == cases() and eval(repr(cl[9])) == cl[9]
    assert S.digest(cl) == DIGEST, S.digest(cl)
    for axis, need in (("wc", {"edge", "uni"}), ("hc", {"edge", "uni"}), ("bd", {8, 10, 12}), ("ss", {"420", "422", "444"}),
                       ("kind", {k for k, _ in KINDS}), ("where", {k for k, _ in WHERE}), ("n", {1, 2, 3, 5}), ("odd", {0, 1})):
        assert need <= {c[axis] for c in cl}, axis
    for unit in (32, TW, 2 * TW):
        assert {unit - 1, unit, unit + 1} <= {c["cw"] for c in cl}, unit
    for unit in (32, TH, 2 * TH):
        assert {unit - 1, unit, unit + 1} <= {c["ch"] for c in cl}, unit
    assert any(c["batch"] == c["n"] + 1 for c in cl) and any(c["batch"] == 1 and c["n"] > 2 for c in cl)
    for c in cl[:12]:  # the planes have the sizes the case names, and the samples stay inside the bit depth
        for k in range(c["n"]):
            noisy, clean = pair_of(c, k)
            assert clean[1].shape == (c["ch"], c["cw"]) and all(int(p.max()) <= (1 << c["bd"]) - 1 for p in noisy + clean)
            subx, suby = S.SUBSAMPLINGS[c["ss"]]
            assert ((clean[0].shape[1] + subx) >> subx, (clean[0].shape[0] + suby) >> suby) == (c["cw"], c["ch"])


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_sweep_equals_the_restatement(chunk):
    from grav1synth_amd.measure import GrainMeter

    meters = {}
    for c in S.chunk_of(cases(), chunk, CHUNKS):
        subx, suby = S.SUBSAMPLINGS[c["ss"]]
        m = meters.setdefault((c["bd"], c["batch"]), None) or GrainMeter(c["bd"], batch_frames=c["batch"], scales=True)
        meters[(c["bd"], c["batch"])] = m
        pairs, keep = [], []
        for k in range(c["n"]):
            noisy, clean = pair_of(c, k)
            pairs.append((noisy, clean))
            dev = c["where"] == "device" or (c["where"] == "mixed" and k % 2 == 0)
            keep.append((_to_dev(noisy, c["bd"]) if dev else noisy, _to_dev(clean, c["bd"]) if dev or c["where"] == "mixed" else clean))
            m.measure(keep[-1][0], keep[-1][1], subx, suby)
        got = m.finish_scales()
        assert len(got) == c["n"], c
        for k, (noisy, clean) in enumerate(pairs):
            bad = MS.mismatches(got[k], MS.scale_frame(noisy, clean, c["bd"], subx, suby), f"record {k}")
            assert not bad, repr(c) + "\n" + "\n".join(bad)
        got = m.finish()
        assert len(got) == c["n"], c
        for k, (noisy, clean) in enumerate(pairs):
            bad = R.mismatches(got[k], R.measure_frame(noisy, clean, c["bd"], subx, suby), f"frame {k}")
            assert not bad, repr(c) + "\n" + "\n".join(bad)
    for m in meters.values():
        m.close()
