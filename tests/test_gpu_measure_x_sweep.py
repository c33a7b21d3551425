"""A seeded, edge-weighted sweep of the cross meter in the manner of tests/test_gpu_measure_t_sweep.py (tests/sweep.py is not
edited).  The case list is drawn from numpy.random.default_rng([SEED, OP_ID]) as plain pasteable records, it is fixed, and its
SHA-256 is printed and pinned here; every cross record is compared field by field with tests/measure_x_ref.py, every ordinary
record with tests/measure_ref.py.  The sizes drawn round the tile are the CHROMA plane's (cw, ch): the luma size follows
from the subsampling, even or odd (odd = 1: the luma plane ends inside the last box, so that rule 12's clamp takes part)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import measure_ref as R
from tests import measure_x_ref as X
from tests import sweep as S
from tests.test_gpu_grain import _to_dev

SEED, N, CHUNKS = 17, 60, 3
OP_ID = len(S.OPS) + 2  # (len(S.OPS) and len(S.OPS) + 1 are the `measure` and the temporal sweep's)
TW, TH = 64, 128        # km_measure_x's chroma tile
DIGEST = "bad1097bf60ec97235477e328ebb00c75240c63606e94d92e89a92d1083bd4d0"

KINDS = [("noise", 3), ("small", 2), ("moved", 3), ("one_bin", 1.5), ("two_bins", 1.5), ("ramp", 1.5), ("extreme", 2)]
WHERE = [("device", 3), ("host", 2), ("mixed", 1)]
# the corner cases of tests/test_gpu_measure_x.py at the head
FORCED = [
    dict(cw=1, ch=1, odd=1, bd=8, ss="420", kind="noise", where="device", n=2, batch=1),
    dict(cw=TW, ch=TH, odd=0, bd=12, ss="444", kind="extreme", where="device", n=2, batch=2),
    dict(cw=TW + 1, ch=TH + 1, odd=1, bd=12, ss="420", kind="extreme", where="mixed", n=3, batch=2),
    dict(cw=2, ch=3, odd=1, bd=10, ss="422", kind="ramp", where="host", n=3, batch=2),
    dict(cw=2 * TW + 2, ch=2 * TH + 1, odd=1, bd=10, ss="420", kind="moved", where="device", n=1, batch=1),
    dict(cw=TW - 1, ch=TH - 1, odd=0, bd=8, ss="420", kind="two_bins", where="host", n=5, batch=4),
    dict(cw=4 * TW - 1, ch=2, odd=1, bd=8, ss="422", kind="one_bin", where="host", n=2, batch=3),
    dict(cw=3, ch=2 * TH - 1, odd=0, bd=12, ss="444", kind="small", where="device", n=5, batch=5),
]


def cases():
    rng = np.random.default_rng([SEED, OP_ID])
    out = []
    for i in range(N):
        if i < len(FORCED):
            c = dict(FORCED[i])
            c["wc"], c["hc"] = S._cls(c["cw"], TW), S._cls(c["ch"], TH)
        else:
            cw, wc = S._edge(rng, TW, 3, (4, 200))
            ch, hc = S._edge(rng, TH, 2, (4, 200))
            n = int(S._pick(rng, [(1, 2), (2, 3), (3, 2), (5, 1)]))
            c = dict(cw=cw, ch=ch, odd=int(rng.integers(0, 2)), bd=int(S._pick(rng, [(8, 1), (10, 1), (12, 1)])),
                     ss=S._pick(rng, [("420", 3), ("422", 1), ("444", 1)]), kind=S._pick(rng, KINDS), where=S._pick(rng, WHERE), n=n,
                     batch=int(S._pick(rng, [(1, 1), (2, 2), (4, 1), (n + 1, 1)])), wc=wc, hc=hc)
        out.append({"op": "measure_x", "i": i, **c, "forced": i < len(FORCED)})
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
    elif c["kind"] == "two_bins":
        luma = np.where(((xs >> 1) + (ys >> 1) + k) & 1, 9 * step, 10 * step)
    elif c["kind"] == "ramp":
        luma = (((xs >> 1) + 3 * (ys >> 1) + 7 * k) % 32) * step + ((ys + k) % step)
    else:
        luma = None
    noisy, clean = [], []
    moved = None
    for j, s in enumerate(shapes):
        if c["kind"] == "extreme":  # every residual +-top: one sign a plane (k even) or sign by parity / at random (k odd)
            if k % 2 == 0:
                b = np.full(s, top if (c["i"] + j + k // 2) & 1 else 0)
            elif j == 0:
                b = np.where(((np.arange(s[0])[:, None] + np.arange(s[1])[None, :]) & 1) == 1, top, 0)
            else:
                b = np.where(rng.integers(0, 2, s) > 0, top, 0)
            a = top - b
        elif c["kind"] == "moved":  # Cr is Cb moved by k + 1 samples right and k down; luma is noise
            b = rng.integers(top // 4, top - top // 4, s)
            if j == 0:
                d = rng.integers(-(top // 4), top // 4 + 1, s)
            elif j == 1:
                d = moved = rng.integers(-(top // 4), top // 4 + 1, s)
            else:
                d = np.roll(moved, (k % 3, (k + 1) % 3), (0, 1))
            a = b + d
        else:
            b = luma if (j == 0 and luma is not None) else rng.integers(0, top + 1, s)
            amp = 12 if c["kind"] == "small" else top
            a = np.clip(b + rng.integers(-amp, amp + 1, s), 0, top)
        noisy.append(np.ascontiguousarray(a.astype(dt)))
        clean.append(np.ascontiguousarray(b.astype(dt)))
    return noisy, clean


def test_the_case_list_is_fixed_and_covers_its_axes():
    cl = cases()
    print("measure_x sweep: %d cases, sha256 %s" % (len(cl), S.digest(cl)))
    assert cl == cases() and eval(repr(cl[9])) == cl[9]
    assert S.digest(cl) == DIGEST, S.digest(cl)
    for axis, need in (("wc", {"ku-1", "ku", "ku+1", "uni"}), ("hc", {"ku-1", "ku", "ku+1", "uni"}), ("bd", {8, 10, 12}),
                       ("ss", {"420", "422", "444"}), ("kind", {k for k, _ in KINDS}), ("where", {k for k, _ in WHERE}), ("n", {1, 2, 3, 5}),
                       ("odd", {0, 1})):
        assert need <= {c[axis] for c in cl}, axis
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
        m = meters.setdefault((c["bd"], c["batch"]), None) or GrainMeter(c["bd"], batch_frames=c["batch"], cross=True)
        meters[(c["bd"], c["batch"])] = m
        pairs, keep = [], []
        for k in range(c["n"]):
            noisy, clean = pair_of(c, k)
            pairs.append((noisy, clean))
            dev = c["where"] == "device" or (c["where"] == "mixed" and k % 2 == 0)
            keep.append((_to_dev(noisy, c["bd"]) if dev else noisy, _to_dev(clean, c["bd"]) if dev or c["where"] == "mixed" else clean))
            m.measure(keep[-1][0], keep[-1][1], subx, suby)
        got = m.finish_cross()
        assert len(got) == c["n"], c
        for k, (noisy, clean) in enumerate(pairs):
            bad = X.mismatches(got[k], X.cross_frame(noisy, clean, c["bd"], subx, suby), f"record {k}")
            assert not bad, repr(c) + "\n" + "\n".join(bad)
        got = m.finish()
        assert len(got) == c["n"], c
        for k, (noisy, clean) in enumerate(pairs):
            bad = R.mismatches(got[k], R.measure_frame(noisy, clean, c["bd"], subx, suby), f"frame {k}")
            assert not bad, repr(c) + "\n" + "\n".join(bad)
    for m in meters.values():
        m.close()
