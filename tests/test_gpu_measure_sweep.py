"""A seeded, edge-weighted sweep of `measure` in the manner of tests/sweep.py (which is not edited: its SUITE and its CPU test
stay as they are).  The case list is drawn from numpy.random.default_rng([SEED, OP_ID]) as plain pasteable records, it is
fixed, and its SHA-256 is printed and pinned here; every record is compared field by field with tests/measure_ref.py."""
from __future__ import annotations

import numpy as np
import pytest

from tests import measure_ref as R
from tests import sweep as S
from tests.test_gpu_grain import _to_dev

SEED, N, CHUNKS = 12, 60, 3
OP_ID = len(S.OPS)  # the first id tests/sweep.py does not use
TW, TH = 64, 128    # km_measure's tile
DIGEST = "8693b8cc574fd4b816b7e2a32415b6387954dbe8c21db808e4da51b73e5e6ce4"

KINDS = [("noise", 3), ("small", 3), ("one_bin", 1.5), ("two_bins", 1.5), ("ramp", 1.5), ("extreme", 1)]
WHERE = [("device", 3), ("host", 1), ("mixed", 1)]
FORCED = [
    dict(w=1, h=1, bd=8, ss="420", kind="noise", where="device", n=1, batch=1),
    dict(w=TW, h=TH, bd=12, ss="444", kind="extreme", where="device", n=1, batch=2),
    dict(w=TW + 1, h=TH + 1, bd=10, ss="420", kind="two_bins", where="mixed", n=3, batch=2),
    dict(w=3, h=2 * TH - 1, bd=10, ss="422", kind="ramp", where="host", n=2, batch=2),
    dict(w=4 * TW - 1, h=3, bd=8, ss="mono", kind="one_bin", where="device", n=5, batch=4),
    dict(w=2, h=2, bd=12, ss="422", kind="small", where="host", n=1, batch=1),
]


def cases():
    rng = np.random.default_rng([SEED, OP_ID])
    out = []
    for i in range(N):
        if i < len(FORCED):
            c = dict(FORCED[i])
            c["wc"], c["hc"] = S._cls(c["w"], TW), S._cls(c["h"], TH)
        else:
            w, wc = S._edge(rng, TW, 4, (4, 300))
            h, hc = S._edge(rng, TH, 2, (4, 300))
            c = dict(w=w, h=h, bd=int(S._pick(rng, [(8, 1), (10, 1), (12, 1)])), ss=S._pick(rng, [("420", 3), ("422", 1), ("444", 1), ("mono", 1)]),
                     kind=S._pick(rng, KINDS), where=S._pick(rng, WHERE), n=int(S._pick(rng, [(1, 3), (2, 1), (3, 1), (5, 1)])),
                     batch=int(S._pick(rng, [(1, 1), (2, 2), (4, 1)])), wc=wc, hc=hc)
        out.append({"op": "measure", "i": i, **c, "forced": i < len(FORCED)})
    return out


def pair_of(c: dict, k: int):
    """(noisy, clean) of frame k of a case (numpy only)."""
    rng = np.random.default_rng([SEED, c["i"], k])
    bd, top = c["bd"], (1 << c["bd"]) - 1
    subx, suby = S.SUBSAMPLINGS[c["ss"]]
    dt = np.uint8 if bd == 8 else np.uint16
    shapes = [(c["h"], c["w"])] + ([] if c["ss"] == "mono" else [((c["h"] + suby) >> suby, (c["w"] + subx) >> subx)] * 2)
    step = 1 << (bd - 5)
    noisy, clean = [], []
    for j, s in enumerate(shapes):
        ys, xs = np.arange(s[0])[:, None], np.arange(s[1])[None, :]
        if c["kind"] == "one_bin":
            b = np.full(s, (5 + k) * step + j)
        elif c["kind"] == "two_bins":
            b = np.where((xs + ys + k) & 1, 9 * step, 10 * step - 1)
        elif c["kind"] == "ramp":
            b = ((xs + 3 * ys + k) % 32) * step + (ys % step)
        elif c["kind"] == "extreme":
            b = np.where(rng.integers(0, 2, s) > 0, top, 0)
        else:
            b = rng.integers(0, top + 1, s)
        amp = 12 if c["kind"] == "small" else top
        a = top - b if c["kind"] == "extreme" else np.clip(b + rng.integers(-amp, amp + 1, s), 0, top)
        noisy.append(np.ascontiguousarray(a.astype(dt)))
        clean.append(np.ascontiguousarray(b.astype(dt)))
    return noisy, clean


def test_the_case_list_is_fixed_and_covers_its_axes():
    cl = cases()
    print("measure sweep: %d cases, sha256 %s" % (len(cl), S.digest(cl)))
    assert cl == cases() and eval(repr(cl[7])) == cl[7]
    assert S.digest(cl) == DIGEST, S.digest(cl)
    for axis, need in (("wc", {"ku-1", "ku", "ku+1", "uni"}), ("hc", {"ku-1", "ku", "ku+1", "uni"}), ("bd", {8, 10, 12}),
                       ("ss", {"420", "422", "444", "mono"}), ("kind", {k for k, _ in KINDS}), ("where", {k for k, _ in WHERE})):
        assert need <= {c[axis] for c in cl}, axis


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_sweep_equals_the_reference(chunk):
    from grav1synth_amd.measure import GrainMeter

    meters = {}
    for c in S.chunk_of(cases(), chunk, CHUNKS):
        subx, suby = S.SUBSAMPLINGS[c["ss"]]
        m = meters.setdefault((c["bd"], c["batch"]), None) or GrainMeter(c["bd"], batch_frames=c["batch"])
        meters[(c["bd"], c["batch"])] = m
        wants = []
        for k in range(c["n"]):
            noisy, clean = pair_of(c, k)
            wants.append(R.measure_frame(noisy, clean, c["bd"], subx, suby))
            dev = c["where"] == "device" or (c["where"] == "mixed" and k % 2 == 0)
            m.measure(_to_dev(noisy, c["bd"]) if dev else noisy, _to_dev(clean, c["bd"]) if dev or c["where"] == "mixed" else clean, subx, suby)
        got = m.finish()
        assert len(got) == c["n"], c
        for k in range(c["n"]):
            bad = R.mismatches(got[k], wants[k], f"frame {k}")
            assert not bad, repr(c) + "\n" + "\n".join(bad)
    for m in meters.values():
        m.close()
