"""A seeded, edge-weighted sweep of the noise level function in the manner of tests/sweep.py (which is not edited: its SUITE
and its CPU test stay as they are).  The case list is drawn from numpy.random.default_rng([SEED, OP_ID]) as plain pasteable
records, it is fixed, and its SHA-256 is printed and pinned here; every record is compared field by field with
tests/nlf_ref.py.  The edges are k_nlf's: 496 output columns and 32 output rows a wave's strip."""
from __future__ import annotations

import numpy as np
import pytest

from tests import nlf_ref as R
from tests import sweep as S
from tests.test_gpu_grain import _to_dev

SEED, N, CHUNKS = 12, 60, 3
OP_ID = 102  # (beside tests/sweep.py's operations, the joint sweep's 100 and the grain prior's 101)
SW, SH = 496, 32
DIGEST = "dae02f182db19dc54824603dfd1689150f36910b7a6a43833423ddf74cbb11d7"

KINDS = [("smooth", 3), ("noisy", 2), ("one_bin", 1.5), ("two_bins", 1.5), ("ramp", 1.5), ("checker", 1), ("wild", 1)]
WHERE = [("device", 3), ("host", 1), ("mixed", 1)]
FORCED = [
    dict(w=1, h=1, bd=8, ss="420", kind="smooth", where="device", n=1, batch=1),
    dict(w=SW + 1, h=SH + 2, bd=12, ss="444", kind="checker", where="device", n=1, batch=2),
    dict(w=SW + 2, h=SH + 3, bd=10, ss="420", kind="two_bins", where="mixed", n=3, batch=2),
    dict(w=3, h=2 * SH + 1, bd=10, ss="422", kind="ramp", where="host", n=2, batch=2),
    dict(w=2 * SW + 1, h=3, bd=8, ss="mono", kind="one_bin", where="device", n=5, batch=4),
    dict(w=2, h=2, bd=12, ss="422", kind="noisy", where="host", n=1, batch=1),
    dict(w=2 * (SW + 1) + 1, h=2 * (SH + 2) + 1, bd=10, ss="420", kind="noisy", where="device", n=2, batch=1),
]


def cases():
    rng = np.random.default_rng([SEED, OP_ID])
    out = []
    for i in range(N):
        if i < len(FORCED):
            c = dict(FORCED[i])
            c["wc"], c["hc"] = S._cls(c["w"], SW, plus2=True), S._cls(c["h"], SH, plus2=True)
        else:
            w, wc = S._edge(rng, SW, 2, (4, 700), plus2=True)
            h, hc = S._edge(rng, SH, 3, (4, 120), plus2=True)
            c = dict(w=w, h=h, bd=int(S._pick(rng, [(8, 1), (10, 1), (12, 1)])), ss=S._pick(rng, [("420", 3), ("422", 1), ("444", 1), ("mono", 1)]),
                     kind=S._pick(rng, KINDS), where=S._pick(rng, WHERE), n=int(S._pick(rng, [(1, 3), (2, 1), (3, 1), (5, 1)])),
                     batch=int(S._pick(rng, [(1, 1), (2, 2), (4, 1)])), wc=wc, hc=hc)
        out.append({"op": "nlf", "i": i, **c, "forced": i < len(FORCED)})
    return out


def frame_of(c: dict, k: int):
    """The planes of frame k of a case (numpy only)."""
    rng = np.random.default_rng([SEED, c["i"], k])
    bd, top = c["bd"], (1 << c["bd"]) - 1
    subx, suby = S.SUBSAMPLINGS[c["ss"]]
    dt = np.uint8 if bd == 8 else np.uint16
    shapes = [(c["h"], c["w"])] + ([] if c["ss"] == "mono" else [((c["h"] + suby) >> suby, (c["w"] + subx) >> subx)] * 2)
    step, up = 1 << (bd - 5), 1 << (bd - 8)
    planes = []
    for j, s in enumerate(shapes):
        ys, xs = np.arange(s[0])[:, None], np.arange(s[1])[None, :]
        small = rng.integers(-2 * up, 2 * up + 1, s)
        if c["kind"] == "one_bin":
            p = np.full(s, (5 + k) * step + j) + 0 * small
        elif c["kind"] == "two_bins":  # (the box mean is 8 step - 1 around an A and 8 step around a B)
            p = np.where((xs + ys + k) & 1, 8 * step - 5, 8 * step + 4) + 0 * small
        elif c["kind"] == "ramp":
            p = ((xs * (1 + j) + 2 * ys + 7 * k) * up) % (top + 1) + small
        elif c["kind"] == "checker":
            p = np.where((xs + ys + j) & 1, top, 0) + 0 * small
        elif c["kind"] == "wild":
            p = rng.integers(0, top + 1, s)
        elif c["kind"] == "noisy":
            p = (40 + 50 * j + 30 * k) * up + np.rint(rng.standard_normal(s) * 6 * up).astype(np.int64)
        else:
            p = ((xs + ys) // 3 + 20 * j) * up + small
        planes.append(np.ascontiguousarray(np.clip(p, 0, top).astype(dt)))
    return planes


def test_the_case_list_is_fixed_and_covers_its_axes():
    cl = cases()
    print("nlf sweep: %d cases, sha256 %s" % (len(cl), S.digest(cl)))
    assert cl == cases() and eval(repr(cl[9])) == cl[9]
    assert S.digest(cl) == DIGEST, S.digest(cl)
    for axis, need in (("wc", {"ku-1", "ku", "ku+1", "ku+2", "uni"}), ("hc", {"ku-1", "ku", "ku+1", "ku+2", "uni"}), ("bd", {8, 10, 12}),
                       ("ss", {"420", "422", "444", "mono"}), ("kind", {k for k, _ in KINDS}), ("where", {k for k, _ in WHERE})):
        assert need <= {c[axis] for c in cl}, axis
    counting = sum(int(R.nlf_frame(frame_of(c, 0), c["bd"], *S.SUBSAMPLINGS[c["ss"]])["n"].sum()) > 0 for c in cl)
    assert counting > len(cl) * 2 // 3, "most cases have samples that pass the gate"


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_sweep_equals_the_reference(chunk):
    from grav1synth_amd.estimate import NoiseLevelMeter

    meters = {}
    for c in S.chunk_of(cases(), chunk, CHUNKS):
        subx, suby = S.SUBSAMPLINGS[c["ss"]]
        m = meters.get((c["bd"], c["batch"])) or NoiseLevelMeter(c["bd"], batch_frames=c["batch"])
        meters[(c["bd"], c["batch"])] = m
        wants = []
        for k in range(c["n"]):
            planes = frame_of(c, k)
            wants.append(R.nlf_frame(planes, c["bd"], subx, suby))
            dev = c["where"] == "device" or (c["where"] == "mixed" and k % 2 == 0)
            m.frame(_to_dev(planes, c["bd"]) if dev else planes, subx, suby)
        got = m.finish()
        assert len(got) == c["n"], c
        for k in range(c["n"]):
            bad = R.mismatches(got[k], wants[k], f"frame {k}")
            assert not bad, repr(c) + "\n" + "\n".join(bad)
    for m in meters.values():
        m.close()
