"""A seeded, edge-weighted sweep of the temporal noise levels in the manner of tests/sweep.py (which is not edited: its
SUITE and its CPU test stay as they are) and of tests/test_gpu_nlf_sweep.py.  The case list is drawn from
numpy.random.default_rng([SEED, OP_ID]) as plain pasteable records, it is fixed, and its SHA-256 is printed and pinned
here; every temporal record is compared field by field with tests/nlf_t_ref.py and every ordinary record with
tests/nlf_ref.py.  The edges are k_nlf_t's: 496 output columns and 32 output rows a wave's strip; a case is one meter's
queue of one or two runs, with a cut or not between them."""
from __future__ import annotations

import numpy as np
import pytest

from tests import nlf_ref as R
from tests import nlf_t_ref as T
from tests import sweep as S
from tests.test_gpu_grain import _to_dev

SEED, N, CHUNKS = 12, 48, 3
OP_ID = 103  # (beside tests/sweep.py's operations, the joint sweep's 100, the grain prior's 101 and the noise levels' 102)
SW, SH = 496, 32
DIGEST = "034d14f191f5841d9159a6d07ded04dce5caa577e94f0bc1297fc2efc8c72867"

KINDS = [("still", 3), ("fade", 2), ("moved", 2), ("one_bin", 1), ("two_bins", 1.5), ("checker", 1), ("wild", 1)]
WHERE = [("device", 3), ("host", 1), ("mixed", 2)]
FORCED = [
    dict(w=1, h=1, bd=8, ss="420", kind="still", where="device", n=2, batch=1, cut=0),
    dict(w=SW + 1, h=SH + 2, bd=12, ss="444", kind="checker", where="device", n=3, batch=2, cut=0),
    dict(w=SW + 2, h=SH + 3, bd=10, ss="420", kind="two_bins", where="mixed", n=4, batch=2, cut=2),
    dict(w=3, h=2 * SH + 1, bd=10, ss="422", kind="fade", where="host", n=3, batch=2, cut=0),
    dict(w=2 * SW + 1, h=3, bd=8, ss="mono", kind="one_bin", where="device", n=5, batch=4, cut=4),
    dict(w=2, h=2, bd=12, ss="422", kind="moved", where="host", n=2, batch=1, cut=0),
    dict(w=2 * (SW + 1) + 1, h=2 * (SH + 2) + 1, bd=10, ss="420", kind="moved", where="mixed", n=3, batch=1, cut=1),
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
            n = int(S._pick(rng, [(2, 3), (3, 2), (5, 1)]))
            c = dict(w=w, h=h, bd=int(S._pick(rng, [(8, 1), (10, 1), (12, 1)])), ss=S._pick(rng, [("420", 3), ("422", 1), ("444", 1), ("mono", 1)]),
                     kind=S._pick(rng, KINDS), where=S._pick(rng, WHERE), n=n, batch=int(S._pick(rng, [(1, 1), (2, 2), (4, 1)])),
                     cut=int(rng.integers(0, n)) if rng.random() < 0.3 else 0, wc=wc, hc=hc)  # (cut: before frame `cut`; 0 = none)
        out.append({"op": "nlf_t", "i": i, **c, "forced": i < len(FORCED)})
    return out


def frame_of(c: dict, k: int):
    """The planes of frame k of a case (numpy only)."""
    rng = np.random.default_rng([SEED, c["i"], k])
    still = np.random.default_rng([SEED, c["i"]])  # (the same draws for every frame of the case)
    bd, top = c["bd"], (1 << c["bd"]) - 1
    subx, suby = S.SUBSAMPLINGS[c["ss"]]
    dt = np.uint8 if bd == 8 else np.uint16
    shapes = [(c["h"], c["w"])] + ([] if c["ss"] == "mono" else [((c["h"] + suby) >> suby, (c["w"] + subx) >> subx)] * 2)
    step, up = 1 << (bd - 5), 1 << (bd - 8)
    planes = []
    for j, s in enumerate(shapes):
        ys, xs = np.arange(s[0])[:, None], np.arange(s[1])[None, :]
        small = rng.integers(-2 * up, 2 * up + 1, s)
        picture = ((xs * (1 + j) + 2 * ys) * up + still.integers(0, top // 2)) % (top + 1)
        picture = np.where(still.random(s) < 0.15, still.integers(0, top + 1, s), picture)
        if c["kind"] == "one_bin":
            p = np.full(s, 5 * step + j + k) + 0 * small
        elif c["kind"] == "two_bins":  # (the two box sums together are 9 below 18 x 8 step around an A and 9 above around a B)
            p = np.where((xs + ys) & 1, 8 * step - 5, 8 * step + 4) + (k & 1) + 0 * small
        elif c["kind"] == "checker":
            p = np.where((xs + ys + (k >> 1)) & 1, top, 0) + 0 * small
        elif c["kind"] == "wild":
            p = rng.integers(0, top + 1, s)
        elif c["kind"] == "fade":
            p = picture + small + (3 * k - 4) * up
        elif c["kind"] == "moved":
            p = np.roll(picture, 2 * k, axis=1) + small
        else:
            p = picture + small
        planes.append(np.ascontiguousarray(np.clip(p, 0, top).astype(dt)))
    return planes


def wanted(c: dict, frames):
    subx, suby = S.SUBSAMPLINGS[c["ss"]]
    return [T.nlf_pair(frames[k], frames[k - 1], c["bd"], subx, suby) for k in range(1, c["n"]) if k != c["cut"]]


def test_the_case_list_is_fixed_and_covers_its_axes():
    cl = cases()
    print("nlf_t sweep: %d cases, sha256 %s" % (len(cl), S.digest(cl)))
    assert cl == cases() and eval(repr(cl[9])) == cl[9]
    assert S.digest(cl) == DIGEST, S.digest(cl)
    for axis, need in (("wc", {"ku-1", "ku", "ku+1", "ku+2", "uni"}), ("hc", {"ku-1", "ku", "ku+1", "ku+2", "uni"}), ("bd", {8, 10, 12}),
                       ("ss", {"420", "422", "444", "mono"}), ("kind", {k for k, _ in KINDS}), ("where", {k for k, _ in WHERE})):
        assert need <= {c[axis] for c in cl}, axis
    assert any(c["cut"] for c in cl if not c["forced"]) and any(c["n"] > c["batch"] for c in cl)
    counting = signed = 0
    for c in cl:
        rec = wanted(c, [frame_of(c, k) for k in range(c["n"])])
        counting += any(int(r["n"].sum()) > 0 for r in rec)
        signed += any((r["s"] < 0).any() for r in rec)
    assert counting > len(cl) * 2 // 3, "most cases have samples that pass the gate"
    assert signed > len(cl) // 3, "and many have sums that fall"


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_sweep_equals_the_reference(chunk):
    from grav1synth_amd.estimate import NoiseLevelMeter

    meters = {}
    for c in S.chunk_of(cases(), chunk, CHUNKS):
        subx, suby = S.SUBSAMPLINGS[c["ss"]]
        m = meters.get((c["bd"], c["batch"])) or NoiseLevelMeter(c["bd"], batch_frames=c["batch"], temporal=True)
        meters[(c["bd"], c["batch"])] = m
        m.cut()
        frames = [frame_of(c, k) for k in range(c["n"])]
        for k, planes in enumerate(frames):
            if k and k == c["cut"]:
                m.cut()
            dev = c["where"] == "device" or (c["where"] == "mixed" and k % 2 == 0)
            m.frame(_to_dev(planes, c["bd"]) if dev else planes, subx, suby)
        got, tgot = m.finish(), m.finish_temporal()
        wants = wanted(c, frames)
        assert len(got) == c["n"] and len(tgot) == len(wants), c
        bad = []
        for k in range(c["n"]):
            bad += R.mismatches(got[k], R.nlf_frame(frames[k], c["bd"], subx, suby), f"frame {k}")
        for k, want in enumerate(wants):
            bad += T.mismatches(tgot[k], want, f"pair {k}")
        assert not bad, repr(c) + "\n" + "\n".join(bad)
    for m in meters.values():
        m.close()
