"""A seeded, edge-weighted sweep of the lagged noise levels in the manner of tests/sweep.py (which is not edited) and of
tests/test_gpu_nlf_t_sweep.py, whose content kinds it takes.  The case list is drawn from numpy.random.default_rng([SEED,
OP_ID]) as plain pasteable records, it is fixed, and its SHA-256 is printed and pinned here; every lag record is compared
field by field with tests/nlf_lags_ref.py.  The edges are k_nlf_lags': a tile of 64 columns and 16 rows (the chroma launch's;
the luma launch's 32 are every other multiple), and beside the drawn sizes the forced ones sit one halo (6 columns, 3 rows)
and one staged ring (7, 4) past a tile.  A case is one meter's queue of one or two runs, with a cut or not between them."""
from __future__ import annotations

import numpy as np
import pytest

from tests import nlf_lags_ref as LG
from tests import sweep as S
from tests.test_gpu_grain import _to_dev
from tests.test_gpu_nlf_t_sweep import KINDS, WHERE, frame_of

SEED, N, CHUNKS = 12, 48, 3  # (SEED is tests/test_gpu_nlf_t_sweep.py's: frame_of draws from it)
OP_ID = 104
TW, TH = 64, 16
DIGEST = "caa09d79fe32473038c68809d856e0450fb4ad3b5bdb20d137fc42d9562894dd"

FORCED = [
    dict(w=1, h=1, bd=8, ss="420", kind="still", where="device", n=2, batch=1, cut=0),
    dict(w=TW + 6, h=2 * TH + 3, bd=12, ss="444", kind="checker", where="device", n=3, batch=2, cut=0),
    dict(w=TW + 7, h=2 * TH + 4, bd=10, ss="420", kind="two_bins", where="mixed", n=4, batch=2, cut=2),
    dict(w=3, h=4 * TH + 1, bd=10, ss="422", kind="fade", where="host", n=3, batch=2, cut=0),
    dict(w=4 * TW + 1, h=3, bd=8, ss="mono", kind="one_bin", where="device", n=5, batch=4, cut=4),
    dict(w=2 * (TW + 6), h=2 * (TH + 3), bd=12, ss="420", kind="fade", where="host", n=2, batch=1, cut=0),
    dict(w=2 * (TW + 7) + 1, h=2 * (2 * TH + 4) + 1, bd=10, ss="420", kind="moved", where="mixed", n=3, batch=1, cut=1),
    dict(w=7, h=4, bd=8, ss="444", kind="still", where="device", n=2, batch=1, cut=0),
]


def cases():
    rng = np.random.default_rng([SEED, OP_ID])
    out = []
    for i in range(N):
        if i < len(FORCED):
            c = dict(FORCED[i])
            c["wc"], c["hc"] = S._cls(c["w"], TW, plus2=True), S._cls(c["h"], TH, plus2=True)
        else:
            w, wc = S._edge(rng, TW, 4, (4, 300), plus2=True)
            h, hc = S._edge(rng, TH, 6, (4, 120), plus2=True)
            n = int(S._pick(rng, [(2, 3), (3, 2), (5, 1)]))
            c = dict(w=w, h=h, bd=int(S._pick(rng, [(8, 1), (10, 1), (12, 1)])), ss=S._pick(rng, [("420", 3), ("422", 1), ("444", 1), ("mono", 1)]),
                     kind=S._pick(rng, KINDS), where=S._pick(rng, WHERE), n=n, batch=int(S._pick(rng, [(1, 1), (2, 2), (4, 1)])),
                     cut=int(rng.integers(0, n)) if rng.random() < 0.3 else 0, wc=wc, hc=hc)  # (cut: before frame `cut`; 0 = none)
        out.append({"op": "nlf_lags", "i": i, **c, "forced": i < len(FORCED)})
    return out


def wanted(c: dict, frames):
    subx, suby = S.SUBSAMPLINGS[c["ss"]]
    return [LG.lags_pair(frames[k], frames[k - 1], c["bd"], subx, suby) for k in range(1, c["n"]) if k != c["cut"]]


def test_the_case_list_is_fixed_and_covers_its_axes():
    cl = cases()
    print("nlf_lags sweep: %d cases, sha256 %s" % (len(cl), S.digest(cl)))
    assert cl == cases() and eval(repr(cl[9])) == cl[9]
    assert S.digest(cl) == DIGEST, S.digest(cl)
    for axis, need in (("wc", {"ku-1", "ku", "ku+1", "ku+2", "uni"}), ("hc", {"ku-1", "ku", "ku+1", "ku+2", "uni"}), ("bd", {8, 10, 12}),
                       ("ss", {"420", "422", "444", "mono"}), ("kind", {k for k, _ in KINDS}), ("where", {k for k, _ in WHERE})):
        assert need <= {c[axis] for c in cl}, axis
    assert any(c["cut"] for c in cl if not c["forced"]) and any(c["n"] > c["batch"] for c in cl)
    far = crossed = signed = 0
    for c in cl:
        rec = wanted(c, [frame_of(c, k) for k in range(c["n"])])
        far += any(int(r["n"][0, 45]) > 0 for r in rec)
        crossed += any(int(r["xn"].min()) > 0 for r in rec)
        signed += any((r["r"] < 0).any() for r in rec)
    assert far > len(cl) // 2, "most cases have pairs at the farthest lag"
    assert crossed > len(cl) // 4 and signed > len(cl) // 3, "many have every cross pair, and products that fall"


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_sweep_equals_the_reference(chunk):
    from grav1synth_amd.estimate import NoiseLevelMeter

    meters = {}
    for c in S.chunk_of(cases(), chunk, CHUNKS):
        subx, suby = S.SUBSAMPLINGS[c["ss"]]
        m = meters.get((c["bd"], c["batch"])) or NoiseLevelMeter(c["bd"], batch_frames=c["batch"], lags=True)
        meters[(c["bd"], c["batch"])] = m
        m.cut()
        frames = [frame_of(c, k) for k in range(c["n"])]
        for k, planes in enumerate(frames):
            if k and k == c["cut"]:
                m.cut()
            dev = c["where"] == "device" or (c["where"] == "mixed" and k % 2 == 0)
            m.frame(_to_dev(planes, c["bd"]) if dev else planes, subx, suby)
        lgot = m.finish_lags()
        wants = wanted(c, frames)
        assert len(lgot) == len(wants) and len(m.finish()) == c["n"] and len(m.finish_temporal()) == len(wants), c
        bad = []
        for k, want in enumerate(wants):
            bad += LG.mismatches(lgot[k], want, f"pair {k}")
        assert not bad, repr(c) + "\n" + "\n".join(bad[:40])
    for m in meters.values():
        m.close()
