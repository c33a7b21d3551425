"""A seeded, edge-weighted sweep of the temporal meter in the manner of tests/test_gpu_measure_sweep.py (tests/sweep.py is not
edited).  The case list is drawn from numpy.random.default_rng([SEED, OP_ID]) as plain pasteable records, it is fixed, and its
SHA-256 is printed and pinned here; every temporal record is compared field by field with tests/measure_t_ref.py, every
ordinary record with tests/measure_ref.py."""
from __future__ import annotations

import numpy as np
import pytest

from tests import measure_ref as R
from tests import measure_t_ref as T
from tests import sweep as S
from tests.test_gpu_grain import _to_dev

SEED, N, CHUNKS = 13, 60, 3
OP_ID = len(S.OPS) + 1  # (len(S.OPS) is the `measure` sweep's)
TW, TH = 64, 128        # km_measure_t's tile
DIGEST = "427fb30d9daa53168864cc3af7f49a15c32da54151fcb4d51241cdecaade0f80"

# what the residual of frame k is to the residual of frame k - 1
KINDS = [("noise", 3), ("small", 2), ("same", 2), ("moved", 3), ("one_bin", 1.5), ("two_bins", 1.5), ("ramp", 1.5), ("extreme", 1.5)]
WHERE = [("device", 3), ("host", 2), ("mixed", 1)]
FORCED = [
    dict(w=1, h=1, bd=8, ss="420", kind="noise", where="device", n=2, batch=1, cut=0),
    dict(w=TW, h=TH, bd=12, ss="444", kind="extreme", where="device", n=3, batch=2, cut=0),
    dict(w=TW + 1, h=TH + 1, bd=10, ss="420", kind="two_bins", where="mixed", n=5, batch=2, cut=3),
    dict(w=3, h=2 * TH - 1, bd=10, ss="422", kind="ramp", where="host", n=3, batch=2, cut=0),
    dict(w=4 * TW - 1, h=3, bd=8, ss="mono", kind="one_bin", where="host", n=5, batch=4, cut=0),
    dict(w=2, h=2, bd=12, ss="422", kind="moved", where="host", n=2, batch=1, cut=0),
    dict(w=2 * TW + 2, h=2 * TH + 1, bd=12, ss="420", kind="moved", where="device", n=3, batch=3, cut=0),
    dict(w=TW - 1, h=TH - 1, bd=8, ss="420", kind="same", where="host", n=1, batch=1, cut=0),
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
            n = int(S._pick(rng, [(1, 1), (2, 3), (3, 2), (5, 2)]))
            c = dict(w=w, h=h, bd=int(S._pick(rng, [(8, 1), (10, 1), (12, 1)])), ss=S._pick(rng, [("420", 3), ("422", 1), ("444", 1), ("mono", 1)]),
                     kind=S._pick(rng, KINDS), where=S._pick(rng, WHERE), n=n, batch=int(S._pick(rng, [(1, 1), (2, 2), (4, 1), (n + 1, 1)])),
                     cut=int(rng.integers(0, n)) if n > 2 and rng.integers(0, 3) == 0 else 0, wc=wc, hc=hc)
        out.append({"op": "measure_t", "i": i, **c, "forced": i < len(FORCED)})
    return out


def pair_of(c: dict, k: int):
    """(noisy, clean) of frame k of a case (numpy only).  cut = j > 0: g1s_measure_cut in front of frame j."""
    rng = np.random.default_rng([SEED, c["i"], k])
    fixed = np.random.default_rng([SEED, c["i"]])  # (what the frames of a case share)
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
            b = ((xs + 3 * ys + 7 * k) % 32) * step + ((ys + k) % step)
        elif c["kind"] == "extreme":
            b = np.where(rng.integers(0, 2, s) > 0, top, 0)
        elif c["kind"] in ("same", "moved"):
            b = rng.integers(top // 4, top - top // 4, s)
        else:
            b = rng.integers(0, top + 1, s)
        if c["kind"] == "extreme":
            a = top - b
        elif c["kind"] in ("same", "moved"):
            d = fixed.integers(-(top // 4), top // 4 + 1, s)  # the case's residual: as it is, or moved by k samples right and down
            if c["kind"] == "moved":
                d = np.roll(d, (k % 3, k % 3), (0, 1))
            a = b + d
        else:
            amp = 12 if c["kind"] == "small" else top
            a = np.clip(b + rng.integers(-amp, amp + 1, s), 0, top)
        noisy.append(np.ascontiguousarray(a.astype(dt)))
        clean.append(np.ascontiguousarray(b.astype(dt)))
    return noisy, clean


def test_the_case_list_is_fixed_and_covers_its_axes():
    cl = cases()
    print("measure_t sweep: %d cases, sha256 %s" % (len(cl), S.digest(cl)))
    assert cl == cases() and eval(repr(cl[9])) == cl[9]
    assert S.digest(cl) == DIGEST, S.digest(cl)
    for axis, need in (("wc", {"ku-1", "ku", "ku+1", "uni"}), ("hc", {"ku-1", "ku", "ku+1", "uni"}), ("bd", {8, 10, 12}),
                       ("ss", {"420", "422", "444", "mono"}), ("kind", {k for k, _ in KINDS}), ("where", {k for k, _ in WHERE}),
                       ("n", {1, 2, 3, 5})):
        assert need <= {c[axis] for c in cl}, axis
    assert any(c["cut"] for c in cl) and any(c["batch"] == c["n"] + 1 for c in cl) and any(c["batch"] == 1 and c["n"] > 2 for c in cl)
    for c in cl[:12]:  # the residuals stay inside the bit depth
        for k in range(c["n"]):
            noisy, clean = pair_of(c, k)
            assert all(int(p.max()) <= (1 << c["bd"]) - 1 for p in noisy + clean)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_sweep_equals_the_restatement(chunk):
    from grav1synth_amd.measure import GrainMeter

    meters = {}
    for c in S.chunk_of(cases(), chunk, CHUNKS):
        subx, suby = S.SUBSAMPLINGS[c["ss"]]
        m = meters.setdefault((c["bd"], c["batch"]), None) or GrainMeter(c["bd"], batch_frames=c["batch"], temporal=True)
        meters[(c["bd"], c["batch"])] = m
        pairs, keep = [], []
        for k in range(c["n"]):
            noisy, clean = pair_of(c, k)
            pairs.append((noisy, clean))
            if c["cut"] and k == c["cut"]:
                m.cut()
            dev = c["where"] == "device" or (c["where"] == "mixed" and k % 2 == 0)
            keep.append((_to_dev(noisy, c["bd"]) if dev else noisy, _to_dev(clean, c["bd"]) if dev or c["where"] == "mixed" else clean))
            m.measure(keep[-1][0], keep[-1][1], subx, suby)
        runs = [pairs[:c["cut"]], pairs[c["cut"]:]] if c["cut"] else [pairs]
        wants = [rec for run in runs for rec in T.run_records(run, c["bd"], subx, suby)]
        got = m.finish_temporal()
        assert len(got) == len(wants), c
        for k, want in enumerate(wants):
            bad = T.mismatches(got[k], want, f"record {k}")
            assert not bad, repr(c) + "\n" + "\n".join(bad)
        got = m.finish()
        assert len(got) == c["n"], c
        for k, (noisy, clean) in enumerate(pairs):
            bad = R.mismatches(got[k], R.measure_frame(noisy, clean, c["bd"], subx, suby), f"frame {k}")
            assert not bad, repr(c) + "\n" + "\n".join(bad)
        m.cut()
    for m in meters.values():
        m.close()
