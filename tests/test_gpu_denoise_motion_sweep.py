"""A seeded, edge-weighted list of motion cases (`denoise` with a temporal radius and a motion range, rules 16 - 20), in
the style of tests/test_gpu_denoise_joint_sweep.py: 48 plain records in 3 chunks, every one run on the device and compared
with tests/denoise_motion_ref.py byte for byte, the vectors of frame 0 towards frame 1 included.  Edges are drawn round the
64 x 48 block for the plane size and round the motion range for the pan of every interval (Mr - 2, Mr, Mr + 2, an odd shift,
none); the clip lengths round the temporal window and the batch.  A failing record prints whole and can be pasted back
into run_cases."""
from __future__ import annotations

import time
from typing import List, Tuple

import numpy as np
import pytest

from tests import motion_content as MC
from tests import sweep as S

SEED, CASES, CHUNKS = 16, 48, 3
OP_ID = 102  # (beside tests/sweep.py's operations 0 .. 5 and the other sweeps' 100, 101)
RANGES = [(2, 1), (8, 1), (16, 2), (32, 2), (64, 1)]
SHIFT_KINDS = [("Mr-2", 2), ("Mr", 3), ("Mr+2", 2), ("odd", 2), ("none", 1)]


def _shift(kind: str, mr: int, sign: Tuple[int, int], axis: int) -> Tuple[int, int]:
    v = {"Mr-2": mr - 2, "Mr": mr, "Mr+2": mr + 2, "odd": (mr // 2) | 1, "none": 0}[kind]
    other = {"Mr-2": 2, "Mr": 0, "Mr+2": -2, "odd": 3, "none": 0}[kind]
    s = (v * sign[0], other * sign[1])
    return s if axis == 0 else (s[1], s[0])


def _dm(w, h, bd, ss, A, S_, D, mr, n, batch, nc, shifts, strength=4.0, chroma_strength=4.0, joint=False, content="noise", split=-1,
        split_kind="none") -> dict:
    return dict(w=w, h=h, wc=S._cls(w, 64), hc=S._cls(h, 48), pool=-1, bd=bd, ss=ss, A=A, S=S_, strength=strength, chroma_strength=chroma_strength,
                joint=joint, content=content, cseed=w * 977 + h + D + mr, D=D, mr=mr, nframes=n, nc=nc, batch=batch, shifts=shifts, split=split,
                split_kind=split_kind)


FORCED = [
    _dm(129, 97, 12, "444", 3, 2, 1, 64, 3, 2, "2D+1", [(64, 0), (0, -64)]), _dm(65, 49, 8, "420", 7, 4, 1, 2, 2, 2, "D+1", [(2, -2)], 60.0, 4.0, True),
    _dm(64, 48, 10, "422", 1, 1, 3, 32, 4, 3, "b+1", [(34, 2), (-32, 0), (17, 3)], joint=True), _dm(1, 1, 8, "420", 3, 2, 2, 64, 3, 2, "D+1", [(0, 0), (0, 0)]),
    _dm(63, 47, 12, "mono", 2, 3, 2, 16, 5, 2, "2D+1", [(16, 0), (-18, 2), (9, -3), (0, 14)], split=2, split_kind="sync"),
    _dm(130, 50, 10, "420", 3, 2, 1, 32, 4, 3, "2D+2", [(30, 2), (32, 0), (-34, -2)], content="ties", split=3, split_kind="geometry"),
]


def cases(seed: int = SEED, n: int = CASES) -> List[dict]:
    rng = np.random.default_rng([seed, OP_ID])
    pool = S._dn_pool(rng, True)
    out = []
    while len(out) < n:
        i = len(out)
        if i < len(FORCED):
            out.append({"op": "denoise_m", "i": i, **FORCED[i], "forced": True})
            continue
        w, wc = S._edge(rng, 64, 2, (4, 140))
        h, hc = S._edge(rng, 48, 2, (4, 100))
        k = int(rng.integers(0, len(pool)))
        p = pool[k]
        ss = S._pick(rng, [("420", 3), ("422", 2), ("444", 2), ("mono", 1)])
        D, batch = max(p["D"], 1), p["batch"]
        mr = S._pick(rng, RANGES)
        nc = S._pick(rng, [("1", 0.5), ("D+1", 1.5), ("2D", 1), ("2D+1", 1.5), ("2D+2", 1), ("b+1", 1.5)])
        nfr = max({"1": 1, "D+1": D + 1, "2D": 2 * D, "2D+1": 2 * D + 1, "2D+2": 2 * D + 2, "b+1": batch + 1}[nc], 1)
        shifts = [_shift(S._pick(rng, SHIFT_KINDS), mr, (int(rng.choice([-1, 1])), int(rng.choice([-1, 1]))), int(rng.integers(0, 2))) for _ in range(nfr - 1)]
        split, split_kind = -1, "none"
        if nfr >= 2:
            split_kind = S._pick(rng, [("none", 3), ("sync", 1), ("geometry", 1)])
            if split_kind != "none":
                split = int(rng.integers(1, nfr))
        c = _dm(w, h, p["bd"], ss, p["A"], p["S"], D, mr, nfr, batch, nc, shifts, p["strength"], p["chroma_strength"], bool(rng.integers(0, 2)) and ss != "mono",
                S._pick(rng, [("noise", 4), ("ties", 1)]), split, split_kind)
        c.update(wc=wc, hc=hc, pool=k, cseed=int(rng.integers(0, 1 << 30)))
        # what the numpy reference pays, capped as _dn_budget caps it: a block may bring a vector of its own, and every distinct
        # vector is a pass over the plane
        blocks = -(-w // 64) * -(-h // 48)
        if S._dn_budget(c, nfr, 1 + min(2 * D, nfr - 1) * min(blocks, 3)) > 2.5e7:
            continue
        out.append({"op": "denoise_m", "i": i, **c, "forced": False})
    return out


def frames_of(c: dict):
    shapes = S.plane_shapes(c["w"], c["h"], c["ss"])  # (rows, columns) a plane
    if c["content"] == "ties":
        return MC.clip([MC.ties(s[1], s[0], c["bd"], c["nframes"], 4) for s in shapes])
    sigma = 2.0 * (1 << (c["bd"] - 8))
    return MC.clip([MC.pan([c["cseed"], i], s[1], s[0], c["bd"], [tuple(x) for x in c["shifts"]], sigma)[1] for i, s in enumerate(shapes)])


def motion_reference(c: dict, frames):
    from grav1synth_amd.denoise import weight_table
    from tests import denoise_motion_ref as MR

    luma = weight_table(c["bd"], c["S"], c["strength"])
    chroma = weight_table(c["bd"], c["S"], c["chroma_strength"], joint_chroma=c["joint"])
    sub = S.SUBSAMPLINGS[c["ss"]] if c["ss"] != "mono" else (1, 1)
    return MR.denoise_clip(frames, *sub, c["D"], c["A"], c["S"], luma, chroma, c["mr"], c["joint"])


def run_cases(case_list) -> List[Tuple[dict, str]]:
    """Every case on the device and through the reference: [(case, what differs)], empty when all agree."""
    from grav1synth_amd.denoise import Denoiser
    from tests import denoise_motion_ref as MR
    from tests.test_gpu_sweep import _to_dev, first_difference

    made, fails = {}, []
    try:
        for c in case_list:
            frames = frames_of(c)
            dev = [_to_dev(f) for f in frames]
            key = (c["bd"], c["A"], c["S"], c["strength"], c["chroma_strength"], c["D"], c["batch"], c["mr"], c["joint"])
            if key not in made:
                made[key] = Denoiser(c["bd"], search_radius=c["A"], patch_radius=c["S"], strength=c["strength"], chroma_strength=c["chroma_strength"],
                                     temporal_radius=c["D"], batch_frames=c["batch"], joint_chroma=c["joint"], motion_range=c["mr"])
            dn, sub, k = made[key], S.SUBSAMPLINGS[c["ss"]] if c["ss"] != "mono" else (1, 1), c["split"]
            msgs = []
            if len(frames) > 1:
                got_v = dn.motion_vectors(dev[0], dev[1], *sub)
                want_v = [MR.search(frames[0][0], frames[1][0], c["mr"])]
                if len(frames[0]) == 3:
                    want_v += [MR.search(frames[0][1:3], frames[1][1:3], c["mr"])] * 2 if c["joint"] else [MR.search(frames[0][p], frames[1][p], c["mr"]) for p in (1, 2)]
                msgs += [None if np.array_equal(a, b) else f"vectors of plane {p}: {a.tolist()} vs {b.tolist()}" for p, (a, b) in enumerate(zip(got_v, want_v))]
            if c["split_kind"] == "sync":
                got = dn.denoise_clip(dev[:k], *sub) + dn.denoise_clip(dev[k:], *sub)
                want = motion_reference(c, frames[:k]) + motion_reference(c, frames[k:])
            elif c["split_kind"] == "geometry":  # a host frame of another geometry inside the queue: three clips
                oc = dict(c, w=c["w"] + 3, h=c["h"] + 1, ss="444" if c["ss"] != "444" else "420", nframes=1, shifts=[], cseed=c["cseed"] + 1, content="noise",
                          joint=c["joint"])
                other = frames_of(oc)[0]
                got = [dn.apply(f, *sub, sync=False) for f in dev[:k]]
                got_other = dn.apply(other, *S.SUBSAMPLINGS[oc["ss"]], sync=False)
                got += [dn.apply(f, *sub, sync=False) for f in dev[k:]]
                dn.sync()
                want = motion_reference(c, frames[:k]) + motion_reference(c, frames[k:])
                msgs.append(first_difference(got_other, motion_reference(oc, [other])[0], "the frame of the other geometry"))
            else:
                got = dn.denoise_clip(dev, *sub)
                want = motion_reference(c, frames)
            for t in range(len(frames)):
                msgs.append(first_difference(got[t], want[t], f"frame {t}") or first_difference(dev[t], frames[t], f"input frame {t} after the call"))
            fails += [(c, m) for m in msgs if m]
    finally:
        for d in made.values():
            d.close()
    return fails


def test_the_list_is_what_it_says_without_a_device():
    every = cases()
    assert len(every) == CASES and every == cases() and eval(repr(every)) == every
    assert [c["i"] for c in every] == list(range(CASES)) and all(c["forced"] == (c["i"] < len(FORCED)) for c in every)
    for c in every:
        assert 1 <= c["A"] <= 7 and 1 <= c["S"] <= 4 and 1 <= c["D"] <= 3 and c["nframes"] >= 1 and len(c["shifts"]) == c["nframes"] - 1
        assert c["mr"] % 2 == 0 and 2 <= c["mr"] <= 64 and not (c["joint"] and c["ss"] == "mono")
    # the edges the list is for are in it
    assert {"ku-1", "ku", "ku+1"} <= {c["wc"] for c in every} and {"ku-1", "ku", "ku+1"} <= {c["hc"] for c in every}
    assert {c["ss"] for c in every} == {"420", "422", "444", "mono"} and {c["bd"] for c in every} == {8, 10, 12}
    assert {c["D"] for c in every} == {1, 2, 3} and {c["split_kind"] for c in every} == {"none", "sync", "geometry"}
    assert {c["mr"] for c in every} == {r for r, _ in RANGES} and {c["joint"] for c in every} == {False, True}
    at = {max(abs(s[0]), abs(s[1])) - c["mr"] for c in every for s in c["shifts"]}
    assert {-2, 0, 2} <= at, "pans just inside the range, at it and one step beyond it"
    assert any((s[0] | s[1]) & 1 for c in every for s in c["shifts"]), "odd pans"
    assert any(c["nframes"] > c["batch"] for c in every), "clips that cross a batch"
    assert sorted(sum((S.chunk_of(every, k, CHUNKS) for k in range(CHUNKS)), []), key=lambda c: c["i"]) == every
    assert len(S.digest(every)) == 64


def test_the_references_of_the_list_stay_within_their_budget():
    """the cap is on what numpy pays; the forced corners are small by construction"""
    for c in cases():
        blocks = -(-c["w"] // 64) * -(-c["h"] // 48)
        assert S._dn_budget(c, c["nframes"], 1 + min(2 * c["D"], c["nframes"] - 1) * min(blocks, 3)) <= 2.5e7 or c["forced"], c


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_denoise_m(chunk):
    every = cases()
    mine = S.chunk_of(every, chunk, CHUNKS)
    t0 = time.time()
    fails = run_cases(mine)
    print(f"sweep denoise_m seed {SEED}: chunk {chunk} of {CHUNKS}, {len(mine)} of {CASES} cases, list sha256 {S.digest(every)}, "
          f"{len(fails)} failures, {time.time() - t0:.1f} s")
    bad = {c["i"] for c, _ in fails}
    assert not fails, f"{len(bad)} of {len(mine)} denoise_m cases differ from the reference:\n" + "\n".join(f"FAIL {c!r} :: {m}" for c, m in fails)
