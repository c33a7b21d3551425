"""A seeded, edge-weighted list of joint chroma cases (`denoise` under G1S_DENOISE_JOINT_CHROMA), in the style of
tests/sweep.py and with its menus: 48 plain records in 3 chunks, every one run on the device and compared with
tests/denoise_joint_ref.py byte for byte.  The edges are the chroma tile's (64 x 48), so a record draws the CHROMA size
from the menu and takes the luma size from it, odd (the guide clamps) or even; the clip lengths are drawn around the
temporal window and the batch as denoise_t's are.  A failing record prints whole and can be pasted back into run_cases."""
from __future__ import annotations

import time
from typing import List, Tuple

import numpy as np
import pytest

from tests import denoise_joint_ref as J
from tests import sweep as S

SEED, CASES, CHUNKS = 14, 48, 3
OP_ID = 100  # (beside tests/sweep.py's operations 0 .. 5)


def _dj(cw, ch, odd, bd, ss, A, S_, D, n, batch, nc, strength=4.0, chroma_strength=4.0, kind="grainy", split=-1, split_kind="none") -> dict:
    sx, sy = S.SUBSAMPLINGS[ss]
    w, h = (cw << sx) - (sx if odd else 0), (ch << sy) - (sy if odd else 0)
    return dict(w=w, h=h, cw=cw, ch=ch, wc=S._cls(cw, 64), hc=S._cls(ch, 48), odd=odd, pool=-1, bd=bd, ss=ss, A=A, S=S_, strength=strength,
                chroma_strength=chroma_strength, kind=kind, cseed=cw * 977 + ch + D, D=D, nframes=n, nc=nc, batch=batch, split=split, split_kind=split_kind)


FORCED = [
    _dj(65, 49, True, 12, "420", 3, 4, 0, 1, 2, "1"), _dj(64, 48, False, 8, "420", 7, 4, 1, 3, 2, "2D+1", 60.0, 4.0, "gradient"),
    _dj(63, 47, True, 10, "422", 7, 1, 2, 3, 1, "D+1", 0.05, 60.0, "noise"), _dj(1, 1, True, 8, "420", 3, 2, 1, 2, 2, "2D"),
    _dj(129, 5, False, 10, "444", 1, 4, 0, 2, 3, "b-1", 1.0, 1000.0), _dj(40, 30, True, 12, "420", 7, 1, 3, 7, 3, "2D+1", 1000.0, 1000.0, "const"),
    _dj(66, 50, True, 8, "420", 2, 2, 1, 4, 2, "2D+2", split=2, split_kind="geometry"), _dj(3, 2, False, 12, "422", 5, 3, 2, 5, 4, "2D+1", split=3, split_kind="sync"),
]


def cases(seed: int = SEED, n: int = CASES) -> List[dict]:
    rng = np.random.default_rng([seed, OP_ID])
    pool = S._dn_pool(rng, True)
    out = []
    while len(out) < n:
        i = len(out)
        if i < len(FORCED):
            out.append({"op": "denoise_j", "i": i, **FORCED[i], "forced": True})
            continue
        cw, wc = S._edge(rng, 64, 2, (4, 100))
        ch, hc = S._edge(rng, 48, 2, (4, 75))
        k = int(rng.integers(0, len(pool)))
        p = pool[k]
        ss = S._pick(rng, [("420", 4), ("422", 2), ("444", 2)])
        odd = bool(rng.integers(0, 2))
        D, batch = p["D"], p["batch"]
        nc = S._pick(rng, [("1", 1), ("D", 1), ("D+1", 1.5), ("2D", 1), ("2D+1", 1.5), ("2D+2", 1), ("b-1", 1), ("b+1", 1)])
        nfr = max({"1": 1, "D": D, "D+1": D + 1, "2D": 2 * D, "2D+1": 2 * D + 1, "2D+2": 2 * D + 2, "b-1": batch - 1, "b+1": batch + 1}[nc], 1)
        split, split_kind = -1, "none"
        if nfr >= 2:
            split_kind = S._pick(rng, [("none", 3), ("sync", 1), ("geometry", 1)])
            if split_kind != "none":
                split = int(rng.integers(1, nfr))
        c = _dj(cw, ch, odd, p["bd"], ss, p["A"], p["S"], D, nfr, batch, nc, p["strength"], p["chroma_strength"], S._pick(rng, S.DN_KINDS), split, split_kind)
        c.update(wc=wc, hc=hc, pool=k, cseed=int(rng.integers(0, 1 << 30)))
        if S._dn_budget(c, nfr, min(2 * D + 1, nfr)) > 2.5e7:  # (what the numpy reference pays; drawn again)
            continue
        out.append({"op": "denoise_j", "i": i, **c, "forced": False})
    return out


def joint_reference(c: dict, frames):
    from grav1synth_amd.denoise import weight_table

    luma = weight_table(c["bd"], c["S"], c["strength"])
    joint = weight_table(c["bd"], c["S"], c["chroma_strength"], joint_chroma=True)
    return J.denoise_clip(frames, *S.SUBSAMPLINGS[c["ss"]], c["D"], c["A"], c["S"], luma, joint)


def run_cases(case_list) -> List[Tuple[dict, str]]:
    """Every case on the device and through the reference: [(case, what differs)], empty when all agree."""
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_sweep import _to_dev, first_difference

    made, fails = {}, []
    try:
        for c in case_list:
            frames = S.denoise_frames(c, c["nframes"])
            dev = [_to_dev(f) for f in frames]
            key = (c["bd"], c["A"], c["S"], c["strength"], c["chroma_strength"], c["D"], c["batch"])
            if key not in made:
                made[key] = Denoiser(c["bd"], search_radius=c["A"], patch_radius=c["S"], strength=c["strength"], chroma_strength=c["chroma_strength"],
                                     temporal_radius=c["D"], batch_frames=c["batch"], joint_chroma=True)
            dn, sub, k = made[key], S.SUBSAMPLINGS[c["ss"]], c["split"]
            msgs = []
            if c["split_kind"] == "sync":
                got = dn.denoise_clip(dev[:k], *sub) + dn.denoise_clip(dev[k:], *sub)
                want = joint_reference(c, frames[:k]) + joint_reference(c, frames[k:])
            elif c["split_kind"] == "geometry":  # a host frame of another geometry inside the queue: three clips
                oc, other = S.other_geometry(c)
                got = [dn.apply(f, *sub, sync=False) for f in dev[:k]]
                got_other = dn.apply(other, *S.SUBSAMPLINGS[oc["ss"]], sync=False)
                got += [dn.apply(f, *sub, sync=False) for f in dev[k:]]
                dn.sync()
                want = joint_reference(c, frames[:k]) + joint_reference(c, frames[k:])
                msgs.append(first_difference(got_other, joint_reference(oc, [other])[0], "the frame of the other geometry"))
            else:
                got = dn.denoise_clip(dev, *sub)
                want = joint_reference(c, frames)
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
        sx, sy = S.SUBSAMPLINGS[c["ss"]]
        assert ((c["w"] + sx) >> sx, (c["h"] + sy) >> sy) == (c["cw"], c["ch"]) and c["w"] >= 1 and c["h"] >= 1
        assert 1 <= c["A"] <= 7 and 1 <= c["S"] <= 4 and 0 <= c["D"] <= 3 and c["nframes"] >= 1
    # the edges the list is for are in it
    assert {"ku-1", "ku", "ku+1"} <= {c["wc"] for c in every} and {"ku-1", "ku", "ku+1"} <= {c["hc"] for c in every}
    assert {c["ss"] for c in every} == {"420", "422", "444"} and {c["bd"] for c in every} == {8, 10, 12}
    assert {c["D"] for c in every} == {0, 1, 2, 3} and {c["split_kind"] for c in every} == {"none", "sync", "geometry"}
    assert any(c["odd"] and c["ss"] == "420" for c in every) and any(not c["odd"] for c in every)
    assert sorted(sum((S.chunk_of(every, k, CHUNKS) for k in range(CHUNKS)), []), key=lambda c: c["i"]) == every


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_denoise_j(chunk):
    every = cases()
    mine = S.chunk_of(every, chunk, CHUNKS)
    t0 = time.time()
    fails = run_cases(mine)
    print(f"sweep denoise_j seed {SEED}: chunk {chunk} of {CHUNKS}, {len(mine)} of {CASES} cases, list sha256 {S.digest(every)}, "
          f"{len(fails)} failures, {time.time() - t0:.1f} s")
    bad = {c["i"] for c, _ in fails}
    assert not fails, f"{len(bad)} of {len(mine)} denoise_j cases differ from the reference:\n" + "\n".join(f"FAIL {c!r} :: {m}" for c, m in fails)
