"""A seeded, edge-weighted list of joint chroma cases under a chroma gain (`denoise`, rules 21 - 24), in the style of
tests/sweep.py and with its menus, from a generator of its own: 48 plain records in 3 chunks, every one run on the device
and compared with tests/denoise_gain_ref.py byte for byte.  A record draws the CHROMA size around the 64 x 48 tile and takes
the luma size from it, odd (the guide clamps) or even; the kind of gain; a motion range where it has a temporal radius; and
the clip lengths around the temporal window and the batch.  A failing record prints whole and can be pasted back into
run_cases.  tests/sweep.py and its lists are not touched."""
from __future__ import annotations

import time
from typing import List, Tuple

import numpy as np
import pytest

from tests import denoise_gain_ref as G
from tests import sweep as S

SEED, CASES, CHUNKS = 24, 48, 3
OP_ID = 101  # (beside tests/sweep.py's operations 0 .. 5 and the joint list's 100)
GAINS = [("random", 3), ("step", 2), ("steep", 2), ("flat", 1), ("top", 1)]


def gain_of(c: dict) -> np.ndarray:
    """The case's 256 multipliers: log-uniform random ones; 4 below a level and 16384 from it on; rule 21 at R = 8 on a steep s;
    the flat gain; 16384 everywhere."""
    rng = np.random.default_rng([c["gseed"], 5])
    if c["gain"] == "random":
        return np.rint(np.exp(rng.uniform(0.0, np.log(16384.0), 256))).astype(np.uint16)
    if c["gain"] == "step":
        return np.where(np.arange(256) < int(rng.integers(32, 224)), 4, 16384).astype(np.uint16)
    if c["gain"] == "steep":
        s = np.where(np.arange(256) < int(rng.integers(32, 224)), 3, 255).astype(np.uint8)
        return G.gain_from_s(s, 8)
    return G.FLAT.copy() if c["gain"] == "flat" else np.full(256, 16384, np.uint16)


def _dg(cw, ch, odd, bd, ss, A, S_, D, n, batch, nc, gain, mr=0, strength=4.0, chroma_strength=4.0, kind="grainy", split=-1, split_kind="none") -> dict:
    sx, sy = S.SUBSAMPLINGS[ss]
    w, h = (cw << sx) - (sx if odd else 0), (ch << sy) - (sy if odd else 0)
    return dict(w=w, h=h, cw=cw, ch=ch, wc=S._cls(cw, 64), hc=S._cls(ch, 48), odd=odd, pool=-1, bd=bd, ss=ss, A=A, S=S_, strength=strength,
                chroma_strength=chroma_strength, kind=kind, cseed=cw * 977 + ch + D, D=D, nframes=n, nc=nc, batch=batch, split=split, split_kind=split_kind,
                gain=gain, gseed=cw + 31 * ch, mr=mr)


FORCED = [
    _dg(65, 49, True, 12, "420", 3, 4, 0, 1, 2, "1", "step"), _dg(64, 48, False, 8, "420", 7, 4, 1, 3, 2, "2D+1", "random", 0, 60.0, 4.0, "gradient"),
    _dg(63, 47, True, 10, "422", 7, 1, 2, 3, 1, "D+1", "steep", 8, 0.05, 60.0, "noise"), _dg(1, 1, True, 8, "420", 3, 2, 1, 2, 2, "2D", "random", 8),
    _dg(129, 5, False, 10, "444", 1, 4, 0, 2, 3, "b-1", "top", 0, 1.0, 1000.0), _dg(40, 30, True, 12, "420", 7, 1, 3, 7, 3, "2D+1", "flat", 0, 1000.0, 1000.0, "const"),
    _dg(66, 50, True, 8, "420", 2, 2, 1, 4, 2, "2D+2", "step", 8, split=2, split_kind="geometry"),
    _dg(3, 2, False, 12, "422", 5, 3, 2, 5, 4, "2D+1", "random", 0, split=3, split_kind="sync"),
]


def cases(seed: int = SEED, n: int = CASES) -> List[dict]:
    rng = np.random.default_rng([seed, OP_ID])
    pool = S._dn_pool(rng, True)
    out = []
    while len(out) < n:
        i = len(out)
        if i < len(FORCED):
            out.append({"op": "denoise_jg", "i": i, **FORCED[i], "forced": True})
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
        gain = S._pick(rng, GAINS)
        mr = int(S._pick(rng, [(0, 2), (8, 1), (2, 1)])) if D else 0
        c = _dg(cw, ch, odd, p["bd"], ss, p["A"], p["S"], D, nfr, batch, nc, gain, mr, p["strength"], p["chroma_strength"], S._pick(rng, S.DN_KINDS), split,
                split_kind)
        c.update(wc=wc, hc=hc, pool=k, cseed=int(rng.integers(0, 1 << 30)), gseed=int(rng.integers(0, 1 << 30)))
        if S._dn_budget(c, nfr, min(2 * D + 1, nfr)) > 2.5e7:  # (what the numpy reference pays; drawn again)
            continue
        out.append({"op": "denoise_jg", "i": i, **c, "forced": False})
    return out


def gain_reference(c: dict, frames):
    from grav1synth_amd.denoise import weight_table

    luma = weight_table(c["bd"], c["S"], c["strength"])
    joint = weight_table(c["bd"], c["S"], c["chroma_strength"], joint_chroma=True)
    return G.denoise_clip(frames, *S.SUBSAMPLINGS[c["ss"]], c["D"], c["A"], c["S"], luma, joint, gain_of(c), c["bd"], c["mr"])


def run_cases(case_list) -> List[Tuple[dict, str]]:
    """Every case on the device and through the reference: [(case, what differs)], empty when all agree."""
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_sweep import _to_dev, first_difference

    fails = []
    for c in case_list:
        frames = S.denoise_frames(c, c["nframes"])
        dev = [_to_dev(f) for f in frames]
        dn = Denoiser(c["bd"], search_radius=c["A"], patch_radius=c["S"], strength=c["strength"], chroma_strength=c["chroma_strength"],
                      temporal_radius=c["D"], batch_frames=c["batch"], joint_chroma=True, motion_range=c["mr"], chroma_gain=gain_of(c))
        try:
            sub, k = S.SUBSAMPLINGS[c["ss"]], c["split"]
            msgs = []
            if c["split_kind"] == "sync":
                got = dn.denoise_clip(dev[:k], *sub) + dn.denoise_clip(dev[k:], *sub)
                want = gain_reference(c, frames[:k]) + gain_reference(c, frames[k:])
            elif c["split_kind"] == "geometry":  # a host frame of another geometry inside the queue: three clips
                oc, other = S.other_geometry(c)
                got = [dn.apply(f, *sub, sync=False) for f in dev[:k]]
                got_other = dn.apply(other, *S.SUBSAMPLINGS[oc["ss"]], sync=False)
                got += [dn.apply(f, *sub, sync=False) for f in dev[k:]]
                dn.sync()
                want = gain_reference(c, frames[:k]) + gain_reference(c, frames[k:])
                oc = dict(oc, gain=c["gain"], gseed=c["gseed"], mr=c["mr"])
                msgs.append(first_difference(got_other, gain_reference(oc, [other])[0], "the frame of the other geometry"))
            else:
                got = dn.denoise_clip(dev, *sub)
                want = gain_reference(c, frames)
            for t in range(len(frames)):
                msgs.append(first_difference(got[t], want[t], f"frame {t}") or first_difference(dev[t], frames[t], f"input frame {t} after the call"))
            fails += [(c, m) for m in msgs if m]
        finally:
            dn.close()
    return fails


def test_the_list_is_what_it_says_without_a_device():
    every = cases()
    assert len(every) == CASES and every == cases() and eval(repr(every)) == every
    assert [c["i"] for c in every] == list(range(CASES)) and all(c["forced"] == (c["i"] < len(FORCED)) for c in every)
    for c in every:
        sx, sy = S.SUBSAMPLINGS[c["ss"]]
        assert ((c["w"] + sx) >> sx, (c["h"] + sy) >> sy) == (c["cw"], c["ch"]) and c["w"] >= 1 and c["h"] >= 1
        assert 1 <= c["A"] <= 7 and 1 <= c["S"] <= 4 and 0 <= c["D"] <= 3 and c["nframes"] >= 1
        assert c["mr"] % 2 == 0 and 0 <= c["mr"] <= 64 and (c["D"] or not c["mr"])
        g = gain_of(c)
        assert g.shape == (256,) and g.dtype == np.uint16 and 1 <= int(g.min()) and int(g.max()) <= 16384
    assert {"ku-1", "ku", "ku+1"} <= {c["wc"] for c in every} and {"ku-1", "ku", "ku+1"} <= {c["hc"] for c in every}
    assert {c["ss"] for c in every} == {"420", "422", "444"} and {c["bd"] for c in every} == {8, 10, 12}
    assert {c["D"] for c in every} == {0, 1, 2, 3} and {c["split_kind"] for c in every} == {"none", "sync", "geometry"}
    assert {c["gain"] for c in every} == {g for g, _w in GAINS} and {0, 8} <= {c["mr"] for c in every}
    assert any(c["mr"] and c["D"] >= 2 for c in every)
    assert sorted(sum((S.chunk_of(every, k, CHUNKS) for k in range(CHUNKS)), []), key=lambda c: c["i"]) == every
    print("list sha256", S.digest(every))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_denoise_jg(chunk):
    every = cases()
    mine = S.chunk_of(every, chunk, CHUNKS)
    t0 = time.time()
    fails = run_cases(mine)
    print(f"sweep denoise_jg seed {SEED}: chunk {chunk} of {CHUNKS}, {len(mine)} of {CASES} cases, list sha256 {S.digest(every)}, "
          f"{len(fails)} failures, {time.time() - t0:.1f} s")
    bad = {c["i"] for c, _ in fails}
    assert not fails, f"{len(bad)} of {len(mine)} denoise_jg cases differ from the reference:\n" + "\n".join(f"FAIL {c!r} :: {m}" for c, m in fails)
