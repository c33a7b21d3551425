"""The seeded sweep of `denoise` with a grain prior (rules 12 - 15): the 48 records of tests/denoise_curve_cases.py in 3
chunks, every one run on the device.  Per case: the luma bytes equal tests/denoise_curve_ref.py, the chroma bytes equal
those of a Denoiser made without the curve, the inputs are unchanged and, where the case hands over views, the bytes
around them too.  A failing record prints whole and can be pasted back into run_cases."""
from __future__ import annotations

import time
from typing import List, Tuple

import numpy as np
import pytest

from tests import denoise_curve_cases as DC
from tests import denoise_curve_ref as CR
from tests import sweep as S
from tests import views as V

SEED, CASES, CHUNKS = DC.SEED, DC.CASES, DC.CHUNKS


def case_curve(c: dict):
    from grav1synth_amd.denoise import grain_curve
    from tests.test_denoise_curve_cpu import segment

    points, rng = DC.curve_points(c["curve"])
    return grain_curve([segment(p) for p in points], c["bd"], CR.max_range(c["bd"]) if rng < 0 else rng)


def _views(planes, c, t, output):
    """The planes of a frame as views with a pitch, an odd base and a hostile margin: ([view], [guard])"""
    isz, top = planes[0].dtype.itemsize, (1 << c["bd"]) - 1
    made = [V.device_view(np.zeros_like(p) if output else p, pitch_bytes=p.shape[1] * isz + (18 if output else 26) * isz + 2 * isz * k,
                          base_offset_bytes=(10 if output else 6) * isz + isz * k, fill="max" if output else "random", max_code=top, seed=t)
            for k, p in enumerate(planes)]
    return [v for v, _g in made], [g for _v, g in made]


def run_cases(case_list) -> List[Tuple[dict, str]]:
    """Every case on the device and through the reference: [(case, what differs)], empty when all agree."""
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_sweep import _to_dev, first_difference

    made, fails = {}, []
    try:
        for c in case_list:
            frames = S.denoise_frames(c, c["nframes"])
            sub, k = S.SUBSAMPLINGS[c["ss"]], c["split"]
            fwd, inv = case_curve(c)
            key = (c["bd"], c["A"], c["S"], c["strength"], c["chroma_strength"], c["D"], c["batch"], c["joint"], c["curve"])
            if key not in made:
                kw = dict(search_radius=c["A"], patch_radius=c["S"], strength=c["strength"], chroma_strength=c["chroma_strength"], temporal_radius=c["D"],
                          batch_frames=c["batch"], joint_chroma=c["joint"])
                made[key] = (Denoiser(c["bd"], curve=(fwd, inv), **kw), Denoiser(c["bd"], **kw))
            with_curve, without = made[key]
            clips = [frames[:k], frames[k:]] if c["split_kind"] != "none" else [frames]
            oc, other = S.other_geometry(c) if c["split_kind"] == "geometry" else (None, None)
            guards_in, guards_out, dev_in = [], [], []

            def through(dn, hostile):
                outs = []
                for n, clip in enumerate(clips):
                    for f in clip:
                        t = len(outs)
                        fin, out = _to_dev(f), None
                        if hostile and c["view"] in ("in", "both"):
                            fin, g = _views(f, c, t, False)
                            guards_in.extend(g)
                        elif hostile:
                            dev_in.append((fin, f, t))
                        if hostile and c["view"] in ("out", "both"):
                            out, g = _views(f, c, t, True)
                            guards_out.extend(g)
                        outs.append(dn.apply(fin, *sub, sync=False, out=out))
                    if n + 1 < len(clips):
                        if other is not None:  # a host frame of another geometry inside the queue: three clips
                            outs_other.append(dn.apply(other, *S.SUBSAMPLINGS[oc["ss"]], sync=False))
                        else:
                            dn.sync()
                dn.sync()
                return outs

            outs_other = []
            got, plain = through(with_curve, True), through(without, False)
            luma = sum((CR.denoise_luma_clip([f[0] for f in clip], fwd, inv, c["D"], c["A"], c["S"], c["strength"]) for clip in clips), [])
            msgs = []
            for t in range(len(frames)):
                msgs.append(first_difference(got[t][:1], [luma[t]], f"luma of frame {t}"))
                msgs.append(first_difference(got[t][1:], [p.cpu().numpy() for p in plain[t][1:]], f"chroma of frame {t} against the denoiser without a curve"))
            if other is not None:
                want = CR.denoise_luma_clip([other[0]], fwd, inv, c["D"], c["A"], c["S"], c["strength"])
                msgs.append(first_difference(outs_other[0][:1], want, "luma of the frame of the other geometry"))
                msgs.append(first_difference(outs_other[0][1:], outs_other[1][1:], "chroma of the frame of the other geometry"))
            for fin, f, t in dev_in:
                msgs.append(first_difference(fin, f, f"input frame {t} after the call"))
            for what, guards in (("input", guards_in), ("output", guards_out)):
                for g in guards:
                    bad = g.changed_bytes() if what == "input" else g.changed_margin_bytes()
                    msgs.append(f"{bad.size} bytes of / around a strided {what} were written, first at {int(bad[0])}" if bad.size else "")
            fails += [(c, m) for m in msgs if m]
    finally:
        for a, b in made.values():
            a.close(), b.close()
    return fails


def test_the_list_is_what_it_says_without_a_device():
    every = DC.cases()
    assert len(every) == CASES and every == DC.cases() and eval(repr(every)) == every
    assert [c["i"] for c in every] == list(range(CASES)) and all(c["forced"] == (c["i"] < len(DC.FORCED)) for c in every)
    for c in every:
        assert c["w"] >= 1 and c["h"] >= 1 and c["bd"] in (8, 10) and c["curve"] in DC.CURVES
        assert 1 <= c["A"] <= 7 and 1 <= c["S"] <= 4 and 0 <= c["D"] <= 3 and c["nframes"] >= 1
        assert (c["wc"], c["hc"]) == (S._cls(c["w"], 16), S._cls(c["h"], 32)) or not c["forced"]
    # the edges the list is for are in it
    assert {"ku-1", "ku", "ku+1"} <= {c["wc"] for c in every} and {"ku-1", "ku", "ku+1"} <= {c["hc"] for c in every}
    assert {c["ss"] for c in every} == {"420", "422", "444", "mono"} and {c["bd"] for c in every} == {8, 10}
    assert {c["D"] for c in every} == {0, 1, 2, 3} and {c["split_kind"] for c in every} == {"none", "sync", "geometry"}
    assert {c["curve"] for c in every} == set(DC.CURVES) and {c["view"] for c in every} == {"none", "in", "out", "both"}
    assert {c["joint"] for c in every} == {False, True} and any(c["joint"] and c["D"] and c["ss"] != "mono" for c in every)
    assert sorted(sum((S.chunk_of(every, k, CHUNKS) for k in range(CHUNKS)), []), key=lambda c: c["i"]) == every
    for name in DC.CURVES:
        points, rng = DC.curve_points(name)
        assert points and all(all(b[0] > a[0] for a, b in zip(p, p[1:])) for p in points) and rng in (-1, 0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_denoise_c(chunk):
    every = DC.cases()
    mine = S.chunk_of(every, chunk, CHUNKS)
    t0 = time.time()
    fails = run_cases(mine)
    print(f"sweep denoise_c seed {SEED}: chunk {chunk} of {CHUNKS}, {len(mine)} of {CASES} cases, list sha256 {S.digest(every)}, "
          f"{len(fails)} failures, {time.time() - t0:.1f} s")
    bad = {c["i"] for c, _ in fails}
    assert not fails, f"{len(bad)} of {len(mine)} denoise_c cases differ from the reference:\n" + "\n".join(f"FAIL {c!r} :: {m}" for c, m in fails)
