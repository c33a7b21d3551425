"""A seeded, edge-weighted sweep of `denoise` with coarse levels on the device against tests/denoise_levels_ref.py, bit for bit:
32 cases in 2 chunks from the generator below.  A case is a dict of plain values; the failure message lists every failing case
as the record to paste into run_case().  The list's SHA-256 is printed, so that two runs can be seen to have drawn the same."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

from tests import denoise_levels_content as LC
from tests import denoise_levels_ref as LR

pytestmark = pytest.mark.gpu

SEED, CASES, CHUNKS = 2905, 32, 2
# sizes where something changes: a lane's 8 coarse samples (16 fine), a 16-byte step at either sample size, the filter's tile
# (64 x 48) at the fine and at both coarse levels, and the very small
EDGE_W = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 255, 257]
EDGE_H = [1, 2, 3, 5, 47, 48, 49, 95, 96, 97, 98]


def cases(seed: int = SEED, n: int = CASES):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pick = lambda xs: xs[int(rng.integers(len(xs)))]  # noqa: E731
        edge = rng.random() < 0.7
        w = pick(EDGE_W) if edge else int(rng.integers(1, 200))
        h = pick(EDGE_H) if edge else int(rng.integers(1, 120))
        bd = pick([8, 8, 10, 10, 12])
        ss = pick(["mono", "420", "420", "422", "444"])
        D = pick([0, 0, 1, 2])
        joint = ss != "mono" and rng.random() < 0.4
        c = dict(i=i, w=w, h=h, bd=bd, ss=ss, K=pick([1, 2, 2]), rho=pick([0.0, 0.0, 0.0625, 0.5, 2.0, 4.0]), h8=pick([1.5, 4.0, 9.0]), A=pick([1, 2, 3, 3, 5]),
                 S=pick([1, 2, 2, 3]), D=D, n=pick([1, 2, 3, 4]) if D else pick([1, 2]), mr=pick([0, 0, 2, 6, 16]) if D else 0, joint=bool(joint),
                 gain=bool(joint and rng.random() < 0.5), curve=bool(bd < 12 and rng.random() < 0.3), batch=pick([0, 0, 1, 2, 3]),
                 memory=pick(["device", "device", "host", "view"]), seed=int(rng.integers(1 << 30)))
        out.append(c)
    return out


def digest(cs) -> str:
    return hashlib.sha256(repr(cs).encode()).hexdigest()


def run_case(c) -> str:
    """"" or what differs"""
    from grav1synth_amd.denoise import Denoiser
    from tests import views as V
    from tests.test_gpu_grain import _to_dev
    from tests.test_gpu_sweep import first_difference

    bd, ss = c["bd"], c["ss"]
    kw = dict(K=c["K"], rho=c["rho"] or 1.0, h=c["h8"], A=c["A"], S=c["S"], D=c["D"], mr=c["mr"], joint=c["joint"])
    if c["gain"]:
        from tests.test_gpu_denoise_gain import steep_gain

        kw["gain"] = steep_gain()
    if c["curve"]:
        from tests.test_gpu_denoise_curve import curve

        kw["curve"] = curve("example", bd)
    frames = LC.grainy(c["n"], c["w"], c["h"], bd, ss, seed=c["seed"], sigma=3.0 + c["h8"] / 2)
    want = LR.denoise_clip(frames, *LC.SUB[ss], bd, **kw)
    dn = Denoiser(bd, batch_frames=c["batch"], search_radius=c["A"], patch_radius=c["S"], strength=c["h8"], temporal_radius=c["D"], motion_range=c["mr"],
                  joint_chroma=c["joint"], chroma_gain=kw.get("gain"), curve=kw.get("curve"), coarse_levels=c["K"], coarse_ratio=c["rho"])
    guards = []
    try:
        if c["memory"] == "host":
            ins = frames
        elif c["memory"] == "device":
            ins = [_to_dev(f, bd) for f in frames]
        else:
            isz = 1 if bd == 8 else 2
            made = [[V.device_view(p, pitch_bytes=p.shape[1] * isz + isz * (3 + 4 * k), base_offset_bytes=isz * (1 + 2 * k), max_code=(1 << bd) - 1, seed=t)
                     for k, p in enumerate(f)] for t, f in enumerate(frames)]
            ins = [[v for v, _g in f] for f in made]
            guards = [g for f in made for _v, g in f]
        got = dn.denoise_clip(ins, *LC.SUB[ss])
        for t, (a, b) in enumerate(zip(got, want)):
            bad = first_difference(a, b, f"frame {t}")
            if bad:
                return bad
        for g in guards:
            g.assert_unchanged("an input view")
    finally:
        dn.close()
    return ""


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_the_sweep(chunk):
    cs = cases()
    print(f"levels sweep: seed {SEED}, {len(cs)} cases, SHA-256 {digest(cs)}")
    assert cs == cases() and cases(SEED + 1) != cs, "seeded"
    failed = []
    for c in cs[chunk::CHUNKS]:
        why = run_case(c)
        if why:
            failed.append(f"{why}\n    run_case({c!r})")
    assert not failed, f"{len(failed)} cases differ:\n" + "\n".join(failed)
