"""Coarse levels of `denoise` on a grid of the level kernels' own tiles, against tests/denoise_levels_ref.py byte for byte.

A workgroup of kd_down, kd_lowres and kd_add covers 256 x 8 coarse samples, 512 x 16 fine ones, and the tiles are counted on the
luma plane.  The fixed cases of tests/denoise_levels_content.py's grid_cases() put more than one tile column and more than one
tile row on the grid at once, at level 0 and at level 1, with chroma planes that end before the luma plane does in both
directions; tests/test_denoise_levels_grid_cpu.py shows on the reference alone that every tile of every plane has something to
do there.  Then a seeded sweep at such sizes, and what the other levels tests leave out: a temporal radius of 3, the ring of
host frames wrapping under levels, and the output of a clip with the timing on."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import denoise_levels_content as LC
from tests import views as V
from tests.test_gpu_denoise_levels import check, denoiser, reference
from tests.test_gpu_denoise_levels_sweep import digest, run_case
from tests.test_gpu_denoise_temporal import assert_clips_equal
from tests.test_gpu_grain import _to_dev, assert_planes_equal

pytestmark = pytest.mark.gpu

FIXED = [(c["name"], K) for c in LC.grid_cases() if "views" not in c["name"] for K in c["Ks"]]


@functools.lru_cache(maxsize=None)
def grid_clip(name):
    """(frames, what the reference makes of them at K = 1 and K = 2): computed once, not written to"""
    case = LC.grid_case(name)
    return LC.grid_frames(case), {}


def wanted(name, K):
    frames, made = grid_clip(name)
    if K not in made:
        case = LC.grid_case(name)
        made[K] = reference(frames, case["bd"], case["ss"], **LC.grid_kw(case, K))
    return made[K]


# ------------------------------------------------------------------------------------------------------- the fixed cases
@pytest.mark.parametrize("name,K", FIXED, ids=[f"{n}-K{K}" for n, K in FIXED])
def test_fixed_grid_cases(name, K):
    """every output plane of the clip from contiguous device frames, and the inputs afterwards"""
    case = LC.grid_case(name)
    frames, bd = grid_clip(name)[0], case["bd"]
    dn = denoiser(bd, case["batch"], **LC.grid_kw(case, K))
    try:
        dev = [_to_dev(f, bd) for f in frames]
        assert_clips_equal(dn.denoise_clip(dev, *LC.SUB[case["ss"]]), wanted(name, K), f"{name} K {K}")
        for d, f in zip(dev, frames):
            assert_planes_equal(d, f, f"{name} K {K}: input after the call")
    finally:
        dn.close()


# (bit depth, input pitch beyond the row and base, output pitch beyond the row and base, all in bytes): rows no 16-byte access
# fits, and rows of which every one (at 8 bits: of the chroma planes every second one) begins on a 16-byte address
VIEWS = [(8, 7, 3, 9, 5), (8, 16, 0, 32, 16), (10, 2, 14, 6, 18), (10, 32, 16, 16, 0)]


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("bd,in_extra,in_base,out_extra,out_base", VIEWS)
def test_views_with_a_pitch_and_an_odd_base_over_the_grid(bd, in_extra, in_base, out_extra, out_base, K):
    """the 16-byte and the sample-by-sample paths of a lane in tile columns 1 and 2, under hostile margins"""
    name = f"420 views {bd}"
    case = LC.grid_case(name)
    frame = grid_clip(name)[0][0]
    isz, top = (1 if bd == 8 else 2), (1 << bd) - 1
    vin = [V.device_view(p, pitch_bytes=p.shape[1] * isz + in_extra, base_offset_bytes=in_base, max_code=top, seed=c) for c, p in enumerate(frame)]
    vout = [V.device_view(np.zeros_like(p), pitch_bytes=p.shape[1] * isz + out_extra, base_offset_bytes=out_base, fill="max", max_code=top, seed=9 + c)
            for c, p in enumerate(frame)]
    dn = denoiser(bd, **LC.grid_kw(case, K))
    try:
        got = dn.apply([v for v, _g in vin], 1, 1, out=[v for v, _g in vout])
    finally:
        dn.close()
    assert_planes_equal(got, wanted(name, K)[0], f"views {bd} bit +{in_extra} at {in_base} to +{out_extra} at {out_base}, K {K}")
    for _v, g in vin:
        g.assert_unchanged("an input view")
    for _v, g in vout:
        g.assert_margin_intact("an output view")


# -------------------------------------------------------------------------------------------------------------- the sweep
SEED, CASES, CHUNKS = 1307, 12, 4
GRID_W = [1023, 1024, 1025, 1026, 1039, 1040, 1537]
GRID_H = [17, 31, 32, 33, 34, 35, 49]


def cases(seed: int = SEED, n: int = CASES):
    """as tests/test_gpu_denoise_levels_sweep.py draws a case, but the sides from the lists above and A and S from 1 and 2"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pick = lambda xs: xs[int(rng.integers(len(xs)))]  # noqa: E731
        w, h = pick(GRID_W), pick(GRID_H)
        bd = pick([8, 8, 10, 10, 12])
        ss = pick(["mono", "420", "420", "422", "444"])
        D = pick([0, 0, 1, 2])
        joint = ss != "mono" and rng.random() < 0.4
        c = dict(i=i, w=w, h=h, bd=bd, ss=ss, K=pick([1, 2, 2]), rho=pick([0.0, 0.0, 0.0625, 0.5, 2.0, 4.0]), h8=pick([1.5, 4.0, 9.0]), A=pick([1, 2]),
                 S=pick([1, 2]), D=D, n=pick([1, 2, 3, 4]) if D else pick([1, 2]), mr=pick([0, 0, 2, 6, 16]) if D else 0, joint=bool(joint),
                 gain=bool(joint and rng.random() < 0.5), curve=bool(bd < 12 and rng.random() < 0.3), batch=pick([0, 0, 1, 2, 3]),
                 memory=pick(["device", "device", "host", "view"]), seed=int(rng.integers(1 << 30)))
        out.append(c)
    return out


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_the_sweep_at_grid_sizes(chunk):
    cs = cases()
    print(f"levels grid sweep: seed {SEED}, {len(cs)} cases, SHA-256 {digest(cs)}")
    assert cs == cases() and cases(SEED + 1) != cs, "seeded"
    assert all(min(LC.tiles(c["w"], c["h"])) >= 2 for c in cs), "every case has more than one tile column and row"
    failed = []
    for c in cs[chunk::CHUNKS]:
        why = run_case(c)
        if why:
            failed.append(f"{why}\n    run_case({c!r})")
    assert not failed, f"{len(failed)} cases differ:\n" + "\n".join(failed)


# --------------------------------------------------------------------------------------------------- a temporal radius of 3
@functools.lru_cache(maxsize=None)
def long_clip():
    frames = LC.grainy(8, 66, 50, 8, "420", seed=80)
    return frames, reference(frames, 8, "420", K=2, D=3)


@pytest.mark.parametrize("batch", [1, 3])
def test_a_temporal_radius_of_3_under_two_levels(batch):
    """batch + D jobs a launch of the level kernels, rings of batch + 2 D slots, the hand-over to the inner level 3 frames ahead"""
    frames, want = long_clip()
    dn = denoiser(8, batch, K=2, D=3)
    try:
        dev = [_to_dev(f, 8) for f in frames]
        assert_clips_equal(dn.denoise_clip(dev, 1, 1), want, f"D 3, batch {batch}")
        for d, f in zip(dev, frames):
            assert_planes_equal(d, f, f"D 3, batch {batch}: input after the call")
    finally:
        dn.close()


def test_a_temporal_radius_of_3_with_motion_under_a_level():
    """Mr = 8, so Mr' = 4 on the coarse frames"""
    check(LC.grainy(5, 66, 50, 8, "420", seed=81), 8, "420", "D 3, Mr 8, K 1", K=1, D=3, mr=8)


# ----------------------------------------------------------------------------------------------- the ring of host frames
@functools.lru_cache(maxsize=None)
def host_clip():
    frames = LC.grainy(11, 66, 50, 8, "420", seed=82)
    return frames, reference(frames, 8, "420", K=2, D=1)


@pytest.mark.parametrize("every_third_on_the_device", [False, True])
def test_the_ring_of_host_frames_wraps_under_levels(every_third_on_the_device):
    """batch 2 and D = 1: 4 staging slots for 11 frames, so kd_down reads slots that were written a second and a third time"""
    frames, want = host_clip()
    dn = denoiser(8, 2, K=2, D=1)
    try:
        ins = [_to_dev(f, 8) if every_third_on_the_device and t % 3 == 2 else [p.copy() for p in f] for t, f in enumerate(frames)]
        assert_clips_equal(dn.denoise_clip(ins, 1, 1), want, f"11 host frames, every third on the device: {every_third_on_the_device}")
        for d, f in zip(ins, frames):
            assert_planes_equal(d, f, "input after the call")
    finally:
        dn.close()


# ----------------------------------------------------------------------------------------------------------------- timing
@pytest.mark.parametrize("which", ["1040 x 36", "66 x 50"])
def test_the_output_with_the_timing_on(which):
    """events and two waits in flush(), and the inner levels timed as well: the clip is the clip, and the times nest"""
    if which == "1040 x 36":
        case = LC.grid_case("420 clip")
        frames, want, kw = grid_clip(case["name"])[0], wanted(case["name"], 2), LC.grid_kw(case, 2)
    else:
        (frames, want), kw = host_clip(), dict(K=2, D=1)
        frames, want = frames[:4], reference(frames[:4], 8, "420", **kw)
    dn = denoiser(8, **kw)
    try:
        dn.kernel_times(True)
        assert_clips_equal(dn.denoise_clip([_to_dev(f, 8) for f in frames], 1, 1), want, f"{which} with the timing on")
        ms, n = dn.kernel_times(True)
        assert n == len(frames)
        assert 0.0 < dn.level_kernel_time() <= dn.level_time() < ms, (dn.level_kernel_time(), dn.level_time(), ms)
    finally:
        dn.close()
