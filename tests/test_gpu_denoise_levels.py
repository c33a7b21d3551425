"""Coarse levels of `denoise` on the device (rules 25 - 29 of include/g1s_diff.h) against tests/denoise_levels_ref.py, byte for
byte: plane sizes around a tile of the three small kernels, depths, every form of the filter under a level, ratios, the clip at
both ends of the range, frames of every kind of memory, views, batches and queueing, geometry changes, K = 0, far views, the
longest sides and the two .y4m commands."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import denoise_levels_content as LC
from tests import denoise_levels_ref as LR
from tests import views as V
from tests.test_gpu_denoise_temporal import _y4m_frames, assert_clips_equal
from tests.test_gpu_grain import _to_dev, assert_planes_equal

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 5), (63, 47), (64, 48), (65, 49), (127, 95), (129, 97), (130, 98)]
NAMES = dict(K="coarse_levels", rho="coarse_ratio", h="strength", hc="chroma_strength", A="search_radius", S="patch_radius", D="temporal_radius",
             mr="motion_range", joint="joint_chroma", gain="chroma_gain", curve="curve")


def denoiser(bd, batch=0, **kw):
    from grav1synth_amd.denoise import Denoiser

    return Denoiser(bd, batch_frames=batch, **{NAMES[k]: v for k, v in kw.items()})


def reference(frames, bd, ss, **kw):
    kw = dict(kw)
    kw["rho"] = kw.get("rho", 0.0) or 1.0
    return LR.denoise_clip(frames, *LC.SUB[ss], bd, **kw)


def check(frames, bd, ss, what, batch=0, **kw):
    """every output plane of the clip from contiguous device frames, and the inputs afterwards"""
    dn = denoiser(bd, batch, **kw)
    try:
        dev = [_to_dev(f, bd) for f in frames]
        assert_clips_equal(dn.denoise_clip(dev, *LC.SUB[ss]), reference(frames, bd, ss, **kw), what)
        for d, f in zip(dev, frames):
            assert_planes_equal(d, f, f"{what}: input after the call")
    finally:
        dn.close()


# ------------------------------------------------------------------------------------------------------------ plane sizes
@pytest.mark.parametrize("w,h", SIZES)
def test_luma_plane_sizes_at_8_bits(w, h):
    """a coarse plane below, on and above a tile of the filter (64 x 48) and a lane's 8 samples; odd sizes clamp"""
    frames = LC.grainy(1, w, h, 8, "mono", seed=10)
    for K in (1, 2):
        check(frames, 8, "mono", f"{w}x{h} K {K}", K=K)


@pytest.mark.parametrize("w,h", SIZES)
def test_420_plane_sizes_at_10_bits(w, h):
    frames = LC.grainy(1, w, h, 10, "420", seed=11)
    for K in (1, 2):
        check(frames, 10, "420", f"{w}x{h} K {K}", K=K)


# ----------------------------------------------------------------------------------------------------------------- depths
@pytest.mark.parametrize("bd,with_curve", [(8, False), (10, False), (12, False), (8, True), (10, True)])
def test_depths_with_and_without_a_curve(bd, with_curve):
    from tests.test_gpu_denoise_curve import curve

    frames = LC.grainy(1, 97, 65, bd, "420", seed=12 + bd)
    kw = dict(curve=curve("example", bd)) if with_curve else {}
    check(frames, bd, "420", f"{bd} bit curve {with_curve}", K=2, **kw)
    if with_curve and bd == 10:
        f, b, ss, kw = LC.with_curve()
        check(f, b, ss, "the curve case of the restatements", **kw)


# ------------------------------------------------------------------------------------------------------------------ forms
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_temporal_radius_on_short_clips(D, n):
    check(LC.grainy(n, 66, 50, 8, "420", seed=20 + n), 8, "420", f"D {D}, {n} frames", K=2 if n < 5 else 1, D=D)


@pytest.mark.parametrize("mr", [8, 6])
def test_motion_on_pans(mr):
    """Mr' = 4 either way: 8 halves, 6 rounds up"""
    frames, bd, ss, kw = LC.panned(mr)
    check(frames, bd, ss, f"Mr {mr}", **kw)


@pytest.mark.parametrize("gain", [False, True])
def test_joint_chroma_with_and_without_a_steep_gain(gain):
    frames, bd, ss, kw = LC.joint(gain)
    check(frames, bd, ss, f"joint chroma, gain {gain}", **kw)
    check(LC.grainy(3, 65, 49, 10, "420", seed=7), 10, "420", f"joint chroma, gain {gain}, D 1, K 2", **dict(kw, K=2, D=1))


@pytest.mark.parametrize("rho", [0.0625, 0.5, 1.0, 4.0])
def test_ratios(rho):
    for K in (1, 2):
        frames, bd, ss, kw = LC.ratio(rho, K)
        check(frames, bd, ss, f"rho {rho} K {K}", **(dict(kw, h=2.0) if rho == 4.0 else kw))


@pytest.mark.parametrize("A,S", [(1, 1), (1, 4), (7, 1), (7, 4)])
def test_parameter_corners(A, S):
    check(LC.grainy(1, 65, 49, 10, "mono", seed=30), 10, "mono", f"A {A} S {S}", K=2, A=A, S=S)


def test_the_clip_at_both_ends_of_the_range():
    frames, bd, ss, kw = LC.clipping()
    want = reference(frames, bd, ss, **kw)
    raw = LR.denoise_clip(frames, 1, 1, bd, **dict(kw, wrong=("noclip",)))[0][0]
    assert raw.min() < 0 and raw.max() > 255, "the content makes the sum leave the range at both ends"
    check(frames, bd, ss, "0 / max checker", **kw)
    assert want[0][0].min() == 0 and want[0][0].max() == 255
    for b in (10, 12):
        check(LC.checker(66, 50, b, seed=2), b, "mono", f"0 / max checker at {b} bits", **kw)


# ----------------------------------------------------------------------------------------------------------- frame memory
def test_host_pinned_device_and_view_frames_in_one_batch():
    import torch

    from grav1synth_amd.diff import Frame

    bd, ss, D = 10, "420", 1
    subx, suby = LC.SUB[ss]
    frames = LC.grainy(8, 131, 99, bd, ss, seed=40)
    want = reference(frames, bd, ss, K=2, D=D)
    dn = denoiser(bd, 8, K=2, D=D)
    L = _lib.lib()
    outs, guards_in, guards_out, keep = [], [], [], []
    for t, planes in enumerate(frames):
        kind = ("host", "pinned", "device", "view")[t % 4]
        if kind == "host":
            outs.append(dn.apply(planes, subx, suby, sync=False))
        elif kind == "pinned":
            pin_in = [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
            pin_out = [torch.from_numpy(np.zeros(p.shape, p.dtype)).pin_memory() for p in planes]
            fin, fout = Frame(pin_in, subx, suby, async_host=True).to_c(keep), Frame(pin_out, subx, suby, async_host=True).to_c(keep)
            assert fin.on_device == 2 and fout.on_device == 2
            keep += [pin_in, pin_out]
            assert L.g1s_denoise_frame(dn._h, C.byref(fin), C.byref(fout)) == 0
            dn._frames += 1
            outs.append([p.numpy() for p in pin_out])
        elif kind == "device":
            outs.append(dn.apply(_to_dev(planes, bd), subx, suby, sync=False))
        else:
            # a pitch, an odd base (not even a multiple of the sample size times two) and a hostile margin
            vin = [V.device_view(p, pitch_bytes=p.shape[1] * 2 + 26 + 2 * c, base_offset_bytes=6 + 2 * c, max_code=1023, seed=t) for c, p in enumerate(planes)]
            vout = [V.device_view(np.zeros_like(p), pitch_bytes=p.shape[1] * 2 + 18, base_offset_bytes=10, fill="max", max_code=1023, seed=t) for p in planes]
            guards_in += [g for _v, g in vin]
            guards_out += [g for _v, g in vout]
            outs.append(dn.apply([v for v, _g in vin], subx, suby, sync=False, out=[v for v, _g in vout]))
    dn.sync()
    assert_clips_equal(outs, want, "mixed memory")
    for g in guards_in:
        g.assert_unchanged("a strided input")
    for g in guards_out:
        g.assert_margin_intact("a strided output")
    dn.close()


@pytest.mark.parametrize("bd,pitch_extra,base", [(8, 7, 3), (8, 16, 0), (10, 2, 14), (10, 34, 16)])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(bd, pitch_extra, base):
    frames = LC.grainy(1, 131, 67, bd, "420", seed=41)
    isz = 1 if bd == 8 else 2
    top = (1 << bd) - 1
    vin = [V.device_view(p, pitch_bytes=p.shape[1] * isz + pitch_extra, base_offset_bytes=base, max_code=top, seed=c) for c, p in enumerate(frames[0])]
    vout = [V.device_view(np.zeros_like(p), pitch_bytes=p.shape[1] * isz + pitch_extra + 2 * isz, base_offset_bytes=(base + 2 * isz) % 256, fill="max",
                          max_code=top, seed=9 + c) for c, p in enumerate(frames[0])]
    dn = denoiser(bd, K=2)
    got = dn.apply([v for v, _g in vin], 1, 1, out=[v for v, _g in vout])
    dn.close()
    assert_planes_equal(got, reference(frames, bd, "420", K=2)[0], f"views {bd} bit +{pitch_extra} at {base}")
    for _v, g in vin:
        g.assert_unchanged("an input view")
    for _v, g in vout:
        g.assert_margin_intact("an output view")


# -------------------------------------------------------------------------------------------------- batches and queueing
@pytest.mark.parametrize("batch", [1, 2, 6, 7])
def test_batches_of_1_2_n_and_n_plus_1(batch):
    frames = LC.grainy(6, 66, 50, 8, "420", seed=50)
    check(frames, 8, "420", f"batch {batch}", batch=batch, K=2, D=1)


def test_a_drain_in_mid_clip_and_two_clips_with_a_sync_between():
    bd, ss, D = 8, "420", 1
    frames = LC.grainy(7, 66, 50, bd, ss, seed=51)
    dev = [_to_dev(f, bd) for f in frames]
    one = reference(frames, bd, ss, K=2, D=D)
    dn = denoiser(bd, 4, K=2, D=D)
    outs = []
    for k, f in enumerate(dev):
        outs.append(dn.apply(f, 1, 1, sync=False))
        if k in (0, 2, 5):
            done = dn.drain()
            assert done == max(k + 1 - D, 0), (k, done)
            if done:
                assert_planes_equal(outs[done - 1], one[done - 1], f"frame {done - 1} after the drain at {k}: counted only when its merge is done")
    dn.sync()
    assert_clips_equal(outs, one, "one clip with drains")
    got = dn.denoise_clip(dev[:3], 1, 1) + dn.denoise_clip(dev[3:], 1, 1)
    want = reference(frames[:3], bd, ss, K=2, D=D) + reference(frames[3:], bd, ss, K=2, D=D)
    assert_clips_equal(got, want, "two clips")
    assert any((a != b).any() for a, b in zip(one[2], want[2])), "one clip of seven is something else"
    dn.close()


def test_a_geometry_change_in_mid_queue_and_back():
    bd, D = 10, 1
    frames = LC.grainy(6, 100, 60, bd, "420", seed=52)
    small = LC.grainy(3, 71, 51, bd, "444", seed=53)
    dev = [_to_dev(f, bd) for f in frames]
    dn = denoiser(bd, K=2, D=D)
    outs = [dn.apply(f, 1, 1, sync=False) for f in dev[:3]]
    outs_small = [dn.apply(f, 0, 0, sync=False) for f in small]
    assert dn.drain() == 3 + 2, "the first clip is complete, and the second up to its last frame"
    outs_again = [dn.apply(f, 1, 1, sync=False) for f in dev[3:]]
    dn.sync()
    assert_clips_equal(outs, reference(frames[:3], bd, "420", K=2, D=D), "before the geometry change")
    assert_clips_equal(outs_small, reference(small, bd, "444", K=2, D=D), "the other geometry")
    assert_clips_equal(outs_again, reference(frames[3:], bd, "420", K=2, D=D), "after it")
    dn.close()


def test_no_coarse_level_is_the_filter_as_it_was():
    from grav1synth_amd.denoise import Denoiser

    frames = LC.grainy(3, 129, 97, 10, "420", seed=54)
    dev = [_to_dev(f, 10) for f in frames]
    a, b = Denoiser(10, temporal_radius=1, joint_chroma=True), Denoiser(10, temporal_radius=1, joint_chroma=True, coarse_levels=0)
    want = a.denoise_clip(dev, 1, 1)
    assert_clips_equal(b.denoise_clip(dev, 1, 1), [[p.cpu().numpy() for p in f] for f in want], "coarse_levels = 0")
    b.kernel_times(True)
    b.denoise_clip(dev, 1, 1)
    assert b.level_time() == 0.0
    a.close(), b.close()
    c = denoiser(10, K=1)
    c.kernel_times(True)
    c.denoise_clip(dev, 1, 1)
    ms, n = c.kernel_times(True)
    assert n == 3 and 0.0 < c.level_time() < ms, (c.level_time(), ms)
    c.close()


# ---------------------------------------------------------------------------------------------------------------- limits
@pytest.mark.parametrize("io", ["in", "out"])
def test_far_views(io):
    """256 x 160 mono under a pitch of 2^24 + 18 at base 6: rows of every alignment, the last one beyond 2^31 bytes"""
    from tests.test_gpu_limits import FAR_H, FAR_W, _guards_hold, _need, edge_planes
    from tests.test_gpu_limits_forms import OWN_PITCH, _mono_io, _pitch, _release

    _need(_pitch(OWN_PITCH)[0] * FAR_H)
    planes = edge_planes(FAR_W, FAR_H, 10, 1, 1, mono=True, seed=60)
    vin, vout, gin, gout = _mono_io(planes[0], OWN_PITCH, io, 10)
    dn = denoiser(10, K=2)
    try:
        got = dn.apply(vin, 1, 1, out=vout)
    finally:
        dn.close()
    assert_planes_equal(got, reference([planes], 10, "mono", K=2)[0], f"far {io}")
    _guards_hold(gin, gout, f"far {io}")
    del vin, vout, gin, gout, got
    _release()


@pytest.mark.parametrize("w,h", [(65536, 8), (8, 65536)])
def test_the_longest_sides(w, h):
    frames = LC.grainy(1, w, h, 8, "420", seed=61)
    check(frames, 8, "420", f"{w}x{h}", K=2, A=1, S=1)


# -------------------------------------------------------------------------------------------------------------- commands
def test_the_commands_byte_for_byte(tmp_path):
    from grav1synth_amd.ingest import diff_y4m_file_denoised
    from tests.test_gpu_denoise import _clip, _run

    bd, ss = 8, "420"
    src, frames = _clip(tmp_path, 5)  # (320 x 192 with flat blocks and a scene cut: content `diff` makes a table from)
    out, keep, tbl, tbl2 = (tmp_path / n for n in ("den.y4m", "keep.y4m", "a.tbl", "b.tbl"))
    p = _run("denoise", str(src), "-o", str(out), "--coarse-levels", "2", "--coarse-ratio", "0.5", "--temporal-radius", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    assert "Denoised 5 frames" in p.stderr
    assert_clips_equal(_y4m_frames(out, 5), reference(frames, bd, ss, K=2, rho=0.5, D=1), "denoise --coarse-levels 2 --coarse-ratio 0.5")
    p = _run("diff", str(src), "--denoise", "--coarse-levels", "1", "--keep-denoised", str(keep), "-o", str(tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    assert_clips_equal(_y4m_frames(keep, 5), reference(frames, bd, ss, K=1), "diff --denoise --coarse-levels 1 --keep-denoised")
    p = _run("diff", str(src), str(keep), "-o", str(tbl2))
    assert p.returncode == 0, p.stderr[-2000:]
    assert tbl.read_bytes() == tbl2.read_bytes(), "the table is the two-file diff's"
    # the file call, and a refusal through it
    assert diff_y4m_file_denoised(str(src), str(tmp_path / "c.tbl"), coarse_levels=1) == 5
    assert (tmp_path / "c.tbl").read_bytes() == tbl.read_bytes()
    with pytest.raises(RuntimeError) as e:
        diff_y4m_file_denoised(str(src), str(tmp_path / "d.tbl"), coarse_ratio=0.5)
    assert "coarse_ratio needs coarse_levels" in str(e.value)
