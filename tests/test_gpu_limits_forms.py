"""The forms of `denoise`, `measure` and the noise levels that are newer than tests/test_gpu_limits.py, at the same limits of
addressing and with that file's machinery: joint chroma and its chroma gain, the grain prior, motion, the noise levels, the
temporal, cross and scales meters.  Against the references the operations' own fixed tests use, bit for bit or refused --
whichever include/g1s_diff.h documents; no test accepts either, and there is no tolerance anywhere.

A. 65 536 samples a side (8 the other way; the scales meter is there already): right; 65 537 refused, and the refusal sticky.
B. 256 x 160 planes as far views under tests/test_gpu_limits.py's four pitches of 2^24 and 2^25 bytes, and under one of this
   file's own, 2^24 + 18 at base offset 6: row r starts 6 + 2 r bytes past a 16-byte boundary, so one row in eight is 16-byte
   aligned, the other odd rows 4-byte and the even rows 2-byte aligned (8-byte aligned one row in four), which is what
   curve_row (the grain prior) and est_load (the noise levels) choose their loads and stores by, row by row; the four keep
   every row aligned.  The grain prior, the noise levels, the cross and the scales meter run under it.  No case takes more than 10 GiB
   (but for the few KiB by which a pitch of 2^25 + 48 exceeds 2^25, as in tests/test_gpu_limits.py); every case calls _need
   first, and one that does not fit the free device memory skips with both numbers.
C. Motion on ordinary views: a pitch, an odd base, and a margin of full-range samples where the displaced staging would read.

tests/test_limits_forms_cpu.py builds the content and shows on the references alone that it bites: the pans are found in
every block, a row offset kept in 32 bits would change what is compared here, and the clamps take part at the odd sizes."""
from __future__ import annotations

import numpy as np
import pytest

from tests import denoise_curve_ref as CR
from tests import measure_ref as R
from tests import measure_s_ref as S
from tests import measure_t_ref as T
from tests import measure_x_ref as X
from tests import nlf_ref as NR
from tests import views as V
from tests.test_gpu_limits import FAR_H, FAR_PITCHES, FAR_W, FRAME_LIMIT_SHAPES, _blank_far, _far_planes, _guards_hold, _io, _need, edge_planes
from tests.test_limits_forms_cpu import (FAR_MR, LIMIT_MR, ODD_SHAPES, VIEW_MR, curve_planes, far_clip, joint_frames, joint_reference, limit_clip,
                                         measure_pairs, motion_reference, nlf_planes, view_clip)
from tests.views import contiguous

pytestmark = pytest.mark.gpu
GEOMETRY = "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)"
OWN_PITCH = "2^24+18_base6"
OWN = ((1 << 24) + 18, 6, 1 << 31)  # (pitch, base offset, the boundary the last row lies beyond)
SMALL_PITCHES = [p for p, v in FAR_PITCHES.items() if v[0] < 1 << 25]
ALL_PITCHES = list(FAR_PITCHES) + [OWN_PITCH]


def _dev(planes):
    return [contiguous(p) for p in planes]


def _release():
    import torch

    torch.cuda.empty_cache()


def _records_equal(got, wants, ref, what):
    """every field of every record, with the reference module's own field-by-field mismatches()"""
    assert len(got) == len(wants), f"{what}: {len(got)} records, want {len(wants)}"
    bad = [line for k, want in enumerate(wants) for line in ref.mismatches(got[k], want, f"{what}, record {k}")]
    assert not bad, "\n".join(bad[:40])


def _ordinary_equal(got, pairs, what):
    _records_equal(got, [R.measure_frame(n, c, 12, 1, 1) for n, c in pairs], R, f"{what}, ordinary")


# ---- A. 65 536 samples a side ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", FRAME_LIMIT_SHAPES)
@pytest.mark.parametrize("bd,ss", [(8, "mono"), (10, "420")])
def test_motion_at_65536_samples_a_side(w, h, bd, ss):
    """3 panned frames, temporal radius 1, motion range 16 (4:2:0: joint chroma): the vectors of frame 0 towards frame 1 from
    device and from host frames, every output plane, the inputs afterwards."""
    from tests.test_gpu_denoise_motion import check

    check(limit_clip(w, h, bd, ss), bd, ss, 1, LIMIT_MR, f"{w}x{h} {bd} bit {ss}", **(dict(joint=True) if ss == "420" else {}))


# (the odd sizes at D = 1 and the gain at D = 1 would take this file past the running time of tests/test_gpu_limits.py: the
# references of three frames of 65 536 samples are what costs; the depths are thinned, not the orientations)
JOINT_LIMITS = [(w, h, D) for w, h in FRAME_LIMIT_SHAPES for D in (0, 1)] + [(w, h, 0) for w, h in ODD_SHAPES]
GAIN_LIMITS = [(w, h, 0) for w, h in FRAME_LIMIT_SHAPES + ODD_SHAPES]


@pytest.mark.parametrize("w,h,D", JOINT_LIMITS)
def test_joint_chroma_at_65536_and_65535_samples_a_side(w, h, D):
    """10-bit 4:2:0: one frame at D = 0, three at D = 1.  At 65 535 x 9 and 9 x 65 535 the guide's last row and column clamp."""
    from tests.test_gpu_denoise_joint import joint_clip
    from tests.test_gpu_denoise_temporal import assert_clips_equal

    frames = joint_frames(w, h, 3 if D else 1)
    assert_clips_equal(joint_clip(frames, 10, (1, 1), temporal_radius=D), joint_reference(frames, D), f"{w}x{h} D {D}")


@pytest.mark.parametrize("w,h,D", GAIN_LIMITS)
def test_joint_chroma_with_a_steep_gain_at_65536_and_65535_samples_a_side(w, h, D):
    from tests.test_gpu_denoise_gain import gain_clip, steep_gain
    from tests.test_gpu_denoise_temporal import assert_clips_equal

    frames = joint_frames(w, h, 3 if D else 1, seed=75)
    gain = steep_gain()
    assert_clips_equal(gain_clip(frames, 10, (1, 1), gain, temporal_radius=D), joint_reference(frames, D, gain), f"{w}x{h} D {D}")


@pytest.mark.parametrize("w,h,D", [(8, 65536, 0), (65536, 8, 1)])
def test_grain_prior_at_65536_samples_a_side(w, h, D):
    """The tallest plane, and the widest one with a temporal radius: the stabilised ring's rows and planes at their largest."""
    from tests.test_gpu_denoise_curve import check_clip, curve

    check_clip(curve_planes(w, h, 3 if D else 1), 10, (1, 1), curve("example", 10), f"{w}x{h} D {D}", D=D, A=2, S=1, strength=8.0)


@pytest.mark.parametrize("w,h", FRAME_LIMIT_SHAPES)
def test_temporal_meter_at_65536_samples_a_side_with_extreme_residuals_at_the_far_edge(w, h):
    """3 pairs, 12-bit 4:2:0, batches of 2, the ordinary records fetched after the first batch: the third pair's predecessor
    lives in the batch before and is read from the meter's own copy of it."""
    from grav1synth_amd.measure import GrainMeter

    pairs = measure_pairs(w, h, 3, extreme_edge=True)
    m = GrainMeter(12, batch_frames=2, temporal=True)
    try:
        for noisy, clean in pairs[:2]:
            m.measure(_dev(noisy), _dev(clean), 1, 1)
        ordinary = list(m.finish())
        m.measure(_dev(pairs[2][0]), _dev(pairs[2][1]), 1, 1)
        got = m.finish_temporal()
        ordinary += list(m.finish())
    finally:
        m.close()
    _records_equal(got, T.run_records(pairs, 12, 1, 1), T, f"{w}x{h}")
    _ordinary_equal(ordinary, pairs, f"{w}x{h}")


@pytest.mark.parametrize("w,h", ODD_SHAPES)
def test_cross_meter_at_65535_samples_a_side(w, h):
    """The luma box under the last chroma row and column clamps (rule 12 of `measure`)."""
    from grav1synth_amd.measure import GrainMeter

    pairs = measure_pairs(w, h, 1, seed=7, amp=300)
    m = GrainMeter(12, cross=True)
    try:
        m.measure(_dev(pairs[0][0]), _dev(pairs[0][1]), 1, 1)
        got, ordinary = m.finish_cross(), m.finish()
    finally:
        m.close()
    _records_equal(got, [X.cross_frame(n, c, 12, 1, 1) for n, c in pairs], X, f"{w}x{h}")
    _ordinary_equal(ordinary, pairs, f"{w}x{h}")


def _zeros(w, h, nplanes):
    shapes = [(h, w)] + [((h + 1) // 2, (w + 1) // 2)] * (nplanes - 1)
    return [np.zeros(s, np.uint16) for s in shapes]


@pytest.mark.parametrize("w,h", [(65537, 8), (8, 65537)])
@pytest.mark.parametrize("op", ["motion", "motion_vectors", "joint", "temporal_meter"])
def test_one_more_is_refused_and_the_refusal_is_sticky(op, w, h):
    """G1S_ERR_INVALID with the documented text from the call that was handed the frame; errors of a denoiser and of a meter
    are sticky (include/g1s_diff.h), so a legal frame afterwards meets the same refusal."""
    from grav1synth_amd import _lib
    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.measure import GrainMeter

    nplanes = 1 if op.startswith("motion") else 3
    big, legal = _dev(_zeros(w, h, nplanes)), _dev(_zeros(64, 48, nplanes))
    if op == "temporal_meter":
        obj = GrainMeter(10, temporal=True)
        call = lambda f: obj.measure(f, f, 1, 1)
    else:
        obj = Denoiser(10, temporal_radius=1, motion_range=LIMIT_MR) if nplanes == 1 else Denoiser(10, joint_chroma=True)
        call = (lambda f: obj.motion_vectors(f, f, 1, 1)) if op == "motion_vectors" else (lambda f: obj.apply(f, 1, 1))
    try:
        for frame in (big, legal):
            with pytest.raises(_lib.G1SError) as e:
                call(frame)
            assert e.value.code == -1 and GEOMETRY in str(e.value), str(e.value)
    finally:
        obj.close()


# ---- B. far views ---------------------------------------------------------------------------------------------------------------

def _pitch(pitch_name):
    return OWN if pitch_name == OWN_PITCH else FAR_PITCHES[pitch_name][:3]


def _mono_io(plane, pitch_name, io, bd):
    """_io for one plane under any of the five pitches: ([input], [output], input guards, output guards)"""
    import torch

    pitch, off, boundary = _pitch(pitch_name)
    vin, gin = _far_planes([plane], pitch, off, boundary, bd) if io != "out" else ([contiguous(plane)], [])
    if io == "in":
        return vin, [torch.zeros(plane.shape, dtype=vin[0].dtype, device="cuda")], gin, []
    v, g = _blank_far(plane, pitch, off, 50)
    assert v[plane.shape[0] - 1:].data_ptr() - v.data_ptr() + plane.shape[1] * plane.dtype.itemsize > boundary
    return vin, [v], gin, [g]


def _alignments(view):
    """the alignment of every row's first sample: 16, 8, 4 or 2 (bytes)"""
    return {next(a for a in (16, 8, 4, 2, 1) if view[r:].data_ptr() % a == 0) for r in range(view.shape[0])}


def _side(planes, far, pitch, off, boundary, bd, seed, only_luma=False, chroma_pitch=None):
    """(device planes, guards): far views of the planes (of the luma alone: the chroma contiguous) or contiguous tensors"""
    if not far:
        return _dev(planes), []
    if only_luma:
        v, g = _far_planes(planes[:1], pitch, off, boundary, bd, seed=seed)
        return v + _dev(planes[1:]), g
    return _far_planes(planes, pitch, off, boundary, bd, seed=seed, chroma_pitch=chroma_pitch)


def _frame_bytes(pitch, nplanes):
    return pitch * FAR_H + (2 * ((pitch // 2 + 15) & ~15) * (FAR_H // 2) if nplanes == 3 else 0)


JOINT_FAR = [(p, io) for p in SMALL_PITCHES for io in ("in", "out", "both")]


@pytest.mark.parametrize("pitch_name,io", JOINT_FAR, ids=[f"{p}-{io}" for p, io in JOINT_FAR])
def test_joint_chroma_on_far_views(pitch_name, io):
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_grain import assert_planes_equal

    _need(FAR_PITCHES[pitch_name][0] * (FAR_H + FAR_H // 2) * (2 if io == "both" else 1))  # (_io asks again, for the same bytes)
    frame = joint_frames(FAR_W, FAR_H, 1)[0]
    vin, vout, gin, gout = _io(frame, pitch_name, io, 10)
    dn = Denoiser(10, joint_chroma=True)
    try:
        got = dn.apply(vin, 1, 1, out=vout)
    finally:
        dn.close()
    assert_planes_equal(got, joint_reference([frame], 0)[0], f"{pitch_name} {io}")
    _guards_hold(gin, gout, f"{pitch_name} {io}")
    del vin, vout, gin, gout, got
    _release()


@pytest.mark.parametrize("gain", [False, True], ids=["joint", "steep_gain"])
def test_joint_chroma_with_every_input_plane_under_2_to_the_25(gain):
    """Luma under a pitch of 2^25 (5 GiB) and both chroma planes under the same pitch (80 rows: 2.5 GiB each): the luma rows of
    the guide under a chroma sample lie up to 5 GiB from the plane's origin.  Outputs in ordinary tensors (10 GiB)."""
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise_gain import steep_gain
    from tests.test_gpu_grain import assert_planes_equal

    pitch = 1 << 25
    _need(2 * pitch * FAR_H)
    g = steep_gain() if gain else None
    frame = joint_frames(FAR_W, FAR_H, 1)[0]
    vin, gin = _far_planes(frame, pitch, 0, 1 << 31, 10, chroma_pitch=pitch)
    assert vin[0][FAR_H - 1:].data_ptr() - vin[0].data_ptr() > 1 << 32
    dn = Denoiser(10, joint_chroma=True, chroma_gain=g)
    try:
        got = dn.apply(vin, 1, 1)
    finally:
        dn.close()
    assert_planes_equal(got, joint_reference([frame], 0, g)[0], f"4:2:0 under 2^25, gain {gain}")
    _guards_hold(gin, [], "4:2:0 under 2^25")
    del vin, gin, got
    _release()


CURVE_FAR = [(p, io) for p in ALL_PITCHES for io in ("in", "out", "both")]


@pytest.mark.parametrize("pitch_name,io", CURVE_FAR, ids=[f"{p}-{io}" for p, io in CURVE_FAR])
def test_grain_prior_on_far_views(pitch_name, io):
    """Mono 10-bit: the forward launch reads the caller's plane and the inverse writes the caller's output, row by row."""
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise_curve import curve
    from tests.test_gpu_grain import assert_planes_equal

    _need(_pitch(pitch_name)[0] * FAR_H * (2 if io == "both" else 1))
    cv = curve("example", 10)
    planes = edge_planes(FAR_W, FAR_H, 10, 1, 1, mono=True, seed=82)
    vin, vout, gin, gout = _mono_io(planes[0], pitch_name, io, 10)
    for v in (vin if io != "out" else []) + (vout if io != "in" else []):  # the far views: what curve_row reads, what it writes
        assert _alignments(v) == ({16, 8, 4, 2} if pitch_name == OWN_PITCH else {16}), "rows of every alignment in one plane under the own pitch"
    dn = Denoiser(10, curve=cv)
    try:
        got = dn.apply(vin, 1, 1, out=vout)
    finally:
        dn.close()
    assert_planes_equal(got, [CR.denoise_luma(planes[0], cv[0], cv[1], 3, 2, 4.0)], f"{pitch_name} {io}")
    _guards_hold(gin, gout, f"{pitch_name} {io}")
    del vin, vout, gin, gout, got
    _release()


@pytest.mark.parametrize("pitch_name", list(FAR_PITCHES))
def test_motion_on_far_views_with_far_neighbours(pitch_name):
    """Mono 8-bit, temporal radius 1, motion range 32, a panned clip, every input a far view; the memory plan of
    tests/test_gpu_limits.py test_temporal_denoise_on_far_views_with_far_neighbours: three frames and the middle output far
    under the 2^24 pitches, two frames and ordinary outputs under 2^25.  First the vectors of frame 0 towards frame 1."""
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise_motion import vectors_reference
    from tests.test_gpu_denoise_temporal import assert_clips_equal

    bd = 8
    pitch, off, boundary, _o = FAR_PITCHES[pitch_name]
    small = pitch < 1 << 25
    _need(pitch * FAR_H * (4 if small else 2))
    frames = far_clip(3 if small else 2)
    dn = Denoiser(bd, temporal_radius=1, motion_range=FAR_MR)
    gin, gout, outs, keep = [], [], [], []
    try:
        for t, f in enumerate(frames):
            v, g = _far_planes(f, pitch, off, boundary, bd, seed=t)
            gin += g
            keep.append(v)
        got_mv = dn.motion_vectors(keep[0], keep[1], 1, 1)
        for t, (f, v) in enumerate(zip(frames, keep)):
            if small and t == 1:
                vo, go = _blank_far(f[0], pitch, off, 60 + t)
                gout.append(go)
                outs.append(dn.apply(v, 1, 1, sync=False, out=[vo]))
            else:
                outs.append(dn.apply(v, 1, 1, sync=False))
        dn.sync()
    finally:
        dn.close()
    want_mv = vectors_reference(frames[0], frames[1], FAR_MR)
    assert len(got_mv) == 1 and got_mv[0].dtype == np.int16 and np.array_equal(got_mv[0], want_mv[0]), f"{pitch_name}: vectors {got_mv[0].tolist()} vs {want_mv[0].tolist()}"
    assert_clips_equal(outs, motion_reference(frames, bd, "mono", FAR_MR), pitch_name)
    _guards_hold(gin, gout, pitch_name)
    del keep, outs, gin, gout
    _release()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("far", ["luma", "chroma"])
@pytest.mark.parametrize("pitch_name", ALL_PITCHES)
def test_noise_levels_on_far_views(pitch_name, far, bd):
    """4:2:0: the luma far and the chroma contiguous (chroma is binned by luma rows gigabytes apart), and the other way round
    (both chroma planes of 80 rows under the whole pitch: 1.25 or 2.5 GiB each).  Under the own pitch est_load meets, in one
    far plane, rows it reads 16 (at 8 bits: 8) bytes at a time and rows it reads in 4- and 2-byte (single-byte) pieces; the
    luma rows under the chroma rows are the even ones, all of them read in the narrowest pieces, where the four pitches have
    them all aligned."""
    from grav1synth_amd.estimate import NoiseLevelMeter

    pitch, off, boundary = _pitch(pitch_name)
    _need(pitch * FAR_H)
    planes = nlf_planes(bd)
    want = NR.nlf_frame(planes, bd, 1, 1)
    if far == "luma":
        dev, guards = _side(planes, True, pitch, off, boundary, bd, 0, only_luma=True)
    else:
        v, guards = _far_planes(planes[1:], pitch, off, boundary // 2, bd, seed=1, chroma_pitch=pitch)
        dev = _dev(planes[:1]) + v
    for v in dev[:1] if far == "luma" else dev[1:]:
        assert _alignments(v) == ({16, 8, 4, 2} if pitch_name == OWN_PITCH else {16}), "rows of every alignment in one far plane under the own pitch"
        if pitch_name == OWN_PITCH and far == "luma":
            assert all(v[r:].data_ptr() % 4 == 2 for r in range(0, FAR_H, 2)), "the rows chroma is binned by"
    m = NoiseLevelMeter(bd)
    try:
        m.frame(dev, 1, 1)
        got = m.finish()
    finally:
        m.close()
    _records_equal(got, [want], NR, f"{pitch_name} {far} {bd} bit")
    _guards_hold(guards, [], f"{pitch_name} {far}")
    del dev, guards
    _release()


TEMPORAL_FAR = [(p, which, 0) for p in FAR_PITCHES for which in ("noisy", "clean", "both")] + [("2^25+48_base48", "noisy", 1), ("2^24", "both", 1)]


@pytest.mark.parametrize("pitch_name,which,batch", TEMPORAL_FAR, ids=[f"{p}-{w}-batch{b}" for p, w, b in TEMPORAL_FAR])
def test_temporal_meter_on_far_views(pitch_name, which, batch):
    """2 pairs, 12 bit: mono under 2^25, 4:2:0 under 2^24.  noisy / clean: that side of both pairs far; both: the predecessor
    pair far on both sides (10 GiB; under 2^25 + 48 that is 15 KiB more, as the cases of tests/test_gpu_limits.py under that
    pitch are).  batch 0: one batch, the predecessor read in place.  batch 1: batches of one and the ordinary record fetched
    between the pairs, so the far predecessor is copied under its pitch at the hand-over."""
    from grav1synth_amd.measure import GrainMeter

    pitch, off, boundary, _o = FAR_PITCHES[pitch_name]
    mono = pitch >= 1 << 25  # (tests/test_gpu_limits.py _far_frame_planes' rule: two 4:2:0 frames under 2^25 do not fit 10 GiB)
    _need(2 * _frame_bytes(pitch, 1 if mono else 3))
    pairs = measure_pairs(FAR_W, FAR_H, 2, mono=mono, seed=51, amp=300)
    guards, keep, ordinary = [], [], []
    m = GrainMeter(12, batch_frames=batch, temporal=True)
    try:
        for k, pair in enumerate(pairs):
            devs = []
            for j, (name, planes) in enumerate(zip(("noisy", "clean"), pair)):
                v, g = _side(planes, which == name or (which == "both" and k == 0), pitch, off, boundary, 12, 2 * k + j)
                devs.append(v), guards.extend(g)
            keep.append(devs)
            m.measure(devs[0], devs[1], 1, 1)
            if batch:
                ordinary += list(m.finish())
        got = m.finish_temporal()
        ordinary += list(m.finish())
    finally:
        m.close()
    _records_equal(got, T.run_records(pairs, 12, 1, 1), T, f"{pitch_name} {which}")
    _ordinary_equal(ordinary, pairs, f"{pitch_name} {which}")
    _guards_hold(guards, [], f"{pitch_name} {which}")
    del keep, guards
    _release()


CROSS_FAR = [(p, "luma") for p in ALL_PITCHES] + [(p, "all") for p in SMALL_PITCHES + [OWN_PITCH]]


@pytest.mark.parametrize("pitch_name,far", CROSS_FAR, ids=[f"{p}-{f}" for p, f in CROSS_FAR])
def test_cross_meter_on_far_views(pitch_name, far):
    """4:2:0 12-bit, noisy and clean alike: the luma far and the chroma contiguous (10 GiB under 2^25), or all planes far."""
    from grav1synth_amd.measure import GrainMeter

    pitch, off, boundary = _pitch(pitch_name)
    _need(2 * _frame_bytes(pitch, 1 if far == "luma" else 3))
    pairs = measure_pairs(FAR_W, FAR_H, 1, seed=61, amp=300)
    devs, guards = [], []
    for j, planes in enumerate(pairs[0]):
        v, g = _side(planes, True, pitch, off, boundary, 12, j, only_luma=far == "luma")
        devs.append(v), guards.extend(g)
    m = GrainMeter(12, cross=True)
    try:
        m.measure(devs[0], devs[1], 1, 1)
        got, ordinary = m.finish_cross(), m.finish()
    finally:
        m.close()
    _records_equal(got, [X.cross_frame(n, c, 12, 1, 1) for n, c in pairs], X, f"{pitch_name} {far}")
    _ordinary_equal(ordinary, pairs, f"{pitch_name} {far}")
    _guards_hold(guards, [], f"{pitch_name} {far}")
    del devs, guards
    _release()


SCALES_FAR = [(p, which) for p in ALL_PITCHES for which in ("noisy", "clean")] + [(p, "both") for p in SMALL_PITCHES + [OWN_PITCH]]


@pytest.mark.parametrize("pitch_name,which", SCALES_FAR, ids=[f"{p}-{w}" for p, w in SCALES_FAR])
def test_scales_meter_on_far_views(pitch_name, which):
    """4:2:0 12-bit, 256 x 160: 5 rows of boxes of 32, the last one wholly beyond the boundary (both sides far: the 2^24 pitches).  Under the
    own pitch the 8-sample loads of km_measure_s are possible in one row of eight only."""
    from grav1synth_amd.measure import GrainMeter

    pitch, off, boundary = _pitch(pitch_name)
    _need((2 if which == "both" else 1) * _frame_bytes(pitch, 3))
    pairs = measure_pairs(FAR_W, FAR_H, 1, seed=71, amp=300)
    devs, guards = [], []
    for j, (name, planes) in enumerate(zip(("noisy", "clean"), pairs[0])):
        v, g = _side(planes, which in (name, "both"), pitch, off, boundary, 12, j)
        devs.append(v), guards.extend(g)
    m = GrainMeter(12, scales=True)
    try:
        m.measure(devs[0], devs[1], 1, 1)
        got, ordinary = m.finish_scales(), m.finish()
    finally:
        m.close()
    _records_equal(got, [S.scale_frame(n, c, 12, 1, 1) for n, c in pairs], S, f"{pitch_name} {which}")
    _ordinary_equal(ordinary, pairs, f"{pitch_name} {which}")
    _guards_hold(guards, [], f"{pitch_name} {which}")
    del devs, guards
    _release()


# ---- C. motion on ordinary views -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("joint", [False, True], ids=["plain", "joint"])
def test_motion_on_views_with_a_pitch_an_odd_base_and_a_hostile_margin(joint):
    """129 x 97 4:2:0 10-bit, 5 panned frames in batches of 2, motion range 32.  The margin holds samples of the whole code
    range: the half-resolution staging clamps at (W + 1) >> 1, and a neighbour tile is staged from an origin that lies outside
    the plane by up to the range, so anything read past a row or below the plane changes a vector or a weight."""
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise_motion import vectors_reference
    from tests.test_gpu_denoise_temporal import assert_clips_equal

    bd = 10
    frames = view_clip()
    dn = Denoiser(bd, temporal_radius=1, motion_range=VIEW_MR, batch_frames=2, joint_chroma=joint)
    vins, guards_in, guards_out, outs = [], [], [], []
    try:
        for t, planes in enumerate(frames):
            vin = [V.device_view(p, pitch_bytes=p.shape[1] * 2 + 26 + 2 * c, base_offset_bytes=6 + 2 * c, max_code=1023, seed=t) for c, p in enumerate(planes)]
            guards_in += [g for _v, g in vin]
            vins.append([v for v, _g in vin])
        got_mv = dn.motion_vectors(vins[0], vins[1], 1, 1)
        for t, planes in enumerate(frames):
            vout = [V.device_view(np.zeros_like(p), pitch_bytes=p.shape[1] * 2 + 18, base_offset_bytes=10, fill="max", max_code=1023, seed=t) for p in planes]
            guards_out += [g for _v, g in vout]
            outs.append(dn.apply(vins[t], 1, 1, sync=False, out=[v for v, _g in vout]))
        dn.sync()
    finally:
        dn.close()
    want_mv = vectors_reference(frames[0], frames[1], VIEW_MR, joint)
    for c, (a, b) in enumerate(zip(got_mv, want_mv)):
        assert a.dtype == np.int16 and np.array_equal(a, b), f"vectors of plane {c}: {a.tolist()} vs {b.tolist()}"
    assert_clips_equal(outs, motion_reference(frames, bd, "420", VIEW_MR, joint=joint), f"views, joint {joint}")
    for g in guards_in:
        g.assert_unchanged("a strided input")
    for g in guards_out:
        g.assert_margin_intact("a strided output")
