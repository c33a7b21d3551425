"""The content of tests/test_gpu_limits_forms.py, held to what it is meant to reach.  No device and no torch: numpy, the
references of the operations' own tests (imported from those test modules, as the project's other *_cpu files do) and, for
the weight tables, curves and gains those references take, the host-only calls of the built library.

The GPU file feeds the forms of `denoise`, `measure` and the noise levels that are newer than tests/test_gpu_limits.py with
frames of 65 536 samples a side and with 256 x 160 planes whose rows lie 2^24 or 2^25 bytes apart.  A case proves something
only if the content makes a wrong address visible.  This file builds that content (the GPU file imports it from here) and
asserts, on the references alone:

1. the panned clips have nonzero reference vectors in the last block column and row and in at least 90 % of all blocks: the
   displaced staging of the motion forms is reached at the far edge;
2. a row offset kept in 32 bits would be seen.  Under a pitch of 2^25 bytes row r of a 160-row plane wraps onto row r - 128
   for r >= 128 (under 2^24 a signed offset goes negative from there).  For one role at a time -- the joint guide's luma, a
   motion neighbour, the cross meter's luma, the temporal meter's predecessor, the luma the noise levels bin chroma by, ... --
   the reference on planes whose rows 128 .. 159 are rows 0 .. 31 differs from the true one in what the GPU test compares;
3. at the odd luma sizes the clamp of denoise's rule 8 and of measure's rule 12 takes part: the reference that reads one row /
   column further, on a padded plane, differs."""
from __future__ import annotations

import numpy as np
import pytest

from tests import denoise_curve_ref as CR
from tests import denoise_joint_ref as J
from tests import measure_ref as R
from tests import measure_s_ref as S
from tests import measure_t_ref as T
from tests import measure_x_ref as X
from tests import nlf_ref as NR
from tests.test_gpu_limits import FAR_H, FAR_W, FRAME_LIMIT_SHAPES, edge_planes

WIDE, TALL = FRAME_LIMIT_SHAPES
ODD_SHAPES = [(65535, 9), (9, 65535)]
LIMIT_SHIFTS = {WIDE: [(10, 0), (-6, 0)], TALL: [(0, -6), (0, 4)]}  # a pan along the long side, another one every interval
LIMIT_MR, FAR_MR, VIEW_MR = 16, 32, 32
FAR_SHIFTS = [(10, -6), (-12, 4)]
VIEW_SHIFTS = [(10, -6), (-12, 4), (18, 2), (-4, -8)]
WRAP = 128  # the first row of a 160-row plane whose offset under a pitch of 2^25 bytes needs bit 32 (under 2^24: bit 31)


# ---- content (the GPU file's, built here so that both files see the same planes) ---------------------------------------------

def limit_clip(w, h, bd, ss):
    """3 frames of w x h, every plane a window that pans over its own noise world by LIMIT_SHIFTS, grain on each."""
    from tests.test_gpu_denoise_motion import panned

    return panned(3, w, h, bd, ss, LIMIT_SHIFTS[(w, h)], seed=1)


def far_clip(n=3):
    from tests.test_gpu_denoise_motion import panned

    return panned(n, FAR_W, FAR_H, 8, "mono", FAR_SHIFTS, seed=1)


def view_clip():
    from tests.test_gpu_denoise_motion import panned

    return panned(5, 129, 97, 10, "420", VIEW_SHIFTS, seed=5)


def joint_frames(w, h, n, seed=70):
    """10-bit 4:2:0 frames for the joint forms: gentle sawtooth slopes with noise of a few 8-bit code values, so that patches
    a few samples apart keep a weight and the guide decides it; the last 64 columns and 48 rows of every plane (or the last
    half, if the plane is smaller) carry slopes of their own.  (edge_planes' far pattern is so steep that only d = 0 keeps a
    weight there: the output is the input whatever the guide is.)"""
    frames = []
    for t in range(n):
        rng = np.random.default_rng([seed, t, w, h])
        planes = []
        for c, (ph, pw) in enumerate([(h, w)] + [((h + 1) >> 1, (w + 1) >> 1)] * 2):
            ys, xs = np.arange(ph)[:, None], np.arange(pw)[None, :]
            near = 100 + 4 * (((1 + c) * xs + (2 + c) * ys + 17 * t) % 200)
            far = 300 + 2 * ((3 * xs + (1 + c) * ys + 31 * c + 5 * t) % 200)
            edge = (xs >= pw - min(64, pw // 2)) | (ys >= ph - min(48, ph // 2))
            planes.append(np.clip(np.where(edge, far, near) + rng.integers(-20, 21, (ph, pw)), 0, 1023).astype(np.uint16))
        frames.append(planes)
    return frames


def curve_planes(w, h, n, seed=9):
    """10-bit luma planes for the grain prior: tests/test_gpu_denoise_curve.py's widest plane, turned for a tall one."""
    out = []
    for t in range(n):
        y = np.random.default_rng(seed + t).integers(0, 1024, (h, w)).astype(np.uint16)
        if w >= h:
            y[:, ::2] = (np.arange((w + 1) // 2)[None, :] // 32 % 1024).astype(np.uint16)
        else:
            y[::2, :] = (np.arange((h + 1) // 2)[:, None] // 32 % 1024).astype(np.uint16)
        out.append([y])
    return out


def measure_pairs(w, h, n, mono=False, seed=5, amp=40, extreme_edge=False):
    """12-bit (noisy, clean) pairs on edge_planes; extreme_edge: the last column (of a wide frame; row of a tall one) of every
    plane holds residuals of +4095 and -4095 in turn."""
    pairs = []
    for k in range(n):
        clean = edge_planes(w, h, 12, 1, 1, mono=mono, seed=seed + k)
        noisy = [np.clip(p.astype(np.int64) + np.random.default_rng([seed, k, c]).integers(-amp, amp + 1, p.shape), 0, 4095).astype(np.uint16)
                 for c, p in enumerate(clean)]
        if extreme_edge:
            for a_, b_ in zip(noisy, clean):
                a, b = (a_[:, -1], b_[:, -1]) if w > h else (a_[-1, :], b_[-1, :])
                alt = (np.arange(a.size) + k) & 1
                a[...], b[...] = np.where(alt, 4095, 0), np.where(alt, 0, 4095)
        pairs.append((noisy, clean))
    return pairs


def nlf_planes(bd, seed=4):
    """4:2:0 256 x 160 for the noise levels: slopes with little noise (most samples pass the gate), and a luma whose lower
    part is brighter by four bins, so that the chroma under it is binned elsewhere."""
    from tests.test_nlf_cpu import smooth_planes

    planes = smooth_planes(FAR_W, FAR_H, bd, "420", seed=seed)
    top = (1 << bd) - 1
    y = planes[0].astype(np.int64)
    y[FAR_H - 48:] = (y[FAR_H - 48:] + (4 << (bd - 5))) % (top + 1)
    planes[0] = y.astype(planes[0].dtype)
    return planes


def aliased(plane):
    """The plane a 32-bit row offset reads under a pitch of 2^25 bytes: rows 128 .. 159 are rows 0 .. 31."""
    q = np.array(plane, copy=True)
    assert q.shape[0] == FAR_H
    q[WRAP:] = q[:FAR_H - WRAP]
    return q


def padded(plane, fill=0):
    """One more row and column of `fill`: what a guide or a box without its clamp reads at the edge of an odd-sized plane."""
    return np.pad(np.asarray(plane), ((0, 1), (0, 1)), constant_values=fill)


# ---- references with the library's tables -------------------------------------------------------------------------------------

def joint_reference(frames, D, gain=None):
    from tests.test_gpu_denoise_gain import reference as gain_reference
    from tests.test_gpu_denoise_joint import reference

    return reference(frames, 10, (1, 1), D) if gain is None else gain_reference(frames, 10, (1, 1), gain, D)


def motion_reference(frames, bd, ss, mr, joint=False):
    from tests.test_gpu_denoise_motion import reference

    return reference(frames, bd, ss, 1, mr, joint=joint)


def differs(a, b) -> bool:
    """two clips (lists of frames of planes), frames or planes"""
    if isinstance(a, np.ndarray):
        return not np.array_equal(a, b)
    return any(differs(x, y) for x, y in zip(a, b))


def record_differs(a: dict, b: dict) -> bool:
    return any(not np.array_equal(a[k], b[k]) for k in a)


# ---- 1. the pans are found at the far edge ------------------------------------------------------------------------------------

def assert_vectors_bite(fields, what):
    for c, mv in enumerate(fields):
        moved = mv.any(axis=2)
        assert moved[:, -1].all() and moved[-1, :].all(), f"{what}, plane {c}: a zero vector in the last block column or row"
        assert moved.mean() >= 0.9, f"{what}, plane {c}: {moved.mean():.3f} of the blocks moved"


@pytest.mark.parametrize("w,h", FRAME_LIMIT_SHAPES)
@pytest.mark.parametrize("bd,ss", [(8, "mono"), (10, "420")])
def test_the_limit_clips_pan_in_every_block(w, h, bd, ss):
    from tests.test_gpu_denoise_motion import vectors_reference

    frames = limit_clip(w, h, bd, ss)
    fields = vectors_reference(frames[0], frames[1], LIMIT_MR, joint=ss != "mono")
    assert fields[0].shape[:2] == (-(-h // 48), -(-w // 64))
    assert_vectors_bite(fields, f"{w}x{h} {ss}")
    sx, sy = LIMIT_SHIFTS[(w, h)][0]
    assert (fields[0] == (-sx, -sy)).all(), "the pan itself, in every luma block"
    assert_vectors_bite(vectors_reference(frames[1], frames[2], LIMIT_MR, joint=ss != "mono"), f"{w}x{h} {ss}, second interval")


def test_the_far_and_the_view_clip_pan_in_every_block():
    from tests.test_gpu_denoise_motion import vectors_reference

    frames = far_clip()
    assert_vectors_bite(vectors_reference(frames[0], frames[1], FAR_MR), "far clip")
    assert_vectors_bite(vectors_reference(frames[1], frames[2], FAR_MR), "far clip, second interval")
    frames = view_clip()
    for joint in (False, True):
        assert_vectors_bite(vectors_reference(frames[0], frames[1], VIEW_MR, joint), f"view clip, joint {joint}")


# ---- 2. a row offset kept in 32 bits would be seen ----------------------------------------------------------------------------

def test_edge_planes_differ_between_the_rows_a_wrapped_offset_confuses():
    for bd, mono in ((8, True), (10, False), (12, False)):
        y = edge_planes(FAR_W, FAR_H, bd, 1, 1, mono=mono, seed=3)[0]
        assert (y[WRAP:] != y[:FAR_H - WRAP]).mean() > 0.9


@pytest.mark.parametrize("gain", [False, True], ids=["joint", "gain"])
def test_an_aliased_guide_luma_shows_in_the_chroma_output(gain):
    """The 2^25 case: luma and chroma under one pitch.  The guide's luma alone; then each chroma plane alone: its 80 rows end
    2.5 GiB from the first, so only a signed offset goes wrong there, from row 64 on -- other content in those rows stands for it."""
    from tests.test_gpu_denoise_gain import steep_gain

    g = steep_gain() if gain else None
    frame = joint_frames(FAR_W, FAR_H, 1)[0]
    want = joint_reference([frame], 0, g)[0]
    wrong = joint_reference([[aliased(frame[0]), frame[1], frame[2]]], 0, g)[0]
    assert differs(want[1], wrong[1]) and differs(want[2], wrong[2]), "the guide's rows 128 .. 159 reach both chroma planes"
    assert differs(want[0], wrong[0])
    for c in (1, 2):
        low = [p.copy() for p in frame]
        low[c][64:] = low[c][:16]
        wrong = joint_reference([low], 0, g)[0]
        assert differs(want[c], wrong[c])


def test_an_aliased_input_shows_in_the_grain_priors_output():
    from tests.test_gpu_denoise_curve import curve

    cv = curve("example", 10)
    y = edge_planes(FAR_W, FAR_H, 10, 1, 1, mono=True, seed=82)[0]
    want = CR.denoise_luma(y, cv[0], cv[1], 3, 2, 4.0)
    assert differs(want, CR.denoise_luma(aliased(y), cv[0], cv[1], 3, 2, 4.0))
    assert differs(want[WRAP:], want[:FAR_H - WRAP]), "an output row written 4 GiB early would be seen"


def test_an_aliased_motion_neighbour_shows_in_vectors_and_output():
    from tests.test_gpu_denoise_motion import vectors_reference

    frames = far_clip()
    want = motion_reference(frames, 8, "mono", FAR_MR)
    for t in range(3):
        wrong_clip = [[aliased(f[0])] if k == t else f for k, f in enumerate(frames)]
        wrong = motion_reference(wrong_clip, 8, "mono", FAR_MR)
        others = [k for k in range(3) if k != t and abs(k - t) <= 1]
        assert all(differs(want[k], wrong[k]) for k in others), f"frame {t} as a neighbour alone"
    v = vectors_reference(frames[0], frames[1], FAR_MR)[0]
    assert differs(v, vectors_reference(frames[0], [aliased(frames[1][0])], FAR_MR)[0]), "the reference frame of the search"
    assert differs(v, vectors_reference([aliased(frames[0][0])], frames[1], FAR_MR)[0]), "the current frame of the search"


@pytest.mark.parametrize("bd", [8, 10])
def test_an_aliased_plane_shows_in_the_noise_levels(bd):
    planes = nlf_planes(bd)
    want = NR.nlf_frame(planes, bd, 1, 1)
    assert want["n"][0].sum() > 0 and want["n"][1].sum() > 0 and want["q"][1].any()
    wrong = NR.nlf_frame([aliased(planes[0])] + planes[1:], bd, 1, 1)
    assert not np.array_equal(want["n"][1], wrong["n"][1]), "the luma rows chroma is binned by"
    for c in (1, 2):
        low = [p.copy() for p in planes]
        low[c][64:] = low[c][:16]
        assert record_differs(want, NR.nlf_frame(low, bd, 1, 1))


@pytest.mark.parametrize("mono", [True, False])
def test_an_aliased_predecessor_shows_in_the_temporal_record(mono):
    pairs = measure_pairs(FAR_W, FAR_H, 2, mono=mono, seed=51, amp=300)
    want = T.run_records(pairs, 12, 1, 1)[0]
    for side in (0, 1):  # the predecessor's noisy planes alone, its clean planes alone
        prev = list(pairs[0])
        prev[side] = [aliased(prev[side][0])] + list(prev[side][1:])
        wrong = T.run_records([tuple(prev), pairs[1]], 12, 1, 1)[0]
        assert not np.array_equal(want["c"][0], wrong["c"][0]) and not np.array_equal(want["x"][0], wrong["x"][0])
    for side in (0, 1):  # and the current pair's
        cur = list(pairs[1])
        cur[side] = [aliased(cur[side][0])] + list(cur[side][1:])
        assert record_differs(want, T.run_records([pairs[0], tuple(cur)], 12, 1, 1)[0])


def test_an_aliased_luma_shows_in_the_cross_record():
    noisy, clean = measure_pairs(FAR_W, FAR_H, 1, seed=61, amp=300)[0]
    want = X.cross_frame(noisy, clean, 12, 1, 1)
    for side in (0, 1):
        pair = [list(noisy), list(clean)]
        pair[side][0] = aliased(pair[side][0])
        wrong = X.cross_frame(pair[0], pair[1], 12, 1, 1)
        assert not np.array_equal(want["x"][0], wrong["x"][0]) and not np.array_equal(want["c"][1], wrong["c"][1]), "L under Cb and under Cr"
    both = X.cross_frame([aliased(noisy[0])] + noisy[1:], [aliased(clean[0])] + clean[1:], 12, 1, 1)
    assert not np.array_equal(want["x"][0], both["x"][0])


def test_an_aliased_plane_shows_in_the_scale_record():
    noisy, clean = measure_pairs(FAR_W, FAR_H, 1, seed=71, amp=300)[0]
    want = S.scale_frame(noisy, clean, 12, 1, 1)
    assert int(want["n"][0, 4].sum()) == (FAR_W >> 5) * (FAR_H >> 5) == 40, "5 box rows of 32"
    for side in (0, 1):
        pair = [list(noisy), list(clean)]
        pair[side][0] = aliased(pair[side][0])
        wrong = S.scale_frame(pair[0], pair[1], 12, 1, 1)
        assert all(not np.array_equal(want["s2"][0, k], wrong["s2"][0, k]) for k in range(5)), "every scale has boxes in rows 128 .. 159"


# ---- 3. the clamps at the far edge of an odd-sized luma -----------------------------------------------------------------------

@pytest.mark.parametrize("w,h", ODD_SHAPES)
def test_the_guides_clamp_takes_part_at_the_odd_sizes(w, h):
    """Rule 8: min((y << ydec) + j, H - 1).  A guide that reads row H (column W) of a padded plane is another guide in the last
    chroma row (column), and the chroma output there is another one."""
    frame = joint_frames(w, h, 1)[0]
    assert frame[1].shape == ((h + 1) // 2, (w + 1) // 2)
    g, unclamped = J.guide(frame[0], 1, 1), J.guide(padded(frame[0]), 1, 1)
    assert g.shape == unclamped.shape
    assert (g[-1, :] != unclamped[-1, :]).all() and (g[:, -1] != unclamped[:, -1]).all() and np.array_equal(g[:-1, :-1], unclamped[:-1, :-1])
    want = joint_reference([frame], 0)[0]
    wrong = joint_reference([[padded(frame[0]), frame[1], frame[2]]], 0)[0]
    last = (slice(None), slice(-8, None)) if w > h else (slice(-8, None), slice(None))
    assert differs(want[1][last], wrong[1][last]) and differs(want[2][last], wrong[2][last])
    assert (want[1][last] != frame[1][last]).mean() > 0.5, "the filter averages at the far edge"


@pytest.mark.parametrize("w,h", ODD_SHAPES)
def test_the_cross_meters_clamp_takes_part_at_the_odd_sizes(w, h):
    """Rule 12 of `measure`: the luma box under the last chroma row and column repeats the last luma row and column."""
    noisy, clean = measure_pairs(w, h, 1, seed=7, amp=300)[0]
    d = noisy[0].astype(np.int64) - clean[0].astype(np.int64)
    ch, cw = clean[1].shape
    L, unclamped = X.luma_at_chroma(d, cw, ch, 1, 1), X.luma_at_chroma(padded(d), cw, ch, 1, 1)
    assert differs(L[-1, :], unclamped[-1, :]) and differs(L[:, -1], unclamped[:, -1]) and np.array_equal(L[:-1, :-1], unclamped[:-1, :-1])
    want = X.cross_frame(noisy, clean, 12, 1, 1)
    wrong = X.cross_frame([padded(noisy[0], 4095)] + noisy[1:], [padded(clean[0])] + clean[1:], 12, 1, 1)
    assert not np.array_equal(want["x"][0], wrong["x"][0]) and not np.array_equal(want["v"][1], wrong["v"][1])
