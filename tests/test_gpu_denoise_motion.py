"""Motion for the temporal radius of `denoise` on the device (rules 16 - 20 of include/g1s_diff.h) against
tests/denoise_motion_ref.py, byte for byte: the vectors kd_motion finds, every output plane of the filter under them, clips
that cross batches and clip ends, frames of every kind of memory, the flags, the refusals and the two .y4m commands."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import denoise_motion_ref as MR
from tests import motion_content as MC
from tests.test_gpu_denoise import _clip, _run
from tests.test_gpu_denoise_temporal import _y4m_frames, assert_clips_equal
from tests.test_gpu_grain import SUBSAMPLINGS, _to_dev, assert_planes_equal

pytestmark = pytest.mark.gpu

SHIFTS = [(10, -6), (-12, 4), (18, 2), (-4, -8), (6, 6), (2, -14)]  # a different one every interval


def shapes(w, h, ss):
    if ss == "mono":
        return [(w, h)]
    sx, sy = SUBSAMPLINGS[ss]
    return [(w, h)] + [((w + sx) >> sx, (h + sy) >> sy)] * 2


def sub(ss):
    return (1, 1) if ss == "mono" else SUBSAMPLINGS[ss]


def panned(n, w, h, bd, ss, shifts=SHIFTS, seed=0, sigma=2.0, kind="noise"):
    """n frames: every plane a window of its own noise world, panned by shifts[t] (in the plane's samples) from frame t to
    frame t + 1, grain of `sigma` 8-bit code values on each."""
    per_plane = [MC.pan([seed, c, w, h], pw, ph, bd, list(shifts[:n - 1]), sigma * (1 << (bd - 8)), kind)[1] for c, (pw, ph) in enumerate(shapes(w, h, ss))]
    return MC.clip(per_plane)


def tables(bd, S, strength, joint=False, curve=False):
    from grav1synth_amd.denoise import weight_table

    return weight_table(12 if curve else bd, S, strength), weight_table(bd, S, strength, joint_chroma=joint)


def reference(frames, bd, ss, D, mr, A=3, S=2, strength=4.0, joint=False, curve=None):
    luma, chroma = tables(bd, S, strength, joint, curve is not None)
    return MR.denoise_clip(frames, *sub(ss), D, A, S, luma, chroma, mr, joint, curve)


def vectors_reference(cur, ref, mr, joint=False, curve=None):
    planes = [[np.asarray(p) for p in cur], [np.asarray(p) for p in ref]]
    if curve is not None:
        fwd = np.asarray(curve[0]).astype(np.int64)
        planes = [[fwd[f[0]]] + f[1:] for f in planes]
    out = [MR.search(planes[0][0], planes[1][0], mr)]
    if len(cur) == 3 and joint:
        out += [MR.search(planes[0][1:3], planes[1][1:3], mr)] * 2
    elif len(cur) == 3:
        out += [MR.search(planes[0][c], planes[1][c], mr) for c in (1, 2)]
    return out


def check(frames, bd, ss, D, mr, what, batch=0, **kw):
    """the vectors of frame 0 towards frame 1 (when there are two) and every output plane of the clip"""
    from grav1synth_amd.denoise import Denoiser

    names = dict(A="search_radius", S="patch_radius", strength="strength", joint="joint_chroma", curve="curve")
    dn = Denoiser(bd, temporal_radius=D, motion_range=mr, batch_frames=batch, **{names[k]: v for k, v in kw.items()})
    try:
        dev = [_to_dev(f, bd) for f in frames]
        if len(frames) > 1:
            got = dn.motion_vectors(dev[0], dev[1], *sub(ss))
            want = vectors_reference(frames[0], frames[1], mr, kw.get("joint", False), kw.get("curve"))
            for c, (a, b) in enumerate(zip(got, want)):
                assert a.dtype == np.int16 and np.array_equal(a, b), f"{what}: vectors of plane {c}: {a.tolist()} vs {b.tolist()}"
            host = dn.motion_vectors(frames[0], frames[1], *sub(ss))
            assert all(np.array_equal(a, b) for a, b in zip(host, got)), f"{what}: host frames give other vectors"
        assert_clips_equal(dn.denoise_clip(dev, *sub(ss)), reference(frames, bd, ss, D, mr, **kw), what)
        for d, f in zip(dev, frames):
            assert_planes_equal(d, f, f"{what}: input after the call")
    finally:
        dn.close()


# ---------------------------------------------------------------------------------------------------- planes and formats
@pytest.mark.parametrize("ss,bd", [(ss, bd) for ss in ("420", "422", "444", "mono") for bd in (8, 10, 12)])
def test_every_format_and_depth(ss, bd):
    """129 x 97: three blocks with ragged ones; the 4:2:0 chroma is 65 x 49, and every odd size makes a search plane clamp"""
    frames = panned(3, 129, 97, bd, ss, seed=1)
    check(frames, bd, ss, 1, 32, f"{ss} {bd} bit")
    luma, _ = tables(bd, 2, 4.0)
    from tests import denoise_temporal_ref as TR

    still = TR.denoise_plane_clip([f[0] for f in frames], 1, 3, 2, *luma)
    assert any((a != b[0]).any() for a, b in zip(still, reference([f[:1] for f in frames], bd, "mono", 1, 32))), "the vectors did something"


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (63, 47), (64, 48), (65, 49), (129, 97)])
def test_plane_sizes(w, h):
    for bd, ss in ((8, "420"), (12, "444"), (10, "mono")):
        check(panned(3, w, h, bd, ss, seed=2), bd, ss, 1, 32, f"{w}x{h} {ss} {bd} bit")


# ------------------------------------------------------------------------------------------------------------- the range
@pytest.mark.parametrize("mr", [2, 32, 64])
def test_pans_at_the_range_beyond_it_and_odd(mr):
    """frame t to t + 1: a pan equal to the range, one step beyond it (what the key picks then is still the reference's), an
    odd one (found to within a sample: rule 6's own search takes the rest)"""
    odd = min(mr, 7) | 1 if mr > 2 else 1
    shifts = [(mr, 0), (-(mr + 2), 2), (odd, -odd), (0, mr)]
    frames = panned(5, 129, 97, 8, "mono", shifts, seed=3 + mr)
    check(frames, 8, "mono", 1, mr, f"Mr {mr}")
    from grav1synth_amd.denoise import Denoiser

    dn = Denoiser(8, temporal_radius=1, motion_range=mr)
    mv = dn.motion_vectors(frames[0], frames[1], 1, 1)[0]
    dn.close()
    if mr > 2:
        assert (mv[1, 1] == (-mr, 0)).all(), (mr, mv.tolist())  # the interior block finds the pan at the very edge of the range


# ------------------------------------------------------------------------------------------------------------ clip shapes
@pytest.mark.parametrize("D", [1, 2, 3])
def test_clip_lengths_and_batches(D):
    """clips of 1, D + 1 and 2 D + 1 frames, and of batch + 1 frames at batch 2 and 3: vectors and neighbours cross a batch"""
    for n, batch in ((1, 2), (D + 1, 2), (2 * D + 1, 3), (3, 2), (4, 3)):
        frames = panned(n, 65, 49, 10, "mono", seed=10 + n)
        check(frames, 10, "mono", D, 16, f"D {D}, {n} frames, batch {batch}", batch=batch)


@pytest.mark.parametrize("event", ["drain", "sync", "geometry"])
def test_clip_events_in_mid_clip(event):
    from grav1synth_amd.denoise import Denoiser

    bd, ss, D, mr = 8, "420", 1, 32
    frames = panned(5, 70, 50, bd, ss, seed=20)
    other = panned(1, 73, 51, bd, "444", seed=21)[0]
    dn = Denoiser(bd, temporal_radius=D, motion_range=mr, batch_frames=2)
    dev = [_to_dev(f, bd) for f in frames]
    got = [dn.apply(f, *sub(ss), sync=False) for f in dev[:3]]
    if event == "drain":
        assert dn.drain() == 2
        want = reference(frames, bd, ss, D, mr)
    elif event == "sync":
        dn.sync()
        want = reference(frames[:3], bd, ss, D, mr) + reference(frames[3:], bd, ss, D, mr)
    else:
        got_other = dn.apply(_to_dev(other, bd), 0, 0, sync=False)
        want = reference(frames[:3], bd, ss, D, mr) + reference(frames[3:], bd, ss, D, mr)
    got += [dn.apply(f, *sub(ss), sync=False) for f in dev[3:]]
    dn.sync()
    dn.close()
    assert_clips_equal(got, want, event)
    if event == "geometry":
        assert_planes_equal(got_other, reference([other], bd, "444", D, mr)[0], "the frame of the other geometry")


def test_host_pinned_and_device_frames_in_one_clip():
    import torch

    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.diff import Frame

    bd, ss, D, mr = 10, "420", 1, 32
    frames = panned(7, 99, 53, bd, ss, seed=30)
    L = _lib.lib()
    dn = Denoiser(bd, temporal_radius=D, motion_range=mr, batch_frames=3)
    keep, outs = [], []
    for t, planes in enumerate(frames):
        kind = ("host", "pinned", "device")[t % 3]
        if kind == "host":
            outs.append(dn.apply([p.copy() for p in planes], *sub(ss), sync=False))
        elif kind == "pinned":
            pin_in = [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
            pin_out = [torch.from_numpy(np.zeros(p.shape, p.dtype)).pin_memory() for p in planes]
            fin = Frame(pin_in, *sub(ss), async_host=True).to_c(keep)
            fout = Frame(pin_out, *sub(ss), async_host=True).to_c(keep)
            assert fin.on_device == 2 and fout.on_device == 2
            keep += [pin_in, pin_out]
            assert L.g1s_denoise_frame(dn._h, C.byref(fin), C.byref(fout)) == 0
            dn._frames += 1
            outs.append([p.numpy() for p in pin_out])
        else:
            outs.append(dn.apply(_to_dev(planes, bd), *sub(ss), sync=False))
    dn.sync()
    dn.close()
    assert_clips_equal(outs, reference(frames, bd, ss, D, mr), "host, pinned and device frames")


# ------------------------------------------------------------------------------------------------------ parameters, content
@pytest.mark.parametrize("A,S", [(1, 1), (7, 4)])
def test_search_and_patch_radius_corners(A, S):
    frames = panned(3, 65, 49, 8, "420", seed=40 + A)
    check(frames, 8, "420", 1, 32, f"A {A} S {S}", A=A, S=S, strength=6.0)


def test_full_range_noise_and_a_sad_at_its_ceiling():
    rng = np.random.default_rng(50)
    noise = [[rng.integers(0, 4096, (ph, pw)).astype(np.uint16) for pw, ph in shapes(129, 97, "444")] for _ in range(3)]
    check(noise, 12, "444", 1, 64, "12-bit noise", strength=300.0)
    check(noise, 12, "444", 1, 64, "12-bit noise, joint", strength=300.0, joint=True)
    # every sample of every candidate differs by 4095: SAD = 768 x 4095 a plane in a whole block, and the zero vector
    ends = [[np.full((ph, pw), v, np.uint16) for pw, ph in shapes(129, 97, "444")] for v in (0, 4095, 0)]
    check(ends, 12, "444", 1, 64, "0 against 4095")
    check(ends, 12, "444", 1, 64, "0 against 4095, joint", joint=True)


@pytest.mark.parametrize("period", [0, 4])
def test_content_where_many_candidates_tie(period):
    from grav1synth_amd.denoise import Denoiser

    planes = [MC.ties(pw, ph, 10, 3, period) for pw, ph in shapes(129, 97, "420")]
    frames = MC.clip(planes)
    check(frames, 10, "420", 1, 32, f"period {period}")
    dn = Denoiser(10, temporal_radius=1, motion_range=32)
    assert not any(v.any() for v in dn.motion_vectors(frames[0], frames[1], 1, 1)), "the zero vector wins among equals"
    dn.close()


# ------------------------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize("joint,prior", [(True, False), (False, True), (True, True)])
def test_joint_chroma_and_a_grain_prior_with_motion(joint, prior):
    from tests.test_gpu_denoise_curve import curve

    bd, ss = 10, "420"
    frames = panned(3, 129, 97, bd, ss, seed=60)
    kw = dict(joint=True) if joint else {}
    if prior:
        kw["curve"] = curve("example", bd)
    check(frames, bd, ss, 1, 32, f"joint {joint} prior {prior}", batch=2, **kw)


@pytest.mark.parametrize("prior", [False, True])
def test_motion_range_zero_is_the_denoiser_without_it(prior):
    """g1s_denoise_new_motion(..., 0) against g1s_denoise_new_curve / g1s_denoise_new_ex: the same bytes"""
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise_curve import curve

    bd, ss = 10, "420"
    frames = panned(4, 129, 97, bd, ss, seed=70)
    dev = [_to_dev(f, bd) for f in frames]
    cv = curve("example", bd) if prior else None
    old = Denoiser(bd, temporal_radius=1, joint_chroma=True, curve=cv, batch_frames=2)
    want = old.denoise_clip(dev, *sub(ss))
    new = Denoiser(bd, temporal_radius=1, joint_chroma=True, curve=cv, batch_frames=2)
    L = _lib.lib()
    L.g1s_denoise_free(new._h)
    from grav1synth_amd.denoise import denoise_opts

    opts = denoise_opts(batch_frames=2)
    fwd, inv = (cv[0].ctypes.data, cv[1].ctypes.data) if prior else (None, None)
    new._h = L.g1s_denoise_new_motion(bd, C.byref(opts), 1, _lib.G1S_DENOISE_JOINT_CHROMA, fwd, inv, 0)
    assert new._h, L.g1s_last_global_error()
    got = new.denoise_clip(dev, *sub(ss))
    assert_clips_equal(got, [[p.cpu().numpy() for p in f] for f in want], "motion_range 0")
    with pytest.raises(_lib.G1SError) as e:
        new.motion_vectors(dev[0], dev[1], *sub(ss))
    assert "needs a denoiser with a motion range" in str(e.value)
    old.close()
    new.close()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_the_refusals(tmp_path):
    from grav1synth_amd.denoise import Denoiser, denoise_opts, denoise_y4m_file
    from grav1synth_amd.ingest import write_y4m

    L = _lib.lib()
    opts = denoise_opts()
    for mr, D, text in ((3, 1, "motion_range must be even and 0..64"), (66, 1, "motion_range must be even and 0..64"),
                        (2, 0, "motion_range needs a temporal radius")):
        assert not L.g1s_denoise_new_motion(8, C.byref(opts), D, 0, None, None, mr)
        assert L.g1s_last_global_error().decode() == text
        with pytest.raises(_lib.G1SError) as e:
            Denoiser(8, temporal_radius=D, motion_range=mr)
        assert text in str(e.value)
    frames = panned(2, 64, 48, 8, "420", seed=80)
    src = tmp_path / "s.y4m"
    write_y4m(str(src), frames, 8, 1, 1, Fraction(24, 1))
    err = C.create_string_buffer(256)
    rc = L.g1s_denoise_y4m_file_motion(str(src).encode(), str(tmp_path / "o.y4m").encode(), C.byref(opts), 1, 0, None, 0, -1, 5, err, len(err))
    assert rc == -1  # G1S_ERR_INVALID
    assert err.value.decode() == "motion_range must be even and 0..64"
    with pytest.raises(_lib.G1SError) as e:
        denoise_y4m_file(str(src), str(tmp_path / "o.y4m"), motion_range=4)
    assert "motion_range needs a temporal radius" in str(e.value)
    frames_out = C.c_uint64()
    rc = L.g1s_diff_y4m_file_denoised_motion(str(src).encode(), str(tmp_path / "o.tbl").encode(), None, None, C.byref(opts), 0, 0, None, 0, -1, 2,
                                             C.byref(frames_out), err, len(err))
    assert rc == -1 and err.value.decode() == "motion_range needs a temporal radius"
    # the capacity of the vector arrays
    dn = Denoiser(8, temporal_radius=1, motion_range=2)
    keep: list = []
    from grav1synth_amd.diff import Frame

    fa, fb = Frame(frames[0], 1, 1).to_c(keep), Frame(frames[1], 1, 1).to_c(keep)
    big = panned(2, 129, 97, 8, "420", seed=81)
    ga, gb = Frame(big[0], 1, 1).to_c(keep), Frame(big[1], 1, 1).to_c(keep)
    mv = [np.zeros((1, 2), np.int16) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[m.ctypes.data for m in mv])
    caps = (C.c_size_t * 3)(1, 1, 1)
    assert L.g1s_denoise_motion_search(dn._h, C.byref(fa), C.byref(fb), ptrs, caps) == 0 and list(caps) == [1, 1, 1]
    assert L.g1s_denoise_motion_search(dn._h, C.byref(ga), C.byref(gb), ptrs, caps) == _lib.G1S_ERR_CAPACITY and list(caps) == [9, 4, 4]
    dn.close()


# --------------------------------------------------------------------------------------------------------------- commands
def test_the_commands_with_a_motion_range(tmp_path):
    """`denoise --motion-range` and `diff --denoise --keep-denoised --motion-range` against the Python path, byte for byte"""
    from grav1synth_amd.denoise import Denoiser

    src, frames = _clip(tmp_path)
    n = len(frames)
    dn = Denoiser(8, temporal_radius=1, motion_range=16, strength=5.0)
    want = [[p.cpu().numpy() for p in f] for f in dn.denoise_clip([_to_dev(f, 8) for f in frames], 1, 1)]
    dn.close()
    den, kept, a_tbl, b_tbl = tmp_path / "den.y4m", tmp_path / "kept.y4m", tmp_path / "a.tbl", tmp_path / "b.tbl"
    p = _run("denoise", str(src), "-o", str(den), "--temporal-radius", "1", "--motion-range", "16", "--strength", "5")
    assert p.returncode == 0 and f"Denoised {n} frames" in p.stderr, p.stderr[-2000:]
    assert_clips_equal(_y4m_frames(den, n), want, "denoise --motion-range 16")
    p = _run("diff", str(src), "--denoise", "--temporal-radius", "1", "--motion-range", "16", "--strength", "5", "-o", str(a_tbl), "--keep-denoised", str(kept))
    assert p.returncode == 0 and f"Computed diff for {n} frames" in p.stderr, p.stderr[-2000:]
    assert kept.read_bytes() == den.read_bytes()
    p = _run("diff", str(src), str(kept), "-o", str(b_tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    assert a_tbl.read_bytes() == b_tbl.read_bytes()
