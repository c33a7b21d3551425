"""The temporal radius of `denoise` on the device against tests/denoise_temporal_ref.py, byte for byte: clips, clip ends,
batches and drains, frames of every kind of memory, the commands."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import content as CT
from tests import denoise_temporal_ref as TR
from tests import views as V
from tests.test_gpu_denoise import _clip, _run, gradient
from tests.test_gpu_denoise import reference as spatial_reference
from tests.test_gpu_grain import SUBSAMPLINGS, _to_dev, assert_planes_equal, make_segment

pytestmark = pytest.mark.gpu


def reference(frames, bd, D, A=3, S=2, strength=4.0, chroma_strength=None):
    from grav1synth_amd.denoise import weight_table

    luma = weight_table(bd, S, strength)
    chroma = weight_table(bd, S, strength if chroma_strength is None else chroma_strength)
    return TR.denoise_clip([[np.asarray(p) for p in f] for f in frames], D, A, S, luma, chroma)


def assert_clips_equal(got, want, what):
    assert len(got) == len(want)
    for t, (a, b) in enumerate(zip(got, want)):
        assert_planes_equal(a, b, f"{what} frame {t}")


def moving_clip(n, w, h, bd, subx, suby, mono=False, seed=0, grain=True):
    """n frames: a window that moves over a larger picture, faster from frame to frame (so the clip played backwards is
    another clip and frame t - 1 is not frame t + 1), with grain rendered on every frame from its own seed."""
    from grav1synth_amd.grain import GrainSynthesizer

    _src, big = CT.make_frames("distinct", w + 64, h + 64, bd, subx, suby, frame=seed)  # (the window moves by less than 30 samples)
    syn = GrainSynthesizer(bd) if grain else None
    frames = []
    for t in range(n):
        ox, oy = (3 * t) % 30, ((t * t) // 2) % 30
        planes = [np.ascontiguousarray(big[0][oy:oy + h, ox:ox + w])]
        ch, cw = (h + suby) >> suby, (w + subx) >> subx
        planes += [np.ascontiguousarray(p[oy:oy + ch, ox:ox + cw]) for p in big[1:]]
        if grain:
            planes = [np.asarray(p) for p in syn.apply(planes, make_segment(3, 40 + bd + 7 * t), subx, suby)]
        frames.append(planes[:1] if mono else planes)
    if syn:
        syn.close()
    return frames


def gradient_clip(n, w, h, bd, subx, suby, seed=0, amp=5, mono=False):
    return [gradient(w, h, bd, subx, suby, seed=seed * 100 + t, mono=mono, amp=amp) for t in range(n)]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
def test_grainy_moving_clips_equal_the_reference(bd, ss):
    from grav1synth_amd.denoise import Denoiser

    mono = ss == "mono"
    subx, suby = (1, 1) if mono else SUBSAMPLINGS[ss]
    frames = moving_clip(7, 136, 104, bd, subx, suby, mono=mono, seed=1)
    dev = [_to_dev(f, bd) for f in frames]
    for D in (1, 2, 3):
        dn = Denoiser(bd, temporal_radius=D)
        got = dn.denoise_clip(dev, subx, suby)
        dn.close()
        want = reference(frames, bd, D)
        assert_clips_equal(got, want, f"{bd} bit {ss} D {D}")
        if D == 1:
            spatial = [spatial_reference(f, bd) for f in frames]
            assert all(any((a != b).any() for a, b in zip(w, s)) for w, s in zip(want, spatial)), "the neighbours did something"


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (3, 7), (64, 48), (65, 49), (131, 97), (2, 210), (300, 2)])
def test_sizes_off_the_tile_and_smaller_than_the_window(size):
    from grav1synth_amd.denoise import Denoiser

    w, h = size
    for bd, ss in ((8, "420"), (10, "422"), (12, "444")):
        subx, suby = SUBSAMPLINGS[ss]
        frames = gradient_clip(5, w, h, bd, subx, suby, seed=1)
        dn = Denoiser(bd, temporal_radius=2)
        got = dn.denoise_clip([_to_dev(f, bd) for f in frames], subx, suby)
        dn.close()
        assert_clips_equal(got, reference(frames, bd, 2), f"{w}x{h} {bd} bit {ss}")


def test_clips_shorter_than_the_window():
    from grav1synth_amd.denoise import Denoiser

    bd, (subx, suby) = 10, (1, 1)
    frames = gradient_clip(2, 150, 101, bd, subx, suby, seed=2)
    dn = Denoiser(bd, temporal_radius=3)
    one = dn.denoise_clip([_to_dev(frames[0], bd)], subx, suby)
    assert_planes_equal(one[0], spatial_reference(frames[0], bd), "a one-frame clip is the spatial filter")
    assert_planes_equal(dn.apply(_to_dev(frames[1], bd), subx, suby), spatial_reference(frames[1], bd), "apply(sync=True) is a one-frame clip")
    two = dn.denoise_clip([_to_dev(f, bd) for f in frames], subx, suby)
    dn.close()
    assert_clips_equal(two, reference(frames, bd, 3), "two frames at D = 3")


@pytest.mark.parametrize("A,S", [(1, 1), (1, 4), (7, 1), (7, 4), (7, 3), (4, 3), (2, 2)])
def test_parameter_corners(A, S):
    from grav1synth_amd.denoise import Denoiser

    bd, (subx, suby) = 10, (1, 1)
    frames = gradient_clip(3, 150, 101, bd, subx, suby, seed=A * 10 + S, amp=6)
    dev = [_to_dev(f, bd) for f in frames]
    for strength, chroma in ((0.05, 0.05), (6.0, 2.5), (300.0, 40.0)):
        dn = Denoiser(bd, search_radius=A, patch_radius=S, strength=strength, chroma_strength=chroma, temporal_radius=1)
        got = dn.denoise_clip(dev, subx, suby)
        dn.close()
        assert_clips_equal(got, reference(frames, bd, 1, A, S, strength, chroma), f"A {A} S {S} h {strength}")


def test_the_64_bit_numerator():
    from grav1synth_amd.denoise import Denoiser, weight_table

    kw = dict(search_radius=7, patch_radius=1, strength=1000.0)
    full = [[np.full((90, 100), 4095, np.uint16)] for _ in range(7)]
    rng = np.random.default_rng(3)
    wild = [[rng.integers(0, 4096, (90, 100)).astype(np.uint16)] for _ in range(7)]
    for f in wild:
        f[0][20:70, 10:90] = 4095 - (f[0][20:70, 10:90] & 3)
    num, _den = TR.sums_plane([f[0] for f in wild], 3, 3, 7, 1, *weight_table(12, 1, 1000.0))
    assert num.max() >= 2 ** 32
    dn = Denoiser(12, temporal_radius=3, **kw)
    got = dn.denoise_clip([_to_dev(f, 12) for f in full])
    assert_clips_equal(got, full, "all maximum")
    got = dn.denoise_clip([_to_dev(f, 12) for f in wild])
    dn.close()
    assert_clips_equal(got, reference(wild, 12, 3, 7, 1, 1000.0), "full range, A 7, D 3, 12 bit")


def test_70_frames_in_batches_of_32_with_and_without_drains():
    from grav1synth_amd.denoise import Denoiser

    bd, (subx, suby), D = 8, (1, 1), 2
    frames = gradient_clip(70, 130, 70, bd, subx, suby, seed=3)
    dev = [_to_dev(f, bd) for f in frames]
    want = reference(frames, bd, D)
    drained = Denoiser(bd, batch_frames=32, temporal_radius=D)
    outs = []
    assert drained.drain() == 0
    for k, f in enumerate(dev):
        outs.append(drained.apply(f, subx, suby, sync=False))
        if k in (0, 1, 2, 9, 10, 31, 33, 40, 63, 64, 68):
            done = drained.drain()
            assert done == max(k + 1 - D, 0), (k, done)
            if done:
                assert_planes_equal(outs[done - 1], want[done - 1], f"frame {done - 1} after the drain at {k}")
    assert drained.drain() == 70 - D and drained.drain() == 70 - D
    drained.sync()
    assert drained.drain() == 70
    assert_clips_equal(outs, want, "with drains")
    drained.close()
    plain = Denoiser(bd, batch_frames=32, temporal_radius=D)
    assert_clips_equal(plain.denoise_clip(dev, subx, suby), want, "without a drain")
    plain.close()


def test_sync_and_a_geometry_change_end_a_clip():
    from grav1synth_amd.denoise import Denoiser

    bd, (subx, suby), D = 10, (1, 1), 2
    frames = gradient_clip(10, 100, 60, bd, subx, suby, seed=4)
    dev = [_to_dev(f, bd) for f in frames]
    dn = Denoiser(bd, temporal_radius=D)
    got = dn.denoise_clip(dev[:5], subx, suby) + dn.denoise_clip(dev[5:], subx, suby)
    want = reference(frames[:5], bd, D) + reference(frames[5:], bd, D)
    assert_clips_equal(got, want, "two clips of five")
    assert any((a != b).any() for a, b in zip(reference(frames, bd, D)[4], want[4])), "one clip of ten is something else"
    # five frames, then another geometry (host frames), then the first geometry again: three clips
    small = gradient_clip(3, 70, 50, bd, 0, 0, seed=5)
    outs = [dn.apply(f, subx, suby, sync=False) for f in dev[:5]]
    outs_small = [dn.apply(f, 0, 0, sync=False) for f in small]
    assert dn.drain() == 5 + 10 + 1, "the first clip is complete, and the first frame of the second"
    outs_again = [dn.apply(f, subx, suby, sync=False) for f in dev[5:]]
    dn.sync()
    assert_clips_equal(outs, want[:5], "before the geometry change")
    assert_clips_equal(outs_small, reference(small, bd, D), "the other geometry")
    assert_clips_equal(outs_again, want[5:], "after it")
    dn.close()


def test_one_clip_of_host_pinned_device_and_strided_frames():
    import torch

    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.diff import Frame

    bd, (subx, suby), D = 10, (1, 1), 2
    frames = moving_clip(9, 163, 99, bd, subx, suby, seed=2)
    want = reference(frames, bd, D)
    dn = Denoiser(bd, batch_frames=4, temporal_radius=D)
    L = _lib.lib()
    outs, guards_in, guards_out, keep = [], [], [], []
    for t, planes in enumerate(frames):
        kind = ("host", "pinned", "device", "view")[t % 4]
        if kind == "host":
            outs.append(dn.apply(planes, subx, suby, sync=False))
        elif kind == "pinned":
            pin_in = [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
            pin_out = [torch.from_numpy(np.zeros(p.shape, p.dtype)).pin_memory() for p in planes]
            fin = Frame(pin_in, subx, suby, async_host=True).to_c(keep)
            fout = Frame(pin_out, subx, suby, async_host=True).to_c(keep)
            assert fin.on_device == 2 and fout.on_device == 2
            keep += [pin_in, pin_out]
            assert L.g1s_denoise_frame(dn._h, C.byref(fin), C.byref(fout)) == 0
            dn._frames += 1
            outs.append([p.numpy() for p in pin_out])
        elif kind == "device":
            outs.append(dn.apply(_to_dev(planes, bd), subx, suby, sync=False))
        else:
            vin = [V.device_view(p, pitch_bytes=p.shape[1] * 2 + 26 + 2 * c, base_offset_bytes=6 + 2 * c, max_code=1023, seed=t) for c, p in enumerate(planes)]
            vout = [V.device_view(np.zeros_like(p), pitch_bytes=p.shape[1] * 2 + 18, base_offset_bytes=10, fill="max", max_code=1023, seed=t) for p in planes]
            guards_in += [g for _v, g in vin]
            guards_out += [g for _v, g in vout]
            outs.append(dn.apply([v for v, _g in vin], subx, suby, sync=False, out=[v for v, _g in vout]))
        if t == 5:
            assert dn.drain() == 6 - D
    dn.sync()
    assert_clips_equal(outs, want, "mixed memory")
    for g in guards_in:
        g.assert_unchanged("a strided input")
    for g in guards_out:
        g.assert_margin_intact("a strided output")
    dn.close()
    # overlap is still refused: the frame's own planes, and a plane that a queued frame still reads
    own = Denoiser(bd, temporal_radius=1)
    a, b = _to_dev(frames[0], bd), _to_dev(frames[1], bd)
    with pytest.raises(_lib.G1SError) as e:
        own.apply(a, subx, suby, out=a)
    assert "distinct" in str(e.value)
    own.close()
    own = Denoiser(bd, temporal_radius=1)
    own.apply(a, subx, suby, sync=False)
    with pytest.raises(_lib.G1SError) as e:
        own.apply(b, subx, suby, sync=False, out=a)
    assert "distinct" in str(e.value)
    own.close()


def test_radius_0_through_the_new_entry_points_is_the_old_filter(tmp_path):
    from grav1synth_amd.denoise import Denoiser, denoise_opts, denoise_y4m_file
    from grav1synth_amd.ingest import write_y4m

    bd, (subx, suby) = 8, (1, 1)
    frames = gradient_clip(9, 150, 101, bd, subx, suby, seed=6)
    dev = [_to_dev(f, bd) for f in frames]
    L = _lib.lib()
    old = Denoiser.__new__(Denoiser)  # a denoiser made by g1s_denoise_new itself
    old._L, old.bit_depth, old.temporal_radius, old._keep, old._frames = L, bd, 0, [], 0
    old._h = L.g1s_denoise_new(bd, C.byref(denoise_opts(batch_frames=4)))
    assert old._h
    new = Denoiser(bd, batch_frames=4, temporal_radius=0)
    a = old.denoise_clip(dev, subx, suby)
    b = [new.apply(f, subx, suby, sync=False) for f in dev]
    assert new.drain() == 9  # with radius 0 a drain completes what a sync completes
    assert_clips_equal(b, [[p.cpu().numpy() for p in f] for f in a], "g1s_denoise_new_temporal(0) against g1s_denoise_new")
    assert_clips_equal(a, [spatial_reference(f, bd) for f in frames], "and the spatial reference")
    old.close(), new.close()
    src, o1, o2 = tmp_path / "s.y4m", tmp_path / "a.y4m", tmp_path / "b.y4m"
    write_y4m(str(src), frames, bd, subx, suby, Fraction(24, 1))
    err = C.create_string_buffer(256)
    opts = denoise_opts(batch_frames=4)
    assert L.g1s_denoise_y4m_file(str(src).encode(), str(o1).encode(), C.byref(opts), err, len(err)) == 9, err.value
    assert denoise_y4m_file(str(src), str(o2), batch_frames=4, temporal_radius=0) == 9
    assert o1.read_bytes() == o2.read_bytes()


def _y4m_frames(path, n):
    from grav1synth_amd.ingest import Y4MReader

    rd = Y4MReader(str(path))
    got = [[np.asarray(p).copy() for p in rd.get_frame()] for _ in range(n)]
    assert rd.get_frame() is None
    rd.close()
    return got


def test_the_commands_end_to_end(tmp_path):
    from grav1synth_amd.ingest import diff_y4m_file_denoised, write_y4m

    bd, (subx, suby) = 8, (1, 1)
    frames = moving_clip(70, 96, 64, bd, subx, suby, seed=3)
    src = tmp_path / "moving.y4m"
    write_y4m(str(src), frames, bd, subx, suby, Fraction(24, 1))
    # `denoise --temporal-radius 2`: more frames than two batches of 32, one clip
    out = tmp_path / "den.y4m"
    p = _run("denoise", str(src), "-o", str(out), "--temporal-radius", "2", "--strength", "5")
    assert p.returncode == 0, p.stderr[-2000:]
    assert "Denoised 70 frames" in p.stderr
    assert_clips_equal(_y4m_frames(out, 70), reference(frames, bd, 2, strength=5.0), "denoise --temporal-radius 2")
    # `diff --denoise --temporal-radius 1 --keep-denoised K` on a source the estimator finds flat blocks in, with a scene cut: K is
    # what `denoise` writes, the table what `diff SOURCE K` writes
    src, frames = _clip(tmp_path)
    n = len(frames)
    den1, kept, a_tbl, b_tbl = tmp_path / "den1.y4m", tmp_path / "kept.y4m", tmp_path / "a.tbl", tmp_path / "b.tbl"
    p = _run("denoise", str(src), "-o", str(den1), "--temporal-radius", "1", "--strength", "5")
    assert p.returncode == 0, p.stderr[-2000:]
    got = _y4m_frames(den1, n)
    for lo, hi in ((0, 3), (n // 2 - 2, n // 2 + 2), (n - 3, n)):  # frames lo + 1 .. hi - 2 of the clip from their neighbours alone
        want = reference(frames[lo:hi], bd, 1, strength=5.0)
        for t in range(lo + (lo > 0), hi - (hi < n)):
            assert_planes_equal(got[t], want[t - lo], f"denoise --temporal-radius 1 frame {t}")
    p = _run("diff", str(src), "--denoise", "--temporal-radius", "1", "--strength", "5", "-o", str(a_tbl), "--keep-denoised", str(kept))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Computed diff for {n} frames" in p.stderr
    assert kept.read_bytes() == den1.read_bytes()
    p = _run("diff", str(src), str(kept), "-o", str(b_tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    assert a_tbl.read_bytes() == b_tbl.read_bytes()
    # small groups on both sides: the pairs of buffers are used again while their sources are still neighbours
    c_tbl, kept2 = tmp_path / "c.tbl", tmp_path / "kept2.y4m"
    assert diff_y4m_file_denoised(str(src), str(c_tbl), keep_denoised=str(kept2), batch_frames=2, denoise_batch_frames=3, strength=5.0,
                                  temporal_radius=1) == n
    assert kept2.read_bytes() == den1.read_bytes() and c_tbl.read_bytes() == b_tbl.read_bytes()
    p = _run("denoise", str(src), "-o", str(tmp_path / "never.y4m"), "--temporal-radius", "4")
    assert p.returncode == 0 and "--temporal-radius must be 0..3" in p.stderr and not (tmp_path / "never.y4m").exists()


def test_4k_10_bit_clip():
    from grav1synth_amd.denoise import Denoiser, weight_table
    from grav1synth_amd.grain import GrainSynthesizer

    bd, (subx, suby), D, A, S = 10, (1, 1), 1, 3, 2
    syn = GrainSynthesizer(bd)
    frames = []
    for t in range(3):
        _src, den = CT.make_frames("busy", 3840, 2160, bd, subx, suby, frame=t)
        frames.append([np.asarray(p) for p in syn.apply(den, make_segment(3, 77 + t), subx, suby)])
    syn.close()
    dn = Denoiser(bd, temporal_radius=D)
    got = [[p.cpu().numpy() for p in f] for f in dn.denoise_clip([_to_dev(f, bd) for f in frames], subx, suby)]
    dn.close()
    # bands of rows: the reference of rows a - R .. b + R of every frame is the reference of the plane on the rows a .. b
    R = A + S
    tables = [weight_table(bd, S, 4.0)] * 3
    for c in range(3):
        h = frames[0][c].shape[0]
        for a, b in ((0, 40), (h // 2 - 7, h // 2 + 33), (h - 40, h)):
            lo, hi = max(a - R, 0), min(b + R, h)
            want = TR.denoise_plane_clip([f[c][lo:hi] for f in frames], D, A, S, *tables[c])
            for t in range(3):
                assert np.array_equal(got[t][c][a:b], want[t][a - lo:b - lo]), (c, a, t)
