"""Luma-guided joint chroma (`denoise`, rules 8 - 11t) on the device against tests/denoise_joint_ref.py, byte for byte:
formats, sizes around the 64 x 48 chroma tile, the 32-bit ceiling of the joint distance, clips, frames of every kind of
memory, the entry points and the commands."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import denoise_joint_ref as J
from tests import views as V
from tests.test_denoise_joint_cpu import ceiling_frame
from tests.test_gpu_denoise import _clip, _run, gradient
from tests.test_gpu_denoise import reference as independent_reference
from tests.test_gpu_denoise_temporal import _y4m_frames, assert_clips_equal, gradient_clip, moving_clip
from tests.test_gpu_grain import SUBSAMPLINGS, _to_dev, assert_planes_equal

pytestmark = pytest.mark.gpu


def reference(frames, bd, sub, D=0, A=3, S=2, strength=4.0, chroma_strength=None):
    """The clip under the flag: luma by rules 1 - 7, chroma by rules 8 - 11t, the tables from the library."""
    from grav1synth_amd.denoise import weight_table

    luma = weight_table(bd, S, strength)
    joint = weight_table(bd, S, strength if chroma_strength is None else chroma_strength, joint_chroma=True)
    return J.denoise_clip([[np.asarray(p) for p in f] for f in frames], sub[0], sub[1], D, A, S, luma, joint)


def joint_clip(frames, bd, sub, **kw):
    from grav1synth_amd.denoise import Denoiser

    dn = Denoiser(bd, joint_chroma=True, **kw)
    try:
        return dn.denoise_clip([_to_dev(f, bd) for f in frames], *sub)
    finally:
        dn.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444"])
def test_grainy_content_equals_the_reference(bd, ss):
    """Chroma 65 x 49: all four tiles; at 4:2:0 the luma is 129 x 97, so the guide's last column and row clamp."""
    from grav1synth_amd.denoise import Denoiser

    sub = SUBSAMPLINGS[ss]
    w, h = (65 << sub[0]) - sub[0], (49 << sub[1]) - sub[1]
    frame = moving_clip(1, w, h, bd, *sub, seed=2)[0]
    assert frame[1].shape == (49, 65) and frame[0].shape == (h, w)
    got = joint_clip([frame], bd, sub)[0]
    want = reference([frame], bd, sub)[0]
    assert_planes_equal(got, want, f"{bd} bit {ss}")
    ind = independent_reference(frame, bd)
    assert (want[1] != ind[1]).any() and (want[2] != ind[2]).any(), "the joint weight did something"
    plain = Denoiser(bd)
    luma = plain.apply(_to_dev(frame, bd), *sub)[0].cpu().numpy()
    plain.close()
    assert np.array_equal(got[0].cpu().numpy(), luma), "luma is the unflagged denoiser's, to the byte"


@pytest.mark.parametrize("csize", [(63, 47), (64, 48), (128, 96), (3, 2)])
def test_chroma_sizes_around_the_tile_and_below_the_window(csize):
    cw, ch = csize
    for bd, ss, odd in ((8, "420", True), (10, "420", False), (10, "422", True), (12, "444", False)):
        sub = SUBSAMPLINGS[ss]
        w, h = (cw << sub[0]) - (sub[0] if odd else 0), (ch << sub[1]) - (sub[1] if odd else 0)
        frames = gradient_clip(2, w, h, bd, *sub, seed=1)
        assert frames[0][1].shape == (ch, cw)
        for D in (0, 1):
            assert_clips_equal(joint_clip(frames, bd, sub, temporal_radius=D), reference(frames, bd, sub, D), f"chroma {cw}x{ch} {bd} bit {ss} D {D}")


@pytest.mark.parametrize("A,S", [(1, 1), (7, 4), (7, 1), (1, 4)])
def test_parameter_corners(A, S):
    bd, sub = 10, (1, 1)
    frames = gradient_clip(2, 150, 101, bd, *sub, seed=A * 10 + S, amp=6)
    for strength, chroma, D in ((0.05, 0.05, 0), (6.0, 2.5, 1), (300.0, 40.0, 0)):
        got = joint_clip(frames, bd, sub, search_radius=A, patch_radius=S, strength=strength, chroma_strength=chroma, temporal_radius=D)
        assert_clips_equal(got, reference(frames, bd, sub, D, A, S, strength, chroma), f"A {A} S {S} h {strength}/{chroma} D {D}")


@pytest.mark.parametrize("strength", [1000.0, 4.0])
def test_the_32_bit_ceiling_of_the_joint_distance(strength):
    """12 bit, Cb, Cr and luma 0 / 4095 checkerboards (luma in 2 x 2 cells), S = 4: an odd offset gives D_J = 4 074 873 075,
    which no signed 32-bit sum holds."""
    A, S, sub = 3, 4, (1, 1)
    frame = ceiling_frame(150, 110, *sub)
    assert J.max_distance(frame, *sub, A, S) == 4074873075
    kw = dict(search_radius=A, patch_radius=S, strength=strength)
    assert_clips_equal(joint_clip([frame], 12, sub, **kw), reference([frame], 12, sub, 0, A, S, strength), f"h {strength}")
    # the temporal kernel: the neighbours are the checkerboard one sample on, so their offset 0 is at the ceiling
    other = [np.ascontiguousarray(4095 - p) for p in frame]
    clip3 = [other, frame, other]
    assert_clips_equal(joint_clip(clip3, 12, sub, temporal_radius=1, **kw), reference(clip3, 12, sub, 1, A, S, strength), f"h {strength} D 1")


@pytest.mark.parametrize("D", [1, 2])
def test_grainy_moving_clips_and_clips_shorter_than_the_window(D):
    bd, sub = 10, (1, 1)
    frames = moving_clip(5, 136, 104, bd, *sub, seed=1)
    want = reference(frames, bd, sub, D)
    assert_clips_equal(joint_clip(frames, bd, sub, temporal_radius=D), want, f"D {D}")
    spatial = reference(frames, bd, sub, 0)
    assert all((a[1] != b[1]).any() for a, b in zip(want, spatial)), "the neighbours did something"
    for n in (1, 2, 3):
        assert_clips_equal(joint_clip(frames[:n], bd, sub, temporal_radius=D), reference(frames[:n], bd, sub, D), f"{n} frames at D {D}")


def test_the_64_bit_numerators():
    A, S, h, sub = 7, 1, 1000.0, (0, 0)
    rng = np.random.default_rng(3)
    wild = [[rng.integers(0, 4096, (50, 100)).astype(np.uint16) for _ in range(3)] for _ in range(3)]
    for f in wild:
        for c in (1, 2):
            f[c][10:40, 10:90] = 4095 - (f[c][10:40, 10:90] & 3)
    from grav1synth_amd.denoise import weight_table

    nb, nr, _den = J.chroma_sums(wild, 1, 0, 0, 1, A, S, *weight_table(12, S, h, joint_chroma=True))
    assert nb.max() >= 2 ** 32 and nr.max() >= 2 ** 32
    got = joint_clip(wild, 12, sub, search_radius=A, patch_radius=S, strength=h, temporal_radius=1)
    assert_clips_equal(got, reference(wild, 12, sub, 1, A, S, h), "full range, A 7, D 1, 12 bit")


def test_9_frames_in_batches_of_4_with_and_without_drains():
    from grav1synth_amd.denoise import Denoiser

    bd, sub, D = 8, (1, 1), 2
    frames = gradient_clip(9, 130, 98, bd, *sub, seed=3)
    dev = [_to_dev(f, bd) for f in frames]
    want = reference(frames, bd, sub, D)
    drained = Denoiser(bd, batch_frames=4, temporal_radius=D, joint_chroma=True)
    outs = []
    for k, f in enumerate(dev):
        outs.append(drained.apply(f, *sub, sync=False))
        if k in (0, 2, 3, 6):
            done = drained.drain()
            assert done == max(k + 1 - D, 0), (k, done)
            if done:
                assert_planes_equal(outs[done - 1], want[done - 1], f"frame {done - 1} after the drain at {k}")
    drained.sync()
    assert drained.drain() == 9
    assert_clips_equal(outs, want, "with drains")
    drained.close()
    plain = Denoiser(bd, batch_frames=4, temporal_radius=D, joint_chroma=True)
    assert_clips_equal(plain.denoise_clip(dev, *sub), want, "without a drain")
    plain.close()


def test_sync_and_a_geometry_change_end_a_clip():
    from grav1synth_amd.denoise import Denoiser

    bd, sub, D = 10, (1, 1), 1
    frames = gradient_clip(6, 100, 60, bd, *sub, seed=4)
    dev = [_to_dev(f, bd) for f in frames]
    dn = Denoiser(bd, temporal_radius=D, joint_chroma=True)
    got = dn.denoise_clip(dev[:3], *sub) + dn.denoise_clip(dev[3:], *sub)
    want = reference(frames[:3], bd, sub, D) + reference(frames[3:], bd, sub, D)
    assert_clips_equal(got, want, "two clips of three")
    assert (reference(frames, bd, sub, D)[2][1] != want[2][1]).any(), "one clip of six is something else"
    # three frames, then another geometry (host frames, 4:4:4; then a luma-only one), then the first geometry again
    small = gradient_clip(2, 70, 50, bd, 0, 0, seed=5)
    mono = gradient_clip(1, 70, 50, bd, 0, 0, seed=6, mono=True)
    outs = [dn.apply(f, *sub, sync=False) for f in dev[:3]]
    outs_small = [dn.apply(f, 0, 0, sync=False) for f in small]
    out_mono = dn.apply(mono[0], 0, 0, sync=False)
    outs_again = [dn.apply(f, *sub, sync=False) for f in dev[3:]]
    dn.sync()
    assert_clips_equal(outs, want[:3], "before the geometry change")
    assert_clips_equal(outs_small, reference(small, bd, (0, 0), D), "the other geometry")
    assert_planes_equal(out_mono, independent_reference(mono[0], bd), "a luma-only frame under the flag")
    assert_clips_equal(outs_again, want[3:], "after it")
    dn.close()


def test_one_clip_of_host_pinned_device_and_strided_frames():
    import torch

    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.diff import Frame

    bd, sub, D = 10, (1, 1), 1
    frames = moving_clip(8, 163, 99, bd, *sub, seed=2)
    want = reference(frames, bd, sub, D)
    dn = Denoiser(bd, batch_frames=3, temporal_radius=D, joint_chroma=True)
    L = _lib.lib()
    outs, guards_in, guards_out, keep, dev_in = [], [], [], [], []
    for t, planes in enumerate(frames):
        kind = ("view", "host", "pinned", "device")[t % 4]
        if kind == "host":
            outs.append(dn.apply(planes, *sub, sync=False))
        elif kind == "pinned":
            pin_in = [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
            pin_out = [torch.from_numpy(np.zeros(p.shape, p.dtype)).pin_memory() for p in planes]
            fin = Frame(pin_in, *sub, async_host=True).to_c(keep)
            fout = Frame(pin_out, *sub, async_host=True).to_c(keep)
            assert fin.on_device == 2 and fout.on_device == 2
            keep += [pin_in, pin_out]
            assert L.g1s_denoise_frame(dn._h, C.byref(fin), C.byref(fout)) == 0
            dn._frames += 1
            outs.append([p.numpy() for p in pin_out])
        elif kind == "device":
            dev_in.append((_to_dev(planes, bd), planes))
            outs.append(dn.apply(dev_in[-1][0], *sub, sync=False))
        else:  # the luma the guide is read from has a pitch, an odd base and a hostile margin, as the chroma planes have
            vin = [V.device_view(p, pitch_bytes=p.shape[1] * 2 + 26 + 2 * c, base_offset_bytes=6 + 2 * c, max_code=1023, seed=t) for c, p in enumerate(planes)]
            vout = [V.device_view(np.zeros_like(p), pitch_bytes=p.shape[1] * 2 + 18, base_offset_bytes=10, fill="max", max_code=1023, seed=t) for p in planes]
            guards_in += [g for _v, g in vin]
            guards_out += [g for _v, g in vout]
            outs.append(dn.apply([v for v, _g in vin], *sub, sync=False, out=[v for v, _g in vout]))
        if t == 5:
            assert dn.drain() == 6 - D
    dn.sync()
    assert_clips_equal(outs, want, "mixed memory")
    for g in guards_in:
        g.assert_unchanged("a strided input")
    for g in guards_out:
        g.assert_margin_intact("a strided output")
    for dev, planes in dev_in:
        assert_planes_equal(dev, planes, "a device input after the call")
    dn.close()


def test_the_ex_entry_points_without_the_flag_and_a_luma_only_frame_under_it(tmp_path):
    from grav1synth_amd.denoise import Denoiser, denoise_opts, denoise_y4m_file
    from grav1synth_amd.ingest import write_y4m

    bd, sub = 8, (1, 1)
    frames = gradient_clip(5, 150, 101, bd, *sub, seed=6)
    dev = [_to_dev(f, bd) for f in frames]
    L = _lib.lib()
    for D in (0, 1):
        old = Denoiser.__new__(Denoiser)  # a denoiser made by g1s_denoise_new_temporal itself
        old._L, old.bit_depth, old.temporal_radius, old._keep, old._frames = L, bd, D, [], 0
        old._h = L.g1s_denoise_new_temporal(bd, C.byref(denoise_opts(batch_frames=2)), D)
        assert old._h
        new = Denoiser(bd, batch_frames=2, temporal_radius=D, joint_chroma=False)
        a, b = old.denoise_clip(dev, *sub), new.denoise_clip(dev, *sub)
        assert_clips_equal(b, [[p.cpu().numpy() for p in f] for f in a], f"g1s_denoise_new_ex(flags = 0) against g1s_denoise_new_temporal, D {D}")
        if D == 0:
            assert_clips_equal(a, [independent_reference(f, bd) for f in frames], "and the independent reference")
        # a luma-only clip under the flag: the same bytes as without it
        mono = [f[:1] for f in dev]
        flagged = Denoiser(bd, batch_frames=2, temporal_radius=D, joint_chroma=True)
        assert_clips_equal(flagged.denoise_clip(mono, *sub), [[f[0].cpu().numpy()] for f in a], f"luma only under the flag, D {D}")
        old.close(), new.close(), flagged.close()
    src, o1, o2, o3 = tmp_path / "s.y4m", tmp_path / "a.y4m", tmp_path / "b.y4m", tmp_path / "c.y4m"
    write_y4m(str(src), frames, bd, *sub, Fraction(24, 1))
    err = C.create_string_buffer(256)
    opts = denoise_opts(batch_frames=2)
    assert L.g1s_denoise_y4m_file_temporal(str(src).encode(), str(o1).encode(), C.byref(opts), 1, err, len(err)) == 5, err.value
    assert L.g1s_denoise_y4m_file_ex(str(src).encode(), str(o2).encode(), C.byref(opts), 1, 0, err, len(err)) == 5, err.value
    assert denoise_y4m_file(str(src), str(o3), batch_frames=2, temporal_radius=1, joint_chroma=False) == 5
    assert o1.read_bytes() == o2.read_bytes() == o3.read_bytes()
    assert L.g1s_denoise_y4m_file_ex(str(src).encode(), str(o2).encode(), C.byref(opts), 1, 2, err, len(err)) < 0 and b"unknown denoise flags" in err.value


def test_a_parameter_set_over_the_lds_limit_is_refused_and_the_largest_accepted_one_runs():
    """The largest accepted set (A = 7, S = 4, a temporal radius) asks for about 100 KB of LDS a workgroup: refused with its text
    where the device gives a workgroup less, and correct where it gives that much."""
    import torch

    from grav1synth_amd.denoise import Denoiser

    props = torch.cuda.get_device_properties(0)
    limit = getattr(props, "shared_memory_per_block_optin", 0) or getattr(props, "shared_memory_per_block", 0)
    bd, sub = 8, (1, 1)
    frames = gradient_clip(2, 70, 50, bd, *sub, seed=7)
    kw = dict(search_radius=7, patch_radius=4, temporal_radius=1)
    try:
        dn = Denoiser(bd, joint_chroma=True, **kw)
    except _lib.G1SError as e:
        assert "bytes of LDS" in str(e) and "joint chroma" in str(e) and limit < 101 * 1024, (str(e), limit)
        Denoiser(bd, **kw).close()  # the independent kernels of the same parameters fit everywhere
        return
    got = dn.denoise_clip([_to_dev(f, bd) for f in frames], *sub)
    dn.close()
    assert_clips_equal(got, reference(frames, bd, sub, 1, 7, 4), "A 7, S 4, D 1: the largest tile")


def test_the_commands_end_to_end(tmp_path):
    from grav1synth_amd.ingest import write_y4m

    bd, sub = 8, (1, 1)
    frames = moving_clip(6, 96, 64, bd, *sub, seed=3)
    src = tmp_path / "moving.y4m"
    write_y4m(str(src), frames, bd, *sub, Fraction(24, 1))
    for D in (0, 1):
        out = tmp_path / f"den{D}.y4m"
        p = _run("denoise", str(src), "-o", str(out), "--joint-chroma", "--strength", "5", "--chroma-strength", "7", *(["--temporal-radius", "1"] if D else []))
        assert p.returncode == 0, p.stderr[-2000:]
        assert "Denoised 6 frames" in p.stderr
        assert_clips_equal(_y4m_frames(out, 6), reference(frames, bd, sub, D, strength=5.0, chroma_strength=7.0), f"denoise --joint-chroma, D {D}")
    # `diff --denoise --joint-chroma --keep-denoised K` on a source the estimator finds flat blocks in: K is what `denoise
    # --joint-chroma` writes, the table what the two-file `diff SOURCE K` writes
    src, frames = _clip(tmp_path, n=8)
    den, kept, a_tbl, b_tbl = tmp_path / "den.y4m", tmp_path / "kept.y4m", tmp_path / "a.tbl", tmp_path / "b.tbl"
    p = _run("denoise", str(src), "-o", str(den), "--joint-chroma", "--strength", "5")
    assert p.returncode == 0, p.stderr[-2000:]
    got = _y4m_frames(den, len(frames))
    for t in (0, len(frames) - 1):
        assert_planes_equal(got[t], reference([frames[t]], bd, sub, strength=5.0)[0], f"denoise --joint-chroma frame {t}")
    p = _run("diff", str(src), "--denoise", "--joint-chroma", "--strength", "5", "-o", str(a_tbl), "--keep-denoised", str(kept))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Computed diff for {len(frames)} frames" in p.stderr
    assert kept.read_bytes() == den.read_bytes()
    p = _run("diff", str(src), str(kept), "-o", str(b_tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    assert a_tbl.read_bytes() == b_tbl.read_bytes()
