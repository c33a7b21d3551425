"""`denoise` with a grain prior (rules 12 - 15) on the device.  Every case asserts three things: the luma bytes equal
tests/denoise_curve_ref.py, the chroma bytes equal those of a Denoiser made without the curve, and the inputs are
unchanged.  Sizes around kd_curve's 16-sample step and the tiles, every entry of both tables, the clamp above M, the
curves, views, frames of every kind of memory, batches, clips, geometry changes, joint chroma, the widest plane, the
refusals and the commands."""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import denoise_curve_ref as CR
from tests import views as V
from tests.denoise_curve_cases import curve_points
from tests.test_denoise_curve_cpu import EXAMPLE, segment
from tests.test_gpu_denoise import _clip, _run, gradient
from tests.test_gpu_denoise_temporal import _y4m_frames, gradient_clip, moving_clip
from tests.test_gpu_grain import SUBSAMPLINGS, _to_dev, assert_planes_equal

pytestmark = pytest.mark.gpu

_CURVES = {}


def curve(name: str, bd: int):
    """(fwd, inv) of one of tests/denoise_curve_cases.py's priors: flat (R = 1), step (two levels, the largest R), example."""
    from grav1synth_amd.denoise import grain_curve

    if (name, bd) not in _CURVES:
        points, rng = curve_points(name)
        _CURVES[name, bd] = grain_curve([segment(p) for p in points], bd, CR.max_range(bd) if rng < 0 else rng)
    return _CURVES[name, bd]


def check_clip(frames, bd, sub, cv, what, D=0, joint=False, batch=0, A=3, S=2, strength=4.0, chroma_strength=0.0):
    """One clip of contiguous device frames through a denoiser with the curve and one without: the three assertions."""
    from grav1synth_amd.denoise import Denoiser

    kw = dict(search_radius=A, patch_radius=S, strength=strength, chroma_strength=chroma_strength, temporal_radius=D, batch_frames=batch, joint_chroma=joint)
    dev = [_to_dev(f, bd) for f in frames]
    with_curve, without = Denoiser(bd, curve=cv, **kw), Denoiser(bd, **kw)
    try:
        got, plain = with_curve.denoise_clip(dev, *sub), without.denoise_clip(dev, *sub)
    finally:
        with_curve.close(), without.close()
    luma = CR.denoise_luma_clip([f[0] for f in frames], cv[0], cv[1], D, A, S, strength)
    for t, f in enumerate(frames):
        assert_planes_equal(got[t][:1], [luma[t]], f"{what}: luma of frame {t}")
        assert_planes_equal(got[t][1:], [p.cpu().numpy() for p in plain[t][1:]], f"{what}: chroma of frame {t} against the denoiser without a curve")
        assert_planes_equal(dev[t], f, f"{what}: input frame {t} after the call")
    return got, plain


SIZES = [(1, 1), (7, 3), (8, 1), (9, 2), (15, 5), (16, 16), (17, 1), (33, 2), (63, 47), (64, 48), (65, 49), (130, 50)]


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes_depths_and_formats(size):
    w, h = size
    for bd in (8, 10):
        for k, ss in enumerate(("420", "444", "mono")):
            sub = SUBSAMPLINGS.get(ss, (1, 1))
            frame = gradient(w, h, bd, *sub, seed=w + h, mono=ss == "mono", amp=9)
            name = ("example", "step", "flat")[(k + (bd == 10)) % 3]
            check_clip([frame], bd, sub, curve(name, bd), f"{w}x{h} {bd} bit {ss} {name}")


@pytest.mark.parametrize("bd", [8, 10])
def test_every_entry_of_both_tables(bd):
    """A (M + 1) x 2 ramp holds every input value, so every entry of the forward table is read; full-range noise under a
    large strength gives means all over the stabilised domain for the inverse."""
    M = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    ramp = [np.ascontiguousarray(np.stack([np.arange(M + 1), np.arange(M, -1, -1)]).astype(dt))]
    cv = curve("step", bd)
    check_clip([ramp], bd, (1, 1), cv, f"{bd} bit ramp", A=1, S=1)
    check_clip([ramp], bd, (1, 1), curve("example", bd), f"{bd} bit ramp, the example table", A=2, S=1, strength=0.5)
    noise = [np.random.default_rng(bd).integers(0, M + 1, (50, 130)).astype(dt)]
    got, _ = check_clip([noise], bd, (1, 1), curve("example", bd), f"{bd} bit full-range noise", strength=1000.0)
    assert np.unique(got[0][0].cpu().numpy()).size > 3, "means all over the range"
    check_clip([noise], bd, (1, 1), cv, f"{bd} bit full-range noise, step", strength=2.0)


def test_values_above_the_maximum_read_as_the_maximum():
    bd = 10
    frame = gradient(70, 20, bd, 1, 1, seed=3, mono=True, amp=9)
    clean = [frame[0].copy()]
    clean[0][3, 5], clean[0][10, 64], clean[0][19, 69], clean[0][0, 0] = 1023, 1023, 1023, 1023
    wild = [clean[0].copy()]
    wild[0][3, 5], wild[0][10, 64], wild[0][19, 69], wild[0][0, 0] = 1024, 65535, 1024, 65535
    cv = curve("step", bd)
    got, _ = check_clip([wild], bd, (1, 1), cv, "values above M")
    want = CR.denoise_luma(clean[0], cv[0], cv[1], 3, 2, 4.0)
    assert np.array_equal(got[0][0].cpu().numpy(), want), "1024 and 65535 were read as 1023"


@pytest.mark.parametrize("where", ["in", "out", "both"])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(where):
    from grav1synth_amd.denoise import Denoiser

    for bd, ss in ((8, "420"), (10, "444")):
        sub, isz, top = SUBSAMPLINGS[ss], 1 if bd == 8 else 2, (1 << bd) - 1
        frames = gradient_clip(3, 67, 21, bd, *sub, seed=4, amp=9)
        cv = curve("step", bd)
        kw = dict(temporal_radius=1, batch_frames=2)
        with_curve, without = Denoiser(bd, curve=cv, **kw), Denoiser(bd, **kw)
        guards_in, guards_out, outs, plain = [], [], [], []
        for t, f in enumerate(frames):
            fin, out = _to_dev(f, bd), None
            if where in ("in", "both"):
                made = [V.device_view(p, pitch_bytes=(p.shape[1] + 13 + c) * isz, base_offset_bytes=(3 + c) * isz, max_code=top, seed=t) for c, p in enumerate(f)]
                fin, guards_in = [v for v, _g in made], guards_in + [g for _v, g in made]
            if where in ("out", "both"):
                made = [V.device_view(np.zeros_like(p), pitch_bytes=(p.shape[1] + 9) * isz, base_offset_bytes=5 * isz, fill="max", max_code=top, seed=t) for p in f]
                out, guards_out = [v for v, _g in made], guards_out + [g for _v, g in made]
            outs.append(with_curve.apply(fin, *sub, sync=False, out=out))
            plain.append(without.apply(_to_dev(f, bd), *sub, sync=False))
        with_curve.sync(), without.sync()
        luma = CR.denoise_luma_clip([f[0] for f in frames], cv[0], cv[1], 1, 3, 2, 4.0)
        for t in range(3):
            assert_planes_equal(outs[t][:1], [luma[t]], f"{bd} bit views {where}: luma of frame {t}")
            assert_planes_equal(outs[t][1:], [p.cpu().numpy() for p in plain[t][1:]], f"{bd} bit views {where}: chroma of frame {t}")
        for g in guards_in:
            g.assert_unchanged("a strided input")
        for g in guards_out:
            g.assert_margin_intact("a strided output")
        with_curve.close(), without.close()


def test_one_clip_of_host_pinned_device_and_strided_frames():
    import torch

    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.diff import Frame

    bd, sub, D = 10, (1, 1), 1
    frames = moving_clip(8, 99, 37, bd, *sub, seed=2)
    cv = curve("example", bd)
    luma = CR.denoise_luma_clip([f[0] for f in frames], cv[0], cv[1], D, 3, 2, 4.0)
    without = Denoiser(bd, batch_frames=3, temporal_radius=D)
    plain = without.denoise_clip([_to_dev(f, bd) for f in frames], *sub)
    without.close()
    dn = Denoiser(bd, batch_frames=3, temporal_radius=D, curve=cv)
    L = _lib.lib()
    outs, guards_in, guards_out, keep, dev_in = [], [], [], [], []
    for t, planes in enumerate(frames):
        kind = ("view", "host", "pinned", "device")[t % 4]
        if kind == "host":
            host_in = [p.copy() for p in planes]
            outs.append(dn.apply(host_in, *sub, sync=False))
            dev_in.append((host_in, planes))
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
            dev_in.append(([p.numpy() for p in pin_in], planes))
        elif kind == "device":
            dev_in.append((_to_dev(planes, bd), planes))
            outs.append(dn.apply(dev_in[-1][0], *sub, sync=False))
        else:
            vin = [V.device_view(p, pitch_bytes=p.shape[1] * 2 + 26 + 2 * c, base_offset_bytes=6 + 2 * c, max_code=1023, seed=t) for c, p in enumerate(planes)]
            vout = [V.device_view(np.zeros_like(p), pitch_bytes=p.shape[1] * 2 + 18, base_offset_bytes=10, fill="max", max_code=1023, seed=t) for p in planes]
            guards_in += [g for _v, g in vin]
            guards_out += [g for _v, g in vout]
            outs.append(dn.apply([v for v, _g in vin], *sub, sync=False, out=[v for v, _g in vout]))
        if t == 5:
            assert dn.drain() == 6 - D
    dn.sync()
    for t in range(len(frames)):
        assert_planes_equal(outs[t][:1], [luma[t]], f"mixed memory: luma of frame {t}")
        assert_planes_equal(outs[t][1:], [p.cpu().numpy() for p in plain[t][1:]], f"mixed memory: chroma of frame {t}")
    for g in guards_in:
        g.assert_unchanged("a strided input")
    for g in guards_out:
        g.assert_margin_intact("a strided output")
    for dev, planes in dev_in:
        assert_planes_equal(dev, planes, "an input after the call")
    dn.close()


@pytest.mark.parametrize("batch", [1, 5, 4])
def test_batches_of_1_n_and_one_less_than_the_clip(batch):
    bd, sub = 8, (1, 1)
    frames = gradient_clip(5, 45, 35, bd, *sub, seed=2, amp=9)
    for D in (0, 1):
        check_clip(frames, bd, sub, curve("step", bd), f"5 frames in batches of {batch}, D {D}", D=D, batch=batch)


@pytest.mark.parametrize("D", [1, 2])
def test_clips_shorter_than_the_window_and_drains_at_irregular_points(D):
    from grav1synth_amd.denoise import Denoiser

    bd, sub = 10, (1, 1)
    frames = moving_clip(9, 70, 52, bd, *sub, seed=1)
    cv = curve("example", bd)
    for n in (1, 2, 3):
        check_clip(frames[:n], bd, sub, cv, f"{n} frames at D {D}", D=D)
    want = CR.denoise_luma_clip([f[0] for f in frames], cv[0], cv[1], D, 3, 2, 4.0)
    spatial = CR.denoise_luma_clip([f[0] for f in frames], cv[0], cv[1], 0, 3, 2, 4.0)
    assert all((a != b).any() for a, b in zip(want, spatial)), "the neighbours did something"
    dev = [_to_dev(f, bd) for f in frames]
    without = Denoiser(bd, batch_frames=4, temporal_radius=D)
    plain = without.denoise_clip(dev, *sub)
    without.close()
    drained = Denoiser(bd, batch_frames=4, temporal_radius=D, curve=cv)
    outs = []
    for k, f in enumerate(dev):
        outs.append(drained.apply(f, *sub, sync=False))
        if k in (0, 2, 3, 6):
            done = drained.drain()
            assert done == max(k + 1 - D, 0), (k, done)
            if done:
                assert_planes_equal(outs[done - 1][:1], [want[done - 1]], f"luma of frame {done - 1} after the drain at {k}")
    drained.sync()
    assert drained.drain() == 9
    drained.close()
    for t in range(9):
        assert_planes_equal(outs[t][:1], [want[t]], f"with drains: luma of frame {t}")
        assert_planes_equal(outs[t][1:], [p.cpu().numpy() for p in plain[t][1:]], f"with drains: chroma of frame {t}")
        assert_planes_equal(dev[t], frames[t], f"input frame {t} after the call")


def test_a_geometry_change_in_mid_queue_and_one_denoiser_meeting_two_geometries():
    from grav1synth_amd.denoise import Denoiser

    bd, sub, D = 10, (1, 1), 1
    frames = gradient_clip(6, 100, 60, bd, *sub, seed=4, amp=9)
    small = gradient_clip(2, 70, 50, bd, 0, 0, seed=5, amp=9)
    mono = gradient_clip(1, 131, 33, bd, 0, 0, seed=6, mono=True, amp=9)
    cv = curve("step", bd)
    ref = lambda clip: CR.denoise_luma_clip([f[0] for f in clip], cv[0], cv[1], D, 3, 2, 4.0)
    dev = [_to_dev(f, bd) for f in frames]
    dn, without = Denoiser(bd, temporal_radius=D, batch_frames=4, curve=cv), Denoiser(bd, temporal_radius=D, batch_frames=4)

    def through(d):
        outs = [d.apply(f, *sub, sync=False) for f in dev[:3]]
        outs += [d.apply(f, 0, 0, sync=False) for f in small]      # host frames of another geometry, 4:4:4
        outs.append(d.apply(mono[0], 0, 0, sync=False))             # then a luma-only one
        outs += [d.apply(f, *sub, sync=False) for f in dev[3:]]     # then the first geometry again
        d.sync()
        return outs

    got, plain = through(dn), through(without)
    want = ref(frames[:3]) + ref(small) + ref(mono) + ref(frames[3:])
    for t in range(len(got)):
        assert_planes_equal(got[t][:1], [want[t]], f"luma of frame {t}")
        assert_planes_equal(got[t][1:], [np.asarray(p.cpu() if hasattr(p, "cpu") else p) for p in plain[t][1:]], f"chroma of frame {t}")
    # the kept denoiser again, each geometry as a clip of its own
    again = dn.denoise_clip(dev, *sub)
    for t, y in enumerate(ref(frames)):
        assert_planes_equal(again[t][:1], [y], f"one clip of six: luma of frame {t}")
    other = dn.denoise_clip([_to_dev(f, bd) for f in small], 0, 0)
    for t, y in enumerate(ref(small)):
        assert_planes_equal(other[t][:1], [y], f"the other geometry: luma of frame {t}")
    for t, f in enumerate(frames):
        assert_planes_equal(dev[t], f, f"input frame {t} after the calls")
    dn.close(), without.close()


def test_joint_chroma_with_a_temporal_radius():
    """Rule 15: the guide is the unstabilised input luma, so the chroma bytes are those of joint chroma without a curve."""
    for bd, ss in ((8, "420"), (10, "422")):
        sub = SUBSAMPLINGS[ss]
        frames = moving_clip(4, 131, 99, bd, *sub, seed=3)
        got, plain = check_clip(frames, bd, sub, curve("step", bd), f"joint chroma {bd} bit {ss}", D=1, joint=True, batch=3, chroma_strength=6.0)
        assert any((a[0] != b[0]).any() for a, b in zip(got, plain)), "the curve did something to luma"


def test_the_widest_plane():
    bd = 10
    y = np.random.default_rng(9).integers(0, 1024, (4, 65536)).astype(np.uint16)
    y[:, ::2] = (np.arange(32768)[None, :] // 32).astype(np.uint16)
    check_clip([[y]], bd, (1, 1), curve("example", bd), "65536 x 4", A=2, S=1, strength=8.0)


def test_every_constructor_refusal_and_the_stickiness_of_an_error():
    from grav1synth_amd.denoise import Denoiser

    for bd in (8, 10):
        M = (1 << bd) - 1
        f, i = curve("example", bd)

        def mutated(a, at, value):
            b = a.copy()
            b[at] = value
            return b

        shifted = i.copy()
        shifted[int(f[M // 3 - 1]):int(f[M // 3]) + 1] = M // 3 - 1
        for text, cv in (("curve: fwd must run from 0 to 4095", (mutated(f, 0, 1), i)), ("curve: fwd must run from 0 to 4095", (mutated(f, M, 4094), i)),
                         ("curve: fwd must be strictly increasing (at 7)", (mutated(f, 7, 0), i)),
                         ("curve: inv must be non-decreasing (at 2001)", (f, mutated(i, 2001, i[2000] - 1))),
                         ("curve: inv must stay within the clip's bit depth (at 4095)", (f, mutated(i, 4095, M + 1))),
                         (f"curve: inv[fwd[x]] must be x (at {M // 3})", (f, shifted)),
                         (f"fwd must have {M + 1} entries and inv 4096", (f[:-1], i)), (f"fwd must have {M + 1} entries and inv 4096", (f, i[:-1]))):
            with pytest.raises(_lib.G1SError) as e:
                Denoiser(bd, curve=cv)
            assert text in str(e.value)
        for text, kw in (("temporal_radius must be 0..3", dict(temporal_radius=4)), ("search_radius must be 1..7", dict(search_radius=8)),
                         ("patch_radius must be 1..4", dict(patch_radius=5)), ("strength must be greater than 0", dict(strength=-1.0))):
            with pytest.raises(_lib.G1SError) as e:
                Denoiser(bd, curve=(f, i), **kw)
            assert text in str(e.value)
    with pytest.raises(_lib.G1SError) as e:
        Denoiser(12, curve=(np.zeros(4096, np.uint16), np.zeros(4096, np.uint16)))
    assert "a 12-bit clip is refused" in str(e.value)
    # an error of a frame is sticky: input and output that overlap, then a frame that is fine
    bd = 10
    dn = Denoiser(bd, curve=curve("example", bd))
    frame = _to_dev(gradient(40, 30, bd, 1, 1, seed=1, mono=True), bd)
    with pytest.raises(_lib.G1SError) as e:
        dn.apply(frame, out=frame)
    assert "input and output planes overlap" in str(e.value)
    with pytest.raises(_lib.G1SError) as e2:
        dn.apply(frame)
    assert str(e2.value) == str(e.value)
    dn.close()


def test_the_commands_end_to_end(tmp_path):
    from grav1synth_amd.denoise import denoise_y4m_file, grain_curve
    from grav1synth_amd.ingest import write_y4m
    from grav1synth_amd.tbl import parse_tbl

    bd, sub = 8, (1, 1)
    frames = moving_clip(6, 96, 64, bd, *sub, seed=3)
    src = tmp_path / "moving.y4m"
    write_y4m(str(src), frames, bd, *sub, Fraction(24, 1))
    prior = tmp_path / "prior.tbl"
    prior.write_bytes(open(EXAMPLE, "rb").read().replace(b"E 0 26460000000 1 7391 1", b"E 0 100 1 7391 1") +
                      b"E 100 26460000000 1 11 1\n\tp 0 6 0 8 0 1 0 0 0 0 0 0\n\tsY 2  0 10 255 90\n\tsCb 0\n\tsCr 0\n\tcY\n\tcCb 0\n\tcCr 0\n")
    segs = parse_tbl(prior.read_bytes())
    assert len(segs) == 2
    plain = tmp_path / "plain.y4m"
    assert _run("denoise", str(src), "-o", str(plain), "--strength", "5", "--temporal-radius", "1").returncode == 0
    plain_frames = _y4m_frames(plain, 6)
    for args, cv in ((["--grain-prior", str(prior)], grain_curve(segs, bd)),
                     (["--grain-prior", str(prior), "--prior-range", "9", "--prior-segment", "1"], grain_curve(segs, bd, 9, segment=1))):
        out = tmp_path / f"den{len(args)}.y4m"
        p = _run("denoise", str(src), "-o", str(out), "--strength", "5", "--temporal-radius", "1", *args)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "Denoised 6 frames" in p.stderr
        got = _y4m_frames(out, 6)
        luma = CR.denoise_luma_clip([f[0] for f in frames], cv[0], cv[1], 1, 3, 2, 5.0)
        for t in range(6):
            assert_planes_equal(got[t][:1], [luma[t]], f"denoise {' '.join(args[2:])}: luma of frame {t}")
            assert_planes_equal(got[t][1:], plain_frames[t][1:], f"denoise {' '.join(args[2:])}: chroma of frame {t}")
    o2 = tmp_path / "py.y4m"
    assert denoise_y4m_file(str(src), str(o2), strength=5.0, temporal_radius=1, grain_prior=str(prior), prior_range=9, prior_segment=1) == 6
    assert o2.read_bytes() == out.read_bytes()
    # `diff SOURCE --denoise --grain-prior T --keep-denoised K`: K is what `denoise --grain-prior T` writes, the table what
    # the two-file `diff SOURCE K` writes
    src, frames = _clip(tmp_path, n=8)
    den, kept, a_tbl, b_tbl = tmp_path / "den.y4m", tmp_path / "kept.y4m", tmp_path / "a.tbl", tmp_path / "b.tbl"
    p = _run("denoise", str(src), "-o", str(den), "--grain-prior", str(prior), "--strength", "5")
    assert p.returncode == 0, p.stderr[-2000:]
    p = _run("diff", str(src), "--denoise", "--grain-prior", str(prior), "--strength", "5", "-o", str(a_tbl), "--keep-denoised", str(kept))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Computed diff for {len(frames)} frames" in p.stderr
    assert kept.read_bytes() == den.read_bytes()
    p = _run("diff", str(src), str(kept), "-o", str(b_tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    assert a_tbl.read_bytes() == b_tbl.read_bytes() and a_tbl.read_bytes().startswith(b"filmgrn1")
    cv = grain_curve(segs, 8)
    assert_planes_equal(_y4m_frames(kept, len(frames))[0][:1], [CR.denoise_luma(frames[0][0], cv[0], cv[1], 3, 2, 5.0)], "the kept clip's first luma")
    assert os.path.getsize(a_tbl) > 20
