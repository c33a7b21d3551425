"""Noise levels on the device against tests/nlf_ref.py: every field of every record with array_equal, every report byte for
byte.  There is no tolerance anywhere."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import content as CT
from tests import grain_ref as G
from tests import nlf_ref as R
from tests import views as V
from tests.test_gpu_grain import _to_dev, make_segment
from tests.test_nlf_cpu import SUBSAMPLINGS, smooth_planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP_COLS, STRIP_ROWS = 496, 32  # k_nlf's strip of a wave


@pytest.fixture(scope="module")
def meters():
    from grav1synth_amd.estimate import NoiseLevelMeter

    made = {}

    def get(bd, **kw):
        key = (bd, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = NoiseLevelMeter(bd, **kw)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def check_frame(meter, planes, bd, subx, suby, what, dev=True, want=None):
    meter.frame(_to_dev(planes, bd) if dev else planes, subx, suby)
    got = meter.finish()
    assert len(got) == 1
    want = R.nlf_frame(planes, bd, subx, suby) if want is None else want
    bad = R.mismatches(got[0], want, what)
    assert not bad, "\n".join(bad)
    return want


# ------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
def test_formats_on_plane_distinct_content_with_rendered_grain(meters, bd, ss):
    mono = ss == "mono"
    subx, suby = (1, 1) if mono else SUBSAMPLINGS[ss]
    _src, den = CT.make_frames("distinct", 208, 136, bd, subx, suby, frame=1)
    grainy = G.add_noise(den, make_segment(3, 50 + bd), bd, subx, suby)
    if mono:
        grainy = grainy[:1]
    want = check_frame(meters(bd), grainy, bd, subx, suby, f"{bd} bit {ss}")
    assert want["q"][0].any() and np.count_nonzero(want["n"][0]) > 3
    assert mono or (want["q"][1].any() and not np.array_equal(want["q"][1], want["q"][2])), "the planes differ"


SMALL = [(1, 1), (2, 7), (7, 2), (3, 3)]
WIDTHS = [(w, 6) for w in (495, 496, 497, 498, 991, 992, 993, 994)]
HEIGHTS = [(21, h) for h in (33, 34, 35, 65, 66, 67)]


@pytest.mark.parametrize("size", SMALL + WIDTHS + HEIGHTS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_round_the_strip_and_below_the_stencil(meters, size):
    w, h = size
    for bd, ss in ((8, "444"), (10, "mono"), (12, "444"), (10, "420")):
        subx, suby = SUBSAMPLINGS[ss]
        planes = smooth_planes(w, h, bd, ss, seed=2)
        want = check_frame(meters(bd), planes, bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
        if w >= 21 and h >= 6:
            assert want["n"][0].sum() > 0
        if w < 3 or h < 3:
            assert not want["n"].any()


@pytest.mark.parametrize("size", [(995, 37), (2 * 994 + 1, 5), (37, 131), (5, 5), (7, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_odd_luma_sizes_under_decimated_chroma(meters, size):
    """4:2:0 and 4:2:2 with odd luma sizes: the last chroma column sits on the last luma column (averageLuma's clamp) and the
    chroma strips end where the luma's do not."""
    w, h = size
    for bd, ss in ((8, "420"), (10, "422"), (12, "420")):
        subx, suby = SUBSAMPLINGS[ss]
        planes = smooth_planes(w, h, bd, ss, seed=9)
        want = check_frame(meters(bd), planes, bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
        assert w < 9 or want["n"][1].sum() > 0


# ------------------------------------------------------------------------------------------------- adversarial content
def test_a_checkerboard_at_12_bits(meters):
    """0 / 4095, 130 x 70: every interior sample counts with the largest |L| there is, 8 x 4095 = 32760.  Five such squares
    leave 32 bits and a lane adds 256 in a strip: this catches a 32-bit q."""
    w, h = 130, 70
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    board = np.where((xs + ys) & 1, 4095, 0).astype(np.uint16)
    planes = [board, board[:, ::-1].copy(), board.copy()]
    want = check_frame(meters(12), planes, 12, 0, 0, "checkerboard")
    assert int(want["n"][0].sum()) == (w - 2) * (h - 2) and int(want["q"][0].sum()) == (w - 2) * (h - 2) * 32760 ** 2
    assert int(want["q"][1].sum()) == int(want["q"][0].sum())


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_adversarial_bins(meters, bd):
    w, h, step, up = 600, 75, 1 << (bd - 5), 1 << (bd - 8)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    rng = np.random.default_rng(bd)
    dt = np.uint8 if bd == 8 else np.uint16
    noise = rng.integers(-2 * up, 2 * up + 1, (h, w))
    cases = {
        "one intensity": np.full((h, w), 11 * step + 3) + 0 * noise,
        "one intensity with noise": np.full((h, w), 11 * step + step // 2) + noise,
        # (a checkerboard of A = 8 step - 5 and B = 8 step + 4: the box mean is 8 step - 1 around an A and 8 step around a B)
        "two bins alternating sample by sample": np.where((xs + ys) & 1, 8 * step - 5, 8 * step + 4) + 0 * noise,
        "two bins, column by column": np.where(xs & 1, 20 * step, 20 * step + 3 * up) + 0 * ys,
        "a ramp through all 32 bins": np.minimum((xs * 32 * step) // w, (1 << bd) - 1) + 0 * ys + noise.clip(0, None),
        "a ramp down the rows": np.minimum((ys * 32 * step) // h, (1 << bd) - 1) + 0 * xs,
        "isolated full-scale spikes on a period-2 lattice": np.where((xs % 2 == 0) & (ys % 2 == 0), (1 << bd) - 1, 0),
        "spikes of the gate's height on a period-2 lattice": np.where((xs % 2 == 0) & (ys % 2 == 0), 9 * step + 2 * up, 9 * step),
    }
    for what, luma in cases.items():
        luma = np.clip(luma, 0, (1 << bd) - 1).astype(dt)
        chroma = [np.ascontiguousarray(luma[::2, ::2]), np.ascontiguousarray(luma[::2, ::2][:, ::-1])]
        want = check_frame(meters(bd), [luma] + chroma, bd, 1, 1, f"{bd} bit, {what}")
        if what == "one intensity":
            assert np.count_nonzero(want["n"][0]) == 1 and not want["q"].any() and int(want["n"][0].sum()) == (w - 2) * (h - 2)
        if what.startswith("a ramp through"):
            assert np.count_nonzero(want["n"][0]) == 32
        if what.startswith("two bins alternating"):
            k = np.flatnonzero(want["n"][0])
            assert len(k) == 2 and abs(int(want["n"][0][k[0]]) - int(want["n"][0][k[1]])) <= 1, want["n"][0]
        if what.startswith("spikes of the gate"):
            assert want["n"][0].sum() > 0 and want["q"][0].any()


# ------------------------------------------------------------------------------------------------------------ plumbing
@pytest.mark.parametrize("bd,ss", [(8, "420"), (10, "422"), (12, "444")])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    isz = 1 if bd == 8 else 2
    planes = smooth_planes(547, 71, bd, ss, seed=4)
    want = R.nlf_frame(planes, bd, subx, suby)
    assert want["n"][1].sum() > 0
    for k, (extra, base) in enumerate(((6, 2), (34, 14), (0, 250), (130, 6), (8, 16))):
        guards, dev = [], []
        for c, p in enumerate(planes):
            view, guard = V.device_view(p, pitch_bytes=p.shape[1] * isz + extra * isz, base_offset_bytes=(base + 2 * c) % 256 & ~(isz - 1),
                                        fill="random" if k & 1 else "max", max_code=(1 << bd) - 1, seed=10 * k + c)
            dev.append(view)
            guards.append(guard)
        meters(bd).frame(dev, subx, suby)
        got = meters(bd).finish()
        bad = R.mismatches(got[0], want, f"view {k} {bd} bit {ss}")
        assert not bad, "\n".join(bad)
        for g in guards:
            g.assert_unchanged(f"view {k}")


def test_host_pinned_and_device_frames_in_one_batch(meters):
    import torch

    bd, (subx, suby) = 10, (1, 1)
    m = meters(bd, batch_frames=8)
    wants, keep = [], []
    for k in range(6):
        planes = smooth_planes(150, 90, bd, "420", seed=30 + k)
        wants.append(R.nlf_frame(planes, bd, subx, suby))
        kind = k % 3
        if kind == 1:
            planes = _to_dev(planes, bd)
        elif kind == 2:
            planes = [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
        keep.append(planes)
        m.frame(planes, subx, suby, async_host=True)
    got = m.finish()
    assert len(got) == 6
    for k in range(6):
        bad = R.mismatches(got[k], wants[k], f"frame {k}")
        assert not bad, "\n".join(bad)


@pytest.mark.parametrize("batch", [1, 5, 6])
def test_batches_of_one_of_all_and_of_one_more(batch):
    from grav1synth_amd.estimate import NoiseLevelMeter

    bd, n = 8, 5
    m = NoiseLevelMeter(bd, batch_frames=batch)
    wants = []
    for k in range(n):
        planes = smooth_planes(70, 50, bd, "420", seed=60 + k)
        wants.append(R.nlf_frame(planes, bd, 1, 1))
        m.frame(_to_dev(planes, bd) if k & 1 else planes, 1, 1)
    got = m.finish()
    assert len(got) == n
    for k in range(n):
        assert not R.mismatches(got[k], wants[k], f"batch {batch} frame {k}")
    m.close()


def test_capacity_geometry_change_and_reuse():
    from grav1synth_amd.estimate import NLF_RECORD, NoiseLevelMeter

    bd = 8
    m = NoiseLevelMeter(bd, batch_frames=4)
    wants = []
    for k in range(6):  # a batch and two queued frames
        planes = smooth_planes(70, 50, bd, "420", seed=70 + k)
        wants.append(R.nlf_frame(planes, bd, 1, 1))
        m.frame(planes, 1, 1)
    # another geometry in mid-queue sends the queued frames out first
    planes = smooth_planes(33, 41, bd, "444", seed=80)
    wants.append(R.nlf_frame(planes, bd, 0, 0))
    m.frame(planes, 0, 0)
    planes = smooth_planes(33, 41, bd, "mono", seed=81)
    wants.append(R.nlf_frame(planes, bd, 0, 0))
    m.frame(planes, 0, 0)
    n = C.c_size_t()
    small = np.zeros(5, NLF_RECORD)
    assert m._L.g1s_nlf_finish(m._h, small.ctypes.data, 5, C.byref(n)) == _lib.G1S_ERR_CAPACITY and n.value == 8
    with pytest.raises(_lib.G1SError):
        m.finish(cap=7)
    got = m.finish()
    assert len(got) == 8
    for k in range(8):
        bad = R.mismatches(got[k], wants[k], f"frame {k}")
        assert not bad, "\n".join(bad)
    assert not got[7]["n"][1:].any() and not got[7]["q"][1:].any(), "a luma-only frame has zeros for the chroma planes"
    assert len(m.finish()) == 0
    planes = smooth_planes(90, 20, bd, "422", seed=82)
    m.frame(planes, 1, 0)
    got = m.finish()
    assert len(got) == 1 and not R.mismatches(got[0], R.nlf_frame(planes, bd, 1, 0), "after finish")
    m.close()


def test_refusals():
    from grav1synth_amd.diff import Frame
    from grav1synth_amd.estimate import NoiseLevelMeter

    with pytest.raises(_lib.G1SError) as e:
        NoiseLevelMeter(9)
    assert "8, 10 and 12" in str(e.value)
    planes = smooth_planes(64, 40, 10, "420", seed=1)
    m = NoiseLevelMeter(8)
    with pytest.raises(_lib.G1SError) as e:
        m.frame(planes)
    assert "bytes_per_sample" in str(e.value)
    with pytest.raises(_lib.G1SError):  # sticky
        m.frame(smooth_planes(64, 40, 8, "420", seed=1))
    m.close()
    m = NoiseLevelMeter(10)
    keep = []
    f = Frame(planes, 1, 1).to_c(keep)
    f.stride_bytes[1] = planes[1].shape[1] * 2 - 2
    assert m._L.g1s_nlf_frame(m._h, C.byref(f)) == -1
    assert "row stride" in m._L.g1s_nlf_last_error(m._h).decode()
    m.close()
    m = NoiseLevelMeter(10)
    f = Frame(planes, 1, 1).to_c(keep)
    f.stride_bytes[0] = planes[0].shape[1] * 2 + 1  # an odd stride of 16-bit samples
    assert m._L.g1s_nlf_frame(m._h, C.byref(f)) == -1
    m.close()
    m = NoiseLevelMeter(10)
    f = Frame(planes, 1, 1).to_c(keep)
    f.xdec, f.ydec = 0, 1
    assert m._L.g1s_nlf_frame(m._h, C.byref(f)) == -1 and "unsupported frame geometry" in m._L.g1s_nlf_last_error(m._h).decode()
    m.close()


def test_the_longest_side(meters):
    """65 536 samples a side are taken, in a thin plane either way; one more is refused."""
    from grav1synth_amd.diff import Frame
    from grav1synth_amd.estimate import NoiseLevelMeter

    bd = 8
    rng = np.random.default_rng(6)
    for w, h in ((65536, 3), (4, 65536)):
        y = (100 + rng.integers(0, 4, (h, w))).astype(np.uint8)
        if w > h:  # (another bin in the last strip)
            y[:, -3:] = 180 + rng.integers(0, 4, (h, 3))
        else:
            y[-3:, :] = 180 + rng.integers(0, 4, (3, w))
        want = check_frame(meters(bd), [y], bd, 0, 0, f"{w}x{h}")
        assert int(want["n"][0].sum()) > (w - 2) * (h - 2) // 2 and np.count_nonzero(want["n"][0]) >= 2
    for w, h in ((65537, 3), (3, 65537)):
        m = NoiseLevelMeter(bd)
        keep = []
        f = Frame([np.zeros((h, w), np.uint8)], 0, 0).to_c(keep)
        assert m._L.g1s_nlf_frame(m._h, C.byref(f)) == -1 and "up to 65536 x 65536" in m._L.g1s_nlf_last_error(m._h).decode()
        m.close()


# --------------------------------------------------------------------------------------------------------- consistency
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_luma_totals_give_the_estimators_value(meters, bd):
    from grav1synth_amd.estimate import NoiseEstimator

    frames = [smooth_planes(w, h, bd, "mono", seed=90 + k, amp=amp)[0] for k, (w, h, amp) in enumerate(((320, 192, 2), (1000, 70, 5), (5, 5, 1), (64, 64, 400)))]
    values = []
    for y in frames:
        est = NoiseEstimator(bd)  # (an estimator takes one geometry)
        est.estimate_frame(y)
        values += est.finish()
        est.close()
        meters(bd).frame([y], 0, 0)
    recs = meters(bd).finish()
    assert len(values) == len(recs) == len(frames)
    for v, r in zip(values, recs):
        n, a = int(r["n"][0].sum()), int(r["a"][0].sum())
        assert (None if n < 16 else float(a) / float(6 * n) * R.SQRT_PI_BY_2) == v, (n, a, v)


def test_the_prior_and_strength_of_a_measured_clip_go_into_the_denoiser(meters):
    """noise_prior's pair is what Denoiser(curve=...) takes, and auto_strength's values its strengths: the library's
    numbers are the restatement's, from records measured on the device."""
    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.estimate import auto_strength, noise_levels_sum, noise_prior

    bd, w, h = 10, 96, 64
    frames = [_two_level_frame(k, w, h, bd) for k in range(4)]
    for f in frames:
        meters(bd).frame(f, 1, 1)
    total = noise_levels_sum(meters(bd).finish())
    want = R.sum_records([R.nlf_frame(f, bd, 1, 1) for f in frames])
    assert not R.mismatches(total, want, "clip")
    fwd, inv = noise_prior(total, bd, min_count=256)
    wf, wi = R.curve_from_s(R.sigma(want, bd, 256), bd)
    assert np.array_equal(fwd, wf) and np.array_equal(inv, wi)
    assert len(set(R.sigma(want, bd, 256).tolist())) > 1, "two intensities with two noise levels: the curve is not flat"
    hl, hc = auto_strength(total, bd, 256)
    assert (hl, hc) == (R.strength(want, bd, 256, 0), R.strength(want, bd, 256, 1)) and hl > 0 and hc > 0
    d = Denoiser(bd, curve=(fwd, inv), strength=hl, chroma_strength=hc)
    out = d.apply(frames[0], 1, 1)
    d.close()
    assert [np.asarray(p).shape for p in out] == [p.shape for p in frames[0]]


def _two_level_frame(k, w, h, bd):
    """4:2:0: two intensities side by side, the brighter one with three times the noise."""
    rng = np.random.default_rng([11, k])
    up = 1 << (bd - 8)
    out = []
    for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
        xs = np.arange(pw)[None, :]
        base = np.where(xs < pw // 2, 60 * up, 170 * up) + np.zeros((ph, 1), np.int64)
        sg = np.where(xs < pw // 2, 1.0 * up, 3.0 * up)
        out.append(np.clip(np.rint(base + rng.standard_normal((ph, pw)) * sg), 0, (1 << bd) - 1).astype(np.uint16))
    return out


# ------------------------------------------------------------------------------------------------------------ commands
def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "grav1synth_amd", *args], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT,
                          stdin=subprocess.DEVNULL)


def test_estimate_levels_command_and_the_file_call(tmp_path):
    from grav1synth_amd.estimate import noise_levels_y4m_file
    from grav1synth_amd.ingest import write_y4m
    from tests.oracle_binding import estimate_plane_noise

    bd, w, h, n = 10, 96, 64, 4
    frames = [_two_level_frame(k, w, h, bd) for k in range(n)]
    src, out, lev = tmp_path / "src.y4m", tmp_path / "est.txt", tmp_path / "levels.txt"
    write_y4m(str(src), frames, bd, 1, 1, Fraction(24, 1))
    p = _run("estimate", str(src), "-o", str(out), "--levels", str(lev))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Done, wrote output file to {out}" in p.stderr and f"Done, wrote noise levels to {lev}" in p.stderr
    total = R.sum_records([R.nlf_frame(f, bd, 1, 1) for f in frames])
    assert lev.read_bytes() == R.format_noise_levels(total, n, bd, 3)
    want = "filmgrn1\n" + "".join("%.3f\n" % estimate_plane_noise(f[0], bd) for f in frames)
    assert out.read_text() == want
    # without --levels the command writes what it wrote
    out2 = tmp_path / "est2.txt"
    p = _run("estimate", str(src), "-o", str(out2))
    assert p.returncode == 0 and out2.read_text() == want and "noise levels" not in p.stderr
    # the library's own loop over the file: the same record, the same report; a prefix of the clip
    lev2 = tmp_path / "levels2.txt"
    got_n, got = noise_levels_y4m_file(str(src), str(lev2), batch_frames=3)
    assert got_n == n and not R.mismatches(got, total, "file") and lev2.read_bytes() == lev.read_bytes()
    got_n, got = noise_levels_y4m_file(str(src), None, max_frames=2)
    assert got_n == 2 and not R.mismatches(got, R.sum_records([R.nlf_frame(f, bd, 1, 1) for f in frames[:2]]), "prefix")
    with pytest.raises(_lib.G1SError):
        noise_levels_y4m_file(str(tmp_path / "missing.y4m"))


@pytest.fixture(scope="module")
def auto_clip(tmp_path_factory):
    """The 96 x 64 10-bit 4:2:0 clip of 4 frames with two intensities, as a file; its reference record; and the clip that
    Denoiser(curve=noise_prior(reference record), strength=reference h) makes of it, as a file."""
    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.estimate import NLF_RECORD, noise_prior
    from grav1synth_amd.ingest import write_y4m

    bd, w, h, n, nmin = 10, 96, 64, 4, 256
    d = tmp_path_factory.mktemp("auto")
    frames = [_two_level_frame(k, w, h, bd) for k in range(n)]
    src, den = d / "src.y4m", d / "den.y4m"
    write_y4m(str(src), frames, bd, 1, 1, Fraction(24, 1))
    total = R.sum_records([R.nlf_frame(f, bd, 1, 1) for f in frames])
    fwd, inv = noise_prior(R.to_struct(total, NLF_RECORD), bd, min_count=nmin)
    assert np.array_equal(fwd, R.curve_from_s(R.sigma(total, bd, nmin), bd)[0])
    hl, hc = R.strength(total, bd, nmin, 0), R.strength(total, bd, nmin, 1)
    dn = Denoiser(bd, curve=(fwd, inv), strength=hl, chroma_strength=hc)
    write_y4m(str(den), [[np.asarray(p) for p in dn.apply(f, 1, 1)] for f in frames], bd, 1, 1, Fraction(24, 1))
    dn.close()
    plain = Denoiser(bd)
    assert any(not np.array_equal(a, b) for a, b in zip(plain.apply(frames[0], 1, 1), dn_first(den, frames[0]))), "the measured job is not the default one"
    plain.close()
    return dict(src=src, den=den, dir=d, nmin=nmin, n=n)


def dn_first(path, like):
    """The first frame of a .y4m file as planes shaped like `like`."""
    from grav1synth_amd.ingest import Y4MReader

    rd = Y4MReader(str(path))
    planes = rd.get_frame()
    rd.close()
    assert [p.shape for p in planes] == [p.shape for p in like]
    return planes


def test_denoise_with_both_auto_flags_is_the_denoiser_with_the_reference_curve_and_strength(auto_clip):
    out = auto_clip["dir"] / "auto.y4m"
    p = _run("denoise", str(auto_clip["src"]), "-o", str(out), "--auto-prior", "--auto-strength", "--levels-min-count", str(auto_clip["nmin"]))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Denoised {auto_clip['n']} frames" in p.stderr
    assert out.read_bytes() == auto_clip["den"].read_bytes()


def test_a_prefix_of_the_clip_as_the_profile(auto_clip):
    """--profile-frames 1 with --auto-strength alone: another measurement, so other bytes, of the same length."""
    out2 = auto_clip["dir"] / "auto2.y4m"
    p = _run("denoise", str(auto_clip["src"]), "-o", str(out2), "--auto-strength", "--profile-frames", "1", "--levels-min-count", "256")
    assert p.returncode == 0, p.stderr[-2000:]
    want = auto_clip["den"].read_bytes()
    assert len(out2.read_bytes()) == len(want) and out2.read_bytes() != want


def test_a_count_no_bin_reaches_is_refused_by_the_command(auto_clip):
    """N6's refusal through `denoise --auto-prior`: one line, an error exit, nothing written."""
    out3 = auto_clip["dir"] / "auto3.y4m"
    p = _run("denoise", str(auto_clip["src"]), "-o", str(out3), "--auto-prior", "--levels-min-count", "100000000")
    assert p.returncode == 1 and "no luma bin has enough smooth samples for a prior" in p.stderr and not out3.exists()


def test_diff_with_both_auto_flags_closes_the_loop(auto_clip):
    d = auto_clip["dir"]
    auto_tbl, ref_tbl, kept = d / "auto.tbl", d / "ref.tbl", d / "kept.y4m"
    p = _run("diff", str(auto_clip["src"]), "--denoise", "-o", str(auto_tbl), "--keep-denoised", str(kept), "--auto-prior", "--auto-strength",
             "--levels-min-count", str(auto_clip["nmin"]))
    assert p.returncode == 0, p.stderr[-2000:]
    assert kept.read_bytes() == auto_clip["den"].read_bytes()
    p = _run("diff", str(auto_clip["src"]), str(auto_clip["den"]), "-o", str(ref_tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    assert auto_tbl.read_bytes() == ref_tbl.read_bytes() and auto_tbl.read_bytes().startswith(b"filmgrn1")


def test_a_job_without_the_flags_is_the_motion_entry_point(auto_clip):
    from grav1synth_amd.denoise import denoise_opts

    L = _lib.lib()
    d = auto_clip["dir"]
    src = str(auto_clip["src"]).encode()
    err = C.create_string_buffer(512)
    opts = denoise_opts(strength=3.0)
    a, b, c = d / "m.y4m", d / "a.y4m", d / "c.y4m"
    assert L.g1s_denoise_y4m_file_motion(src, str(a).encode(), C.byref(opts), 1, 0, None, 0, -1, 2, err, len(err)) == auto_clip["n"], err.value
    assert L.g1s_denoise_y4m_file_auto(src, str(b).encode(), C.byref(opts), 1, 0, None, 0, -1, 2, 0, 5, 77, err, len(err)) == auto_clip["n"], err.value
    assert a.read_bytes() == b.read_bytes()
    p = _run("denoise", str(auto_clip["src"]), "-o", str(c), "--strength", "3", "--temporal-radius", "1", "--motion-range", "2")
    assert p.returncode == 0 and c.read_bytes() == a.read_bytes()
    g = _lib.G1SOpts(C.sizeof(_lib.G1SOpts), -1, 3, 0, 0, 0)
    frames = C.c_uint64()
    ta, tb = d / "m.tbl", d / "a.tbl"
    assert L.g1s_diff_y4m_file_denoised_motion(src, str(ta).encode(), None, C.byref(g), C.byref(opts), 0, 0, None, 0, -1, 0, C.byref(frames), err, len(err)) == 0
    assert L.g1s_diff_y4m_file_denoised_auto(src, str(tb).encode(), None, C.byref(g), C.byref(opts), 0, 0, None, 0, -1, 0, 0, 0, 0, C.byref(frames), err,
                                             len(err)) == 0
    assert ta.read_bytes() == tb.read_bytes() and frames.value == auto_clip["n"]
