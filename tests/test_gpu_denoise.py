"""`denoise` on the device against tests/denoise_ref.py, byte for byte; the commands; the closed loop with the estimator."""
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
from tests import denoise_ref as R
from tests.test_gpu_grain import SUBSAMPLINGS, _to_dev, assert_planes_equal, make_segment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference(planes, bd, A=3, S=2, strength=4.0, chroma_strength=None):
    from grav1synth_amd.denoise import weight_table

    luma = weight_table(bd, S, strength)
    chroma = weight_table(bd, S, strength if chroma_strength is None else chroma_strength)
    return R.denoise_frame([np.asarray(p) for p in planes], A, S, luma, chroma)


def gradient(w, h, bd, subx, suby, seed=0, mono=False, amp=5):
    """Gradients with noise: planes of any size, chroma rounded up as the library does."""
    rng = np.random.default_rng([seed, w, h, bd])
    top = (1 << bd) - 1
    shapes = [(h, w)] + ([] if mono else [((h + suby) >> suby, (w + subx) >> subx)] * 2)
    out = []
    for i, (ph, pw) in enumerate(shapes):
        base = ((np.arange(pw)[None, :] * (3 + i) + np.arange(ph)[:, None] * (2 + i)) << (bd - 8)) % (top + 1)
        p = np.clip(base + rng.integers(-(amp << (bd - 8)), (amp << (bd - 8)) + 1, (ph, pw)), 0, top)
        out.append(p.astype(np.uint8 if bd == 8 else np.uint16))
    return out


@pytest.fixture(scope="module")
def denoisers():
    from grav1synth_amd.denoise import Denoiser

    made = {}

    def get(bd, **kw):
        key = (bd, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = Denoiser(bd, **kw)
        return made[key]

    yield get
    for d in made.values():
        d.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
def test_grainy_content_equals_the_reference(denoisers, bd, ss):
    """The asymmetric content family with rendered grain on it."""
    from grav1synth_amd.grain import GrainSynthesizer

    mono = ss == "mono"
    subx, suby = (1, 1) if mono else SUBSAMPLINGS[ss]
    w, h = 208, 136
    _src, den = CT.make_frames("distinct", w, h, bd, subx, suby, frame=2)
    syn = GrainSynthesizer(bd)
    grainy = syn.apply(den, make_segment(3, 40 + bd), subx, suby)
    syn.close()
    planes = grainy[:1] if mono else grainy
    got = denoisers(bd).apply(_to_dev(planes, bd), subx, suby)
    want = reference(planes, bd)
    assert any((a != b).any() for a, b in zip(want, planes)), "the filter did something"
    assert_planes_equal(got, want, f"{bd} bit {ss}")


SIZES = [(1, 1), (5, 3), (3, 7), (63, 47), (64, 48), (65, 49), (131, 97), (2, 210), (300, 2), (129, 5)]


@pytest.mark.parametrize("size", SIZES)
def test_sizes_off_the_tile_and_smaller_than_the_search_window(denoisers, size):
    w, h = size
    for bd, ss in ((8, "420"), (10, "422"), (12, "444")):
        subx, suby = SUBSAMPLINGS[ss]
        planes = gradient(w, h, bd, subx, suby, seed=1)
        assert_planes_equal(denoisers(bd).apply(_to_dev(planes, bd), subx, suby), reference(planes, bd), f"{w}x{h} {bd} bit {ss}")


def test_full_range_content(denoisers):
    for bd in (8, 12):
        top = (1 << bd) - 1
        dt = np.uint8 if bd == 8 else np.uint16
        shapes = [(101, 150), (51, 75), (51, 75)]
        zero = [np.zeros(s, dt) for s in shapes]
        assert_planes_equal(denoisers(bd).apply(_to_dev(zero, bd)), zero, "all zero")
        chk = [(((np.arange(s[0])[:, None] + np.arange(s[1])[None, :]) & 1) * top).astype(dt) for s in shapes]
        assert_planes_equal(denoisers(bd).apply(_to_dev(chk, bd)), reference(chk, bd), "checkerboard")
        noise = [np.random.default_rng(c).integers(0, top + 1, s).astype(dt) for c, s in enumerate(shapes)]
        assert_planes_equal(denoisers(bd, strength=60.0).apply(_to_dev(noise, bd)), reference(noise, bd, strength=60.0), "full-range noise")
    # the uint32 ceiling of rule 4: all-max at 12 bit, A = 7, every weight 4096
    full = [np.full((90, 100), 4095, np.uint16)]
    kw = dict(search_radius=7, patch_radius=4, strength=1000.0)
    got = denoisers(12, **kw).apply(_to_dev(full, 12))
    assert_planes_equal(got, full, "all max")
    assert_planes_equal(got, reference(full, 12, 7, 4, 1000.0), "all max against the reference")


@pytest.mark.parametrize("A,S", [(1, 1), (1, 4), (7, 1), (7, 4), (7, 3), (4, 3), (2, 2)])
def test_parameter_corners(denoisers, A, S):
    from grav1synth_amd.denoise import weight_table

    bd, (subx, suby) = 10, (1, 1)
    planes = gradient(150, 101, bd, subx, suby, seed=A * 10 + S, amp=6)
    for strength, chroma in ((0.05, 0.05), (6.0, 2.5), (300.0, 40.0)):
        q = weight_table(bd, S, strength)[1]
        assert (q == 0) == (strength == 0.05) and (strength != 300.0 or q >= 10)
        d = denoisers(bd, search_radius=A, patch_radius=S, strength=strength, chroma_strength=chroma)
        assert_planes_equal(d.apply(_to_dev(planes, bd), subx, suby), reference(planes, bd, A, S, strength, chroma), f"A {A} S {S} h {strength}")


def test_refusals_on_the_device():
    from grav1synth_amd.denoise import Denoiser

    for kw in (dict(search_radius=8), dict(patch_radius=5), dict(strength=-1.0)):
        with pytest.raises(_lib.G1SError):
            Denoiser(10, **kw)
    with pytest.raises(_lib.G1SError) as e:
        Denoiser(9)
    assert "8, 10 and 12" in str(e.value)
    own = Denoiser(10)
    dev = _to_dev(gradient(64, 40, 10, 1, 1), 10)
    with pytest.raises(_lib.G1SError) as e:
        own.apply(dev, out=dev)
    assert "distinct" in str(e.value)
    with pytest.raises(_lib.G1SError):  # sticky
        own.apply(dev)
    own.close()
    other = Denoiser(8)
    with pytest.raises(_lib.G1SError) as e:
        other.apply(dev)
    assert "bytes_per_sample" in str(e.value)
    other.close()


def test_strided_device_tensors_and_host_pinned_device_frames_agree(denoisers):
    import torch

    from grav1synth_amd.diff import Frame

    bd, (subx, suby) = 10, (1, 1)
    planes = gradient(163, 99, bd, subx, suby, seed=5)
    want = reference(planes, bd)
    dn = denoisers(bd)
    strided_in, strided_out, out_bases = [], [], []
    for p in planes:  # rows wider than the plane, starting off a 16-byte boundary
        big = np.zeros((p.shape[0], p.shape[1] + 13), np.uint16)
        big[:, 3:3 + p.shape[1]] = p
        strided_in.append(torch.from_numpy(big).to("cuda")[:, 3:3 + p.shape[1]])
        obig = torch.from_numpy(np.full((p.shape[0], p.shape[1] + 9), 0xABCD, np.uint16)).to("cuda")
        out_bases.append(obig)
        strided_out.append(obig[:, 5:5 + p.shape[1]])
    got = dn.apply(strided_in, subx, suby, out=strided_out)
    assert_planes_equal(got, want, "strided device tensors")
    for o, base in zip(strided_out, out_bases):  # nothing written outside the plane's columns
        full = base.cpu().numpy()
        assert (full[:, :5] == 0xABCD).all() and (full[:, 5 + o.shape[1]:] == 0xABCD).all()
    host = dn.apply(planes, subx, suby)
    assert all(isinstance(p, np.ndarray) for p in host)
    assert_planes_equal(host, want, "host frames")
    L = _lib.lib()
    pin_in = [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
    pin_out = [torch.from_numpy(np.zeros(p.shape, np.uint16)).pin_memory() for p in planes]
    keep = []
    fin = Frame(pin_in, subx, suby, async_host=True).to_c(keep)
    fout = Frame(pin_out, subx, suby, async_host=True).to_c(keep)
    assert fin.on_device == 2 and fout.on_device == 2
    assert L.g1s_denoise_frame(dn._h, C.byref(fin), C.byref(fout)) == 0
    dn.sync()
    assert_planes_equal([p.numpy() for p in pin_out], want, "pinned frames")


def test_a_batch_of_70_frames_equals_70_single_calls_and_a_geometry_change_drains(denoisers):
    from grav1synth_amd.denoise import Denoiser

    bd, (subx, suby) = 8, (1, 1)
    batched = Denoiser(bd, batch_frames=32)
    single = denoisers(bd)
    outs, wants, ins = [], [], []
    for k in range(70):
        planes = gradient(130, 70, bd, subx, suby, seed=k)
        dev = _to_dev(planes, bd)
        ins.append(dev)
        outs.append(batched.apply(dev, subx, suby, sync=False))
        wants.append(single.apply(dev, subx, suby))
        if k in (0, 33, 69):
            assert_planes_equal(wants[-1], reference(planes, bd), f"frame {k}")
    # 6 frames are still queued: another geometry sends them out first, host frames included
    small = gradient(70, 50, bd, 0, 0, seed=99)
    small_out = batched.apply(small, 0, 0, sync=False)
    batched.sync()
    for k in range(70):
        assert_planes_equal(outs[k], [p.cpu().numpy() for p in wants[k]], f"batched frame {k}")
    assert_planes_equal(small_out, reference(small, bd), "the frame after the geometry change")
    batched.close()


def test_4k_10_bit(denoisers):
    from grav1synth_amd.grain import GrainSynthesizer

    bd, (subx, suby) = 10, (1, 1)
    _src, den = CT.make_frames("busy", 3840, 2160, bd, subx, suby, frame=0)
    syn = GrainSynthesizer(bd)
    grainy = syn.apply(den, make_segment(3, 77), subx, suby)
    syn.close()
    assert_planes_equal(denoisers(bd).apply(_to_dev(grainy, bd), subx, suby), reference(grainy, bd), "4K")


def _clip(tmp_path, n=26):
    """A source clip with a scene cut in the middle (twice the noise gain from there on)."""
    from grav1synth_amd.ingest import write_y4m
    from grav1synth_amd.synth import SynthSpec, make_pair

    a, b = SynthSpec(320, 192, 8), SynthSpec(320, 192, 8, gain_scale=2)
    frames = []
    for k in range(n):
        s, _ = make_pair(a if k < n // 2 else b, k, device="cpu")
        frames.append([p.numpy() for p in s])
    src = tmp_path / "src.y4m"
    write_y4m(str(src), frames, 8, 1, 1, Fraction(24, 1))
    return src, frames


def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "grav1synth_amd", *args], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT,
                          stdin=subprocess.DEVNULL)


def test_the_commands_end_to_end(tmp_path):
    from grav1synth_amd.ingest import Y4MReader, diff_y4m_file_denoised
    from grav1synth_amd.tbl import parse_tbl

    src, frames = _clip(tmp_path)
    # `denoise`
    out = tmp_path / "den_cmd.y4m"
    p = _run("denoise", str(src), "-o", str(out), "--strength", "5")
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Denoised {len(frames)} frames" in p.stderr and f"Done, wrote output file to {out}" in p.stderr
    assert open(out, "rb").readline() == open(src, "rb").readline(), "the output's header is the input's"
    rd = Y4MReader(str(out))
    for k, planes in enumerate(frames):
        got = rd.get_frame()
        if k % 6 == 0 or k == len(frames) - 1:
            assert_planes_equal([np.asarray(q) for q in got], reference(planes, 8, strength=5.0), f"frame {k}")
    assert rd.get_frame() is None
    rd.close()
    # `diff --denoise --keep-denoised` = `denoise` + `diff` with two files, to the byte
    a_tbl, den, b_tbl = tmp_path / "a.tbl", tmp_path / "den.y4m", tmp_path / "b.tbl"
    p = _run("diff", str(src), "--denoise", "-o", str(a_tbl), "--keep-denoised", str(den), "--strength", "5")
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Computed diff for {len(frames)} frames" in p.stderr and f"Done, wrote output file to {a_tbl}" in p.stderr
    assert den.read_bytes() == out.read_bytes(), "--keep-denoised writes what `denoise` writes"
    p = _run("diff", str(src), str(den), "-o", str(b_tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    assert a_tbl.read_bytes() == b_tbl.read_bytes()
    assert len(parse_tbl(a_tbl.read_bytes())) >= 2, "the content change did not cut the table"
    # small launch groups on both sides: several groups, and more frames than the first ring of buffer pairs holds
    c_tbl, den2 = tmp_path / "c.tbl", tmp_path / "den2.y4m"
    assert diff_y4m_file_denoised(str(src), str(c_tbl), keep_denoised=str(den2), batch_frames=2, denoise_batch_frames=3, strength=5.0) == len(frames)
    assert c_tbl.read_bytes() == b_tbl.read_bytes() and den2.read_bytes() == out.read_bytes()
    # refusals of the commands: same path; an existing output without -y (no terminal: an error exit, as diff's)
    before = out.read_bytes()
    p = _run("denoise", str(src), "-o", str(src))
    assert p.returncode == 0 and "Input and output paths are the same" in p.stderr
    p = _run("denoise", str(src), "-o", str(out))
    assert p.returncode == 1 and "not a terminal" in p.stderr and out.read_bytes() == before
    p = _run("denoise", str(src), "-o", str(tmp_path / "never.y4m"), "--search-radius", "9")
    assert p.returncode == 1 and "search_radius must be 1..7" in p.stderr


# The closed loop through the denoiser, observed on an MI355X (largest luma AR coefficient error; smallest .. largest ratio
# of recovered to true noise strength over the luma range, per emitted segment):
#   A = 5, S = 2, h = 10 (LOOP)   0.055 .. 0.063   0.875 .. 1.037
#   A = 7, S = 2, h = 10          0.043 .. 0.063   0.888 .. 1.051
#   A = 5, S = 2, h = 16          0.043 .. 0.063   0.923 .. 1.081
#   A = 7, S = 3, h = 24          0.043 .. 0.078   0.951 .. 1.108
#   A = 3, S = 2, h = 4 (default) 0.305 .. 0.387   0.093 .. 0.369   <- too weak for this grain (sigma 6 .. 8 code values
#                                                                      at 8 bit): most of it stays in the "denoised" clip
# With the true clean frames (test_closed_loop_on_the_device) the bounds are 0.086 and 20 %.  The bounds below leave margin.
DENOISED_AR_BOUND = 0.09
DENOISED_STD_LOW, DENOISED_STD_HIGH = 0.80, 1.10
LOOP = dict(search_radius=5, patch_radius=2, strength=10.0)


def closed_loop(parameters=LOOP, frames=6):
    """(largest luma AR coefficient error, smallest and largest ratio of recovered to true noise strength) per emitted segment,
    from (grainy, Denoiser(grainy)); everything on the device."""
    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.diff import DiffGenerator
    from grav1synth_amd.grain import GrainSynthesizer
    from tests import grain_ref as G
    from tests.test_grain_cpu import CY3, segment, smooth_frame

    bd, (subx, suby), lag, cy = 10, (1, 1), 3, CY3
    pts_y, pts_c = [(0, 30), (64, 50), (128, 60), (192, 50), (255, 70)], [(0, 30), (255, 60)]
    cc = [c // 2 for c in cy] + [40]
    clean = _to_dev(smooth_frame(640, 384, bd, subx, suby), bd)
    syn, dn = GrainSynthesizer(bd), Denoiser(bd, **parameters)
    differ = DiffGenerator(Fraction(24, 1), bd, bd, ar_coeff_lag=lag, device=0)
    for k in range(frames):
        seg = segment(lag, cy, cc, pts_y, pts_c, (7391 + 10956 * (k + 1)) & 0xFFFF)
        grainy = syn.apply(clean, seg, subx, suby)
        differ.diff_frame(grainy, dn.apply(grainy, subx, suby), subx, suby)
    emitted = differ.finish()
    syn.close()
    dn.close()
    assert emitted
    n = 2 * lag * (lag + 1)
    want = np.array(cy) / 2.0 ** 7
    xs = np.arange(40, 200, 16)
    true_std = G.scaling_lut(pts_y)[xs] / 2.0 ** 8 * G.generate_grain(seg, bd, subx, suby, mono=True)[0][9:, 9:].std()
    seen = []
    for e in emitted:
        got = np.array(e.ar_coeffs_y[:n]) / 2.0 ** e.ar_coeff_shift
        back = segment(lag, list(e.ar_coeffs_y[:n]), list(e.ar_coeffs_y[:n]) + [0], e.scaling_points_y, [], 1,
                       scaling_shift=e.scaling_shift, ar_shift=e.ar_coeff_shift)
        est_std = G.scaling_lut(e.scaling_points_y)[xs] / 2.0 ** e.scaling_shift * G.generate_grain(back, bd, subx, suby, mono=True)[0][9:, 9:].std()
        ratio = est_std / true_std
        seen.append((float(np.abs(got - want).max()), float(ratio.min()), float(ratio.max())))
    return seen


def test_closed_loop_through_the_denoiser():
    """GrainSynthesizer -> Denoiser -> DiffGenerator on (grainy, denoised): the estimator's reason for wanting a denoiser.
    test_closed_loop_on_the_device (tests/test_gpu_grain.py) does the same with the TRUE clean frames as the second
    input and gets the luma AR coefficients within 0.086 and the noise strength within 20 %.  A denoiser leaves part of
    the grain in, so from its output the strength comes back low: observed at LOOP's parameters, AR coefficients within
    0.063, strength 0.875 .. 1.037 of the true one (the table above DENOISED_AR_BOUND has the other settings tried, the
    default strength among them, which is too weak for this grain)."""
    for ar_err, lo, hi in closed_loop():
        assert ar_err <= DENOISED_AR_BOUND, (ar_err, lo, hi)
        assert DENOISED_STD_LOW <= lo and hi <= DENOISED_STD_HIGH, (ar_err, lo, hi)
