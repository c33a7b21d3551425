"""Noise levels (rules N1 - N8) without a device: the numpy restatement against a plain double loop and against the
estimator's oracle, the host-only entry points (g1s_nlf_sum, g1s_nlf_sigma, g1s_nlf_strength, g1s_denoise_curve_sigma,
g1s_format_noise_levels) against the restatement, the record's layout against the compiler's, the command's refusals, the
loud failure without a device, and one statistical test of the definition itself."""
from __future__ import annotations

import ctypes as C
import logging
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import denoise_curve_cases as DC
from tests import denoise_curve_ref as CR
from tests import nlf_ref as R
from tests.oracle_binding import estimate_plane_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSAMPLINGS = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "mono": (0, 0)}
NO_12 = "a grain prior needs headroom above the clip's bit depth: the stabilised domain is 12 bits, so a 12-bit clip is refused"


def smooth_planes(w, h, bd, ss, seed, amp=3):
    """[Y] or [Y, U, V]: a slope per plane with noise of up to +- amp eight-bit code values on it, so that most samples pass
    the gate and the bins differ; a fifth of the samples are wild, so that some do not."""
    rng = np.random.default_rng([seed, w, h, bd])
    subx, suby = SUBSAMPLINGS[ss]
    top = (1 << bd) - 1
    up = 1 << (bd - 8)
    shapes = [(h, w)] + ([] if ss == "mono" else [((h + suby) >> suby, (w + subx) >> subx)] * 2)
    out = []
    for c, (ph, pw) in enumerate(shapes):
        ys, xs = np.arange(ph)[:, None], np.arange(pw)[None, :]
        base = ((xs * (2 + c) + ys * (3 - c)) * up + int(rng.integers(0, top // 2))) % (top + 1)
        p = base + rng.integers(-amp * up, amp * up + 1, (ph, pw))
        wild = rng.random((ph, pw)) < 0.2
        p = np.where(wild, rng.integers(0, top + 1, (ph, pw)), p)
        out.append(np.clip(p, 0, top).astype(np.uint8 if bd == 8 else np.uint16))
    return out


def double_loop(planes, bd, xdec, ydec):
    """N1 - N4 as written, one sample at a time, in Python integers."""
    sh = bd - 8
    half = (1 << (sh - 1)) if sh else 0
    rec = {name: [[0] * 32 for _ in range(3)] for name in R.NAMES}
    H, W = planes[0].shape
    for c, plane in enumerate(planes):
        ph, pw = plane.shape
        u = [[int(v) for v in row] for row in plane]
        for y in range(1, ph - 1):
            for x in range(1, pw - 1):
                m = [[u[y - 1 + i][x - 1 + j] for j in range(3)] for i in range(3)]
                gx = (m[0][0] - m[0][2]) + (m[2][0] - m[2][2]) + 2 * (m[1][0] - m[1][2])
                gy = (m[0][0] - m[2][0]) + (m[0][2] - m[2][2]) + 2 * (m[0][1] - m[2][1])
                if (abs(gx) + abs(gy) + half) >> sh >= 50:
                    continue
                L = 4 * m[1][1] - 2 * (m[0][1] + m[2][1] + m[1][0] + m[1][2]) + (m[0][0] + m[0][2] + m[2][0] + m[2][2])
                if c == 0:
                    k = sum(sum(row) for row in m) // (9 * 2 ** (bd - 5))
                else:
                    ys, xs = y << ydec, x << xdec
                    I = int(planes[0][ys, xs])
                    if xdec:
                        I = (I + int(planes[0][ys, min(xs + 1, W - 1)]) + 1) >> 1
                    k = I >> (bd - 5)
                rec["n"][c][k] += 1
                rec["a"][c][k] += (abs(L) + half) >> sh
                rec["q"][c][k] += L * L
    return {name: np.array(rec[name], np.uint64) for name in R.NAMES}


def assert_same(a, b, what):
    for name in R.NAMES:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), f"{what}: {name}"


@pytest.mark.parametrize("ss", ["420", "444", "mono", "422"])
@pytest.mark.parametrize("size", [(1, 1), (2, 7), (7, 2), (3, 3), (4, 5), (9, 7), (13, 11), (6, 3), (33, 26)])
def test_reference_equals_a_double_loop(ss, size):
    w, h = size
    subx, suby = SUBSAMPLINGS[ss]
    for bd in (8, 10, 12):
        planes = smooth_planes(w, h, bd, ss, seed=5)
        got = R.nlf_frame(planes, bd, subx, suby)
        assert_same(got, double_loop(planes, bd, subx, suby), f"{w}x{h} {bd} bit {ss}")
        if w >= 33:
            assert got["n"][0].sum() > 0 and (ss == "mono" or got["n"][1].sum() > 0), "some samples count"
            assert got["n"][0].sum() < (w - 2) * (h - 2), "and some do not"
    rec = R.nlf_frame(smooth_planes(13, 11, 8, "mono", seed=1), 8)
    assert not rec["n"][1:].any() and not rec["q"][1:].any(), "zeros for the planes a frame lacks"


def test_the_extremes_of_one_sample():
    """A 0 / 4095 checkerboard at 12 bits: Gx = Gy = 0 and |L| = 8 x 4095 = 32760 at every interior sample, the largest there
    is (the centre and the corners against the four neighbours): five such squares leave 32 bits."""
    ys, xs = np.arange(9)[:, None], np.arange(11)[None, :]
    board = np.where((xs + ys) & 1, 4095, 0).astype(np.uint16)
    rec = R.nlf_frame([board], 12)
    assert int(rec["n"][0].sum()) == 7 * 9 and int(rec["q"][0].sum()) == 63 * 32760 ** 2 and 5 * 32760 ** 2 > 2 ** 32
    assert int(rec["a"][0].sum()) == 63 * ((32760 + 8) >> 4)
    assert_same(rec, double_loop([board], 12, 0, 0), "checkerboard")
    rng = np.random.default_rng(3)
    worst = max(abs(int(R.stencil(rng.choice([0, 4095], (3, 3)))[2][0, 0])) for _ in range(2000))
    assert worst <= 32760


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_luma_totals_are_the_estimators_sums(bd):
    """N4's identity: a / (6 n) sqrt(pi / 2) with the reference's three operations is the oracle's f64, bit for bit."""
    for seed, (w, h), amp in ((1, (64, 48), 2), (2, (37, 29), 6), (3, (5, 5), 1), (4, (40, 30), 300)):
        y = smooth_planes(w, h, bd, "mono", seed, amp)[0]
        rec = R.nlf_frame([y], bd)
        n, a = int(rec["n"][0].sum()), int(rec["a"][0].sum())
        want = estimate_plane_noise(y, bd)
        got = None if n < 16 else float(a) / float(6 * n) * R.SQRT_PI_BY_2
        assert got == want, (seed, got, want)


# ------------------------------------------------------------------------------------------------- the host-only calls
def _struct(rec):
    from grav1synth_amd.estimate import NLF_RECORD

    return R.to_struct(rec, NLF_RECORD)


def _clip_record(bd=10, ss="420", frames=3, w=96, h=80, amp=3):
    subx, suby = SUBSAMPLINGS[ss]
    return [R.nlf_frame(smooth_planes(w, h, bd, ss, seed=40 + k, amp=amp + k), bd, subx, suby) for k in range(frames)]


def test_sum_and_its_overflow():
    from grav1synth_amd.estimate import NLF_RECORD, noise_levels_sum

    recs = _clip_record()
    got = noise_levels_sum(np.array([_struct(r) for r in recs], NLF_RECORD))
    assert not R.mismatches(got, R.sum_records(recs), "total")
    assert not R.mismatches(noise_levels_sum(np.zeros(0, NLF_RECORD)), R.empty_record(), "no records")
    for name in R.NAMES:
        a, b = R.empty_record(), R.empty_record()
        a[name][2, 31] = np.uint64(2 ** 63)
        b[name][2, 31] = np.uint64(2 ** 63)
        with pytest.raises(OverflowError):
            R.sum_records([a, b])
        with pytest.raises(_lib.G1SError):
            noise_levels_sum(np.array([_struct(a), _struct(b)], NLF_RECORD))
        b[name][2, 31] = np.uint64(2 ** 63 - 1)  # the largest sum that fits is taken
        got = noise_levels_sum(np.array([_struct(a), _struct(b)], NLF_RECORD))
        assert int(got[name][2, 31]) == 2 ** 64 - 1


def _record_of(bins, bd=10):
    """A record whose luma bins are {k: (n, sigma in code values of the depth)}: q = 36 sigma^2 n."""
    rec = R.empty_record()
    for k, (n, sg) in bins.items():
        rec["n"][0, k] = n
        rec["q"][0, k] = int(round(36 * sg * sg * n))
    return rec


SIGMA_CASES = {
    "one valid bin": {7: (5000, 2.5)},
    "adjacent bins": {k: (4096 + k, 1.0 + 0.3 * k) for k in range(32)},
    "gaps between valid bins": {2: (9000, 4.0), 3: (100, 90.0), 11: (4096, 1.0), 12: (4095, 50.0), 30: (70000, 2.0)},
    "a descending pair": {5: (8000, 8.0), 6: (8000, 1.0)},
    "a bin without noise": {9: (5000, 0.0), 20: (5000, 3.0)},
    "nothing but bins without noise": {9: (5000, 0.0), 10: (6000, 0.0)},
    "the ends": {0: (5000, 1.0), 31: (5000, 7.0)},
}


@pytest.mark.parametrize("name", list(SIGMA_CASES))
@pytest.mark.parametrize("bd", [8, 10])
def test_sigma_equals_the_restatement(name, bd):
    from grav1synth_amd.estimate import noise_sigma

    rec = _record_of(SIGMA_CASES[name], bd)
    got, want = noise_sigma(_struct(rec), bd), R.sigma(rec, bd)
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert got.min() >= 1, "s lies in 1 .. 255"
    if name == "one valid bin":
        assert (got == 255).all(), "a flat s"
    if name == "nothing but bins without noise":
        assert (got == 1).all()
    if name == "a descending pair":
        c5, c6 = (5 << (bd - 5)) + (1 << (bd - 6)), (6 << (bd - 5)) + (1 << (bd - 6))
        assert got[c5] == 255 and got[c6] == 31 and (np.diff(got[c5:c6 + 1].astype(int)) <= 0).all(), "the negative numerator floors downwards"
    if name == "gaps between valid bins":
        assert got[(3 << (bd - 5)) + 1] < 255 and got[(12 << (bd - 5)) + 1] < 255, "bins below the count take no part"


def test_sigma_min_count_and_refusals():
    from grav1synth_amd.estimate import noise_sigma

    rec = _record_of({4: (300, 2.0), 9: (299, 9.0)})
    with pytest.raises(_lib.G1SError) as e:
        noise_sigma(_struct(rec), 10)  # the default, 4096
    assert "no luma bin has enough smooth samples for a prior" in str(e.value)
    with pytest.raises(ValueError):
        R.sigma(rec, 10)
    with pytest.raises(_lib.G1SError):
        noise_sigma(_struct(rec), 10, min_count=301)
    on = noise_sigma(_struct(rec), 10, min_count=300)  # on bin 4's n, one above bin 9's
    assert (on == 255).all() and np.array_equal(on, R.sigma(rec, 10, 300))
    both = noise_sigma(_struct(rec), 10, min_count=299)
    assert np.array_equal(both, R.sigma(rec, 10, 299)) and both[0] == 56 and both[-1] == 255
    # chroma bins are not luma bins
    chroma = R.empty_record()
    chroma["n"][1, 3] = chroma["q"][1, 3] = 10 ** 6
    with pytest.raises(_lib.G1SError):
        noise_sigma(_struct(chroma), 8)
    for bd, text in ((12, NO_12), (9, "a grain prior is defined for bit depths 8 and 10")):
        with pytest.raises(_lib.G1SError) as e:
            noise_sigma(_struct(_record_of({4: (5000, 2.0)})), bd)
        assert text in str(e.value)
    with pytest.raises(ValueError) as e2:
        R.sigma(rec, 12)
    assert str(e2.value) == NO_12


@pytest.mark.parametrize("name", list(SIGMA_CASES))
@pytest.mark.parametrize("bd", [8, 10])
def test_curve_from_sigma_equals_the_restatement_and_passes_the_constructors_checks(name, bd):
    from grav1synth_amd.denoise import denoise_opts
    from grav1synth_amd.estimate import noise_prior

    L = _lib.lib()
    rec = _record_of(SIGMA_CASES[name], bd)
    for rng in (0, 1, CR.max_range(bd)):
        fwd, inv = noise_prior(_struct(rec), bd, rng)
        wf, wi = R.curve_from_s(R.sigma(rec, bd), bd, rng)
        assert np.array_equal(fwd, wf) and np.array_equal(inv, wi), rng
        M = (1 << bd) - 1
        assert fwd[0] == 0 and fwd[M] == 4095 and (np.diff(fwd.astype(int)) > 0).all() and np.array_equal(inv[fwd], np.arange(M + 1))
        # g1s_denoise_new_curve checks the pair before it looks for a device
        opts = denoise_opts()
        h = L.g1s_denoise_new_curve(bd, C.byref(opts), 0, 0, fwd.ctypes.data, inv.ctypes.data)
        text = L.g1s_last_global_error().decode()
        if h:
            L.g1s_denoise_free(h)
        else:
            assert text == "no HIP device available: denoise has no CPU fallback", text


def test_curve_from_sigma_refusals():
    L = _lib.lib()
    s = np.full(4096, 9, np.uint8)
    fwd, inv = np.zeros(4096, np.uint16), np.zeros(4096, np.uint16)

    def refused(text, s_, bd, rng, f=fwd, i=inv):
        assert L.g1s_denoise_curve_sigma(None if s_ is None else s_.ctypes.data, bd, rng, None if f is None else f.ctypes.data,
                                         None if i is None else i.ctypes.data) == -1
        assert L.g1s_last_global_error().decode() == text

    refused(NO_12, s, 12, 0)
    refused("a grain prior is defined for bit depths 8 and 10", s, 9, 0)
    refused("prior range must be 1..16 at 8 bits (0 = the default)", s, 8, 17)
    refused("prior range must be 1..4 at 10 bits (0 = the default)", s, 10, 5)
    refused("a curve needs the scaling function it is made from", None, 10, 0)
    refused("g1s_denoise_curve_sigma needs both output tables", s, 10, 0, None)
    refused("g1s_denoise_curve_sigma needs both output tables", s, 10, 0, fwd, None)


@pytest.mark.parametrize("curve", DC.CURVES)
@pytest.mark.parametrize("bd", [8, 10])
def test_the_curve_of_a_table_is_what_it_was(curve, bd):
    """g1s_denoise_curve on the priors of tests/denoise_curve_cases.py: the restatement's bytes (as before the builder was
    split), and the same bytes from the two halves: s from the segments, the curve from s."""
    from grav1synth_amd.denoise import grain_curve
    from tests.test_denoise_curve_cpu import segment

    L = _lib.lib()
    points, rng = DC.curve_points(curve)
    rng = CR.max_range(bd) if rng < 0 else rng
    fwd, inv = grain_curve([segment(p) for p in points], bd, rng)
    wf, wi = CR.curve(points, bd, rng)
    assert np.array_equal(fwd, wf) and np.array_equal(inv, wi)
    s = CR.scaling(points, bd)
    assert s.max() <= 255
    s8 = np.ascontiguousarray(s, np.uint8)
    f2, i2 = np.zeros(1 << bd, np.uint16), np.zeros(4096, np.uint16)
    assert L.g1s_denoise_curve_sigma(s8.ctypes.data, bd, rng, f2.ctypes.data, i2.ctypes.data) == 0
    assert np.array_equal(f2, wf) and np.array_equal(i2, wi)
    rf, ri = R.curve_from_s(s, bd, rng)
    assert np.array_equal(rf, wf) and np.array_equal(ri, wi), "the two restatements agree"


def test_strength_and_its_refusals():
    from grav1synth_amd.estimate import auto_strength

    L = _lib.lib()
    for bd in (8, 10, 12):
        for recs in (_clip_record(bd, "420"), _clip_record(bd, "mono", amp=9), _clip_record(bd, "444", amp=1)):
            total = R.sum_records(recs)
            hl, hc = auto_strength(_struct(total), bd, 256)
            assert hl == R.strength(total, bd, 256, 0) and hc == R.strength(total, bd, 256, 1)
            assert hl is not None and (hc is None) == (not total["n"][1:].any())
    # white noise of sigma = 3 ten-bit code values: h = sqrt(2) x 3 / 4
    rec = _record_of({k: (1000, 3.0) for k in range(8)}, 10)
    assert auto_strength(_struct(rec), 10)[0] == math.sqrt(2.0 * 9.0) / 4.0
    h = C.c_double(-1.0)

    def refused(text, rec_, bd, min_count, cls):
        assert L.g1s_nlf_strength(_struct(rec_).ctypes.data, bd, min_count, cls, C.byref(h)) == -1 and h.value == -1.0
        assert L.g1s_last_global_error().decode() == text

    refused("too few smooth samples for a strength", _record_of({3: (4095, 2.0)}), 10, 0, 0)
    refused("too few smooth samples for a strength", _record_of({3: (500, 2.0)}), 10, 501, 0)
    refused("too few smooth samples for a strength", _record_of({3: (5000, 2.0)}), 10, 0, 1)
    refused("the measured strength is outside 0 < h <= 1000", _record_of({3: (5000, 0.0)}), 10, 0, 0)
    refused("the measured strength is outside 0 < h <= 1000", _record_of({3: (5000, 800.0)}), 8, 0, 0)
    refused("noise levels are defined for bit depths 8, 10 and 12", _record_of({3: (5000, 2.0)}), 9, 0, 0)
    refused("plane_class is 0 (luma) or 1 (chroma)", _record_of({3: (5000, 2.0)}), 10, 0, 2)
    assert L.g1s_nlf_strength(_struct(_record_of({3: (500, 2.0)})).ctypes.data, 10, 500, 0, C.byref(h)) == 0 and h.value > 0
    with pytest.raises(_lib.G1SError) as e:
        auto_strength(_struct(R.empty_record()), 10)
    assert "too few smooth samples" in str(e.value)


def test_the_report_byte_for_byte():
    from grav1synth_amd.estimate import format_noise_levels

    for bd, ss in ((10, "420"), (8, "mono"), (12, "444"), (8, "422")):
        nplanes = 1 if ss == "mono" else 3
        total = R.sum_records(_clip_record(bd, ss))
        for min_count in (0, 256, 10 ** 9):
            text = format_noise_levels(_struct(total), 3, bd, nplanes, min_count)
            assert text == R.format_noise_levels(total, 3, bd, nplanes, min_count), text.decode()
        assert text.startswith(b"noiselevels1\nframes 3 bit_depth %d planes %d\nplane 0\nbin " % (bd, nplanes))
        assert text.endswith(b"auto_strength - -\n")
        fine = format_noise_levels(_struct(total), 3, bd, nplanes, 256).splitlines()[-1].split()
        assert fine[0] == b"auto_strength" and fine[1] != b"-" and (fine[2] == b"-") == (ss == "mono")
        assert text.count(b"plane_sigma ") == nplanes
    # a record without a counting sample, and a capacity one byte short
    empty = format_noise_levels(_struct(R.empty_record()), 0, 8, 1)
    assert empty == b"noiselevels1\nframes 0 bit_depth 8 planes 1\nplane 0\nplane_sigma -\nauto_strength - -\n"
    assert format_noise_levels(_struct(R.empty_record()), 0, 8, 1, cap=len(empty)) == empty
    with pytest.raises(_lib.G1SError) as e:
        format_noise_levels(_struct(R.empty_record()), 0, 8, 1, cap=len(empty) - 1)
    assert e.value.code == _lib.G1S_ERR_CAPACITY
    for bd, nplanes in ((9, 1), (8, 2), (8, 0)):
        with pytest.raises(_lib.G1SError) as e:
            format_noise_levels(_struct(R.empty_record()), 0, bd, nplanes)
        assert e.value.code == -1


def test_the_host_only_half_builds_with_a_host_compiler_and_has_the_headers_layout(tmp_path):
    from grav1synth_amd.estimate import NLF_RECORD

    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "nlf_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tests", "nlf_host.cpp")]
    # (the sanitizer's runtime inside the program where the compiler can do that: it then starts under any preloaded library)
    if subprocess.call(cmd + ["-static-libasan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok"
    size, off_n, off_a, off_q, opts_size, off_batch = (int(v) for v in lines[0].split())
    assert size == C.sizeof(_lib.G1SNlfRecord) == NLF_RECORD.itemsize == 8 * 3 * 96
    for f, off in zip(R.NAMES, (off_n, off_a, off_q)):
        assert off == getattr(_lib.G1SNlfRecord, f).offset == NLF_RECORD.fields[f][1], f
    assert opts_size == C.sizeof(_lib.G1SNlfOpts) and off_batch == _lib.G1SNlfOpts.batch_frames.offset


def test_no_gpu_means_the_meter_refuses():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from grav1synth_amd.estimate import NoiseLevelMeter

    L = _lib.lib()
    assert not L.g1s_nlf_new(10, None)
    assert L.g1s_last_global_error().decode() == "no HIP device available: noise levels has no CPU fallback"
    with pytest.raises(_lib.G1SError) as e:
        NoiseLevelMeter(10)
    assert "noise levels has no CPU fallback" in str(e.value)


def test_bad_bit_depth_and_options_are_refused_before_a_device_is_looked_for():
    L = _lib.lib()
    assert not L.g1s_nlf_new(9, None)
    assert L.g1s_last_global_error().decode() == "noise levels are defined for bit depths 8, 10 and 12"
    bad = _lib.G1SNlfOpts(4, -1, 0)
    assert not L.g1s_nlf_new(10, C.byref(bad))
    assert "struct_size" in L.g1s_last_global_error().decode()


def test_estimate_levels_refuses_like_the_other_outputs(tmp_path, caplog, monkeypatch):
    from grav1synth_amd import cli, estimate

    a, out, lev = (str(tmp_path / n) for n in ("a.y4m", "out.txt", "levels.txt"))
    open(a, "wb").write(b"x")

    def one_line(text, call):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="grav1synth"):
            assert call() == -1
        got = [r.getMessage() for r in caplog.records]
        assert got == [text], got

    one_line(cli.SAME_AS_OUTPUT, lambda: cli.estimate_command(a, out, levels=a))
    one_line(cli.SAME_AS_OUTPUT, lambda: cli.estimate_command(a, out, levels=str(tmp_path) + "//a.y4m"))
    one_line(cli.SAME_LEVELS, lambda: cli.estimate_command(a, out, levels=out))
    open(lev, "wb").write(b"kept")
    one_line(cli.NOT_OVERWRITING, lambda: cli.estimate_command(a, out, levels=lev, confirm=lambda *_: False))
    assert open(lev, "rb").read() == b"kept" and not os.path.exists(out)
    # the wiring: --levels reaches estimate_y4m_file, and without it the call is the one it was
    seen = []
    monkeypatch.setattr(estimate, "estimate_y4m_file", lambda s, o, **kw: seen.append(kw) or 2)
    assert cli.main(["estimate", a, "-o", out, "--levels", lev, "-y"]) == 0 and seen[-1] == dict(device=-1, levels=lev)
    assert cli.main(["estimate", a, "-o", out, "-y", "--device", "1"]) == 0 and seen[-1] == dict(device=1, levels=None)
    args = cli.build_parser().parse_args(["estimate", a, "-o", out])
    assert args.levels is None


def test_the_auto_flags_refuse_with_one_logged_line(tmp_path, caplog):
    from grav1synth_amd import cli

    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
    src12 = tmp_path / "a12.y4m"
    src12.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono12\nFRAME\n" + bytes(16))
    pipe = tmp_path / "pipe.y4m"
    os.mkfifo(pipe)
    example = os.path.join(ROOT, "tests", "golden", "reference-example-table.tbl")
    out, tbl = tmp_path / "o.y4m", tmp_path / "t.tbl"

    def one_line(text, call):
        caplog.clear()
        with caplog.at_level("INFO", logger="grav1synth"):
            assert call() == -1
        got = [r.getMessage() for r in caplog.records]
        assert got == [text], got

    dn = lambda src_, **kw: cli.denoise_command(str(src_), str(out), **kw)  # noqa: E731
    df = lambda src_, **kw: cli.diff_command(str(src_), None, str(tbl), denoise=True, **kw)  # noqa: E731
    for run in (dn, df):
        one_line(cli.AUTO_PRIOR_AND_TABLE, lambda: run(src, auto_prior=True, grain_prior=example))
        one_line(cli.AUTO_STRENGTH_AND_STRENGTH, lambda: run(src, auto_strength=True, strength=3.0))
        one_line(cli.AUTO_STRENGTH_AND_STRENGTH, lambda: run(src, auto_strength=True, auto_prior=True, chroma_strength=2.0))
        one_line(cli.AUTO_NEEDS_FLAG, lambda: run(src, profile_frames=3))
        one_line(cli.AUTO_NEEDS_FLAG, lambda: run(src, levels_min_count=100))
        one_line(cli.AUTO_BAD_NUMBER, lambda: run(src, auto_prior=True, profile_frames=-1))
        one_line(cli.AUTO_BAD_NUMBER, lambda: run(src, auto_strength=True, levels_min_count=-5))
        one_line(cli.AUTO_NEEDS_FILE % pipe, lambda: run(pipe, auto_strength=True))
        one_line(cli.PRIOR_12_BIT.replace("--grain-prior", "--auto-prior"), lambda: run(src12, auto_prior=True))
    assert not out.exists() and not tbl.exists()
    # through main(): a logged line and a normal exit; and the wiring of the four arguments
    assert cli.main(["denoise", str(src), "-o", str(out), "--auto-prior", "--grain-prior", example]) == 0 and not out.exists()
    a = cli.build_parser().parse_args(["diff", "s.y4m", "--denoise", "-o", "t.tbl", "--auto-prior", "--auto-strength", "--profile-frames", "8",
                                       "--levels-min-count", "256"])
    got = cli._denoise_parameters(a)
    assert (got["auto_prior"], got["auto_strength"], got["profile_frames"], got["levels_min_count"]) == (True, True, 8, 256)
    a = cli.build_parser().parse_args(["denoise", "in.y4m", "-o", "out.y4m"])
    got = cli._denoise_parameters(a)
    assert (got["auto_prior"], got["auto_strength"], got["profile_frames"], got["levels_min_count"]) == (False, False, 0, 0)


def test_the_auto_file_calls_refuse_before_they_look_for_a_device(tmp_path):
    from grav1synth_amd.denoise import denoise_opts

    L = _lib.lib()
    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
    pipe = tmp_path / "pipe.y4m"
    os.mkfifo(pipe)
    example = os.path.join(ROOT, "tests", "golden", "reference-example-table.tbl").encode()
    out, tbl = str(tmp_path / "o.y4m").encode(), str(tmp_path / "t.tbl").encode()
    err = C.create_string_buffer(512)
    frames = C.c_uint64(7)

    def both(text, source, opts, prior, auto):
        assert L.g1s_denoise_y4m_file_auto(str(source).encode(), out, C.byref(opts), 0, 0, prior, 0, -1, 0, auto, 0, 0, err, len(err)) == -1
        assert err.value.decode() == text, err.value
        g = _lib.G1SOpts(C.sizeof(_lib.G1SOpts), -1, 3, 0, 0, 0)
        assert L.g1s_diff_y4m_file_denoised_auto(str(source).encode(), tbl, None, C.byref(g), C.byref(opts), 0, 0, prior, 0, -1, 0, auto, 0, 0,
                                                 C.byref(frames), err, len(err)) == -1
        assert err.value.decode() == text and frames.value == 0, err.value

    both("unknown auto flags", src, denoise_opts(), None, 4)
    both("an auto prior does not combine with a grain prior table", src, denoise_opts(), example, _lib.G1S_AUTO_PRIOR)
    both("an auto strength does not combine with a given strength", src, denoise_opts(strength=2.0), None, _lib.G1S_AUTO_STRENGTH)
    both("an auto strength does not combine with a given strength", src, denoise_opts(chroma_strength=2.0), None, 3)
    both(f"{pipe} cannot be read twice (not a regular file): the auto flags need a pre-pass", pipe, denoise_opts(), None, _lib.G1S_AUTO_STRENGTH)
    assert not os.path.exists(out) and not os.path.exists(tbl)


# -------------------------------------------------------------------------------------- the definition, statistically
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("sigma0", [1, 2, 4])
def test_the_definition_recovers_signal_dependent_noise(bd, sigma0):
    """Reference only.  A 512 x 1024 ramp from 0.1 to 0.9 of full scale with Gaussian noise of sigma(v) = sigma0 (0.5 + v / M)
    eight-bit code values, rounded and clipped: sqrt(q / (36 n)) of bins 6, 16 and 26 within 5 % of sqrt(sigma^2 + 1/12) (the
    rounding's variance beside the noise's), each from at least 8 000 counting samples."""
    h, w = 512, 1024
    M = (1 << bd) - 1
    up = 1 << (bd - 8)
    rng = np.random.default_rng([77, bd, sigma0])
    v = np.broadcast_to(np.linspace(0.1 * M, 0.9 * M, w)[None, :], (h, w))
    sg = sigma0 * up * (0.5 + v / M)
    y = np.clip(np.rint(v + rng.standard_normal((h, w)) * sg), 0, M).astype(np.uint8 if bd == 8 else np.uint16)
    rec = R.nlf_frame([y], bd)
    for k in (6, 16, 26):
        n, q = int(rec["n"][0, k]), int(rec["q"][0, k])
        centre = (k << (bd - 5)) + (1 << (bd - 6))
        truth = math.sqrt((sigma0 * up * (0.5 + centre / M)) ** 2 + 1.0 / 12.0)
        got = math.sqrt(q / (36 * n))
        print(f"{bd} bit sigma0 {sigma0} bin {k}: n {n} sigma {got:.4f} truth {truth:.4f} ratio {got / truth:.4f}")
        assert n >= 8000, (k, n)
        assert abs(got / truth - 1.0) <= 0.05, (k, got, truth)
