"""The scale record of `measure` without a device: tests/measure_s_ref.py against a plain loop over boxes and its exact
identities, designed content on which every rule bites, the host-only entry points (g1s_measure_sum_scales,
g1s_format_measure_scales) against the restatement byte for byte, the record's layout against the C compiler's, rule 21's
predicate, the refusals of g1s_measure_new_scales and of the commands, and two statistical tests of the definition."""
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
from tests import measure_ref as R
from tests import measure_s_ref as S
from tests.test_measure_cpu import SUBSAMPLINGS, planes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 3), (5, 5), (9, 7), (13, 10), (37, 35), (64, 33)]  # luma; the odd ones make rule 2's clamp take part


def shapes_of(w, h, ss):
    subx, suby = SUBSAMPLINGS[ss]
    return [(h, w)] + ([] if ss == "mono" else [((h + suby) >> suby, (w + subx) >> subx)] * 2)


def dtype_of(bd):
    return np.uint8 if bd == 8 else np.uint16


def box_loop(noisy, clean, bd, xdec, ydec):
    """Rules 18 - 20 as written: one plane, one scale, one box and one sample at a time, in Python integers."""
    rec = S.empty_record()
    H, W = clean[0].shape
    for c in range(len(clean)):
        ph, pw = clean[c].shape
        for k in range(1, 6):
            L = 1 << k
            for j in range(ph >> k):
                for i in range(pw >> k):
                    B = Csum = 0
                    for y in range(j * L, j * L + L):
                        for x in range(i * L, i * L + L):
                            B += int(noisy[c][y, x]) - int(clean[c][y, x])
                            if c == 0:
                                Csum += int(clean[0][y, x])
                            else:
                                ys, xs = y << ydec, x << xdec
                                I = int(clean[0][ys, xs])
                                if xdec:
                                    I = (I + int(clean[0][ys, min(xs + 1, W - 1)]) + 1) >> 1
                                Csum += I
                    K = min(Csum >> (2 * k + bd - 5), 31)
                    rec["n"][c, k - 1, K] += np.uint64(1)
                    rec["s1"][c, k - 1, K] += B
                    rec["s2"][c, k - 1, K] += np.uint64(B * B)
    return rec


def assert_same(a, b, what):
    for name, _dt in S.FIELDS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), f"{what}: {name}"


@pytest.mark.parametrize("ss", ["420", "422", "444"])
@pytest.mark.parametrize("size", SIZES)
def test_restatement_equals_a_plain_loop_over_boxes(ss, size):
    w, h = size
    subx, suby = SUBSAMPLINGS[ss]
    for bd in (8, 10, 12):
        noisy, clean = planes_of(w, h, bd, ss, seed=5)
        assert_same(S.scale_frame(noisy, clean, bd, subx, suby), box_loop(noisy, clean, bd, subx, suby), f"{w}x{h} {bd} bit {ss}")
    mono = planes_of(w, h, 8, "mono", seed=5)
    got = S.scale_frame(mono[0], mono[1], 8, 0, 0)
    assert_same(got, box_loop(mono[0], mono[1], 8, 0, 0), "one plane")
    assert not got["n"][1:].any(), "the planes a frame does not have are zeros"


# ---- designed content (the GPU tests use the same) ----

def checkerboard_pair(w, h, bd, ss, m, amp):
    """d = +amp / -amp on a checkerboard of 2^m x 2^m cells, on every plane; the clean planes are flat."""
    dt, mid = dtype_of(bd), 1 << (bd - 1)
    clean, noisy = [], []
    for ph, pw in shapes_of(w, h, ss):
        ys, xs = np.arange(ph)[:, None], np.arange(pw)[None, :]
        sign = np.where(((xs >> m) + (ys >> m)) & 1, -amp, amp)
        clean.append(np.full((ph, pw), mid, dt))
        noisy.append((mid + sign).astype(dt))
    return noisy, clean


def alternating_pair(w, h, bd, ss, seed=0, on="luma"):
    """The clean luma alternates between bin 4 and bin 20, sample by sample (on = "luma") or chroma sample by chroma sample
    (on = "chroma": cells of (1 << xdec) x (1 << ydec) luma samples), so that every box of that plane lies in bin 12, which no
    sample of it is in.  The residual is random."""
    subx, suby = SUBSAMPLINGS[ss] if on == "chroma" else (0, 0)
    step = 1 << (bd - 5)
    noisy, clean = planes_of(w, h, bd, ss, seed=seed, amp=step)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    luma = np.where(((xs >> subx) + (ys >> suby)) & 1, 20 * step + step // 2, 4 * step + step // 2)
    d = noisy[0].astype(np.int64) - clean[0]
    clean[0] = luma.astype(clean[0].dtype)
    noisy[0] = np.clip(luma + d, 0, (1 << bd) - 1).astype(clean[0].dtype)
    return noisy, clean


def floor_pair(w, h, bd, ss, seed=0, kind="three"):
    """kind = "three": every 2 x 2 luma box holds three samples on the lower edge e of bin 9 and, at its odd corner, one sample
    one below it: the box mean is below e at every scale and lies in bin 8, a rounded mean lies in bin 9.  kind = "half": the
    luma is e - 1 on even columns and e on odd ones: luma boxes lie in bin 8 (a rounded mean: 9), and a chroma sample's
    averageLuma is (2 e - 1 + 1) >> 1 = e, bin 9, where half the plain sum of the luma samples is e - 1/2, bin 8."""
    step = 1 << (bd - 5)
    e = 9 * step
    noisy, clean = planes_of(w, h, bd, ss, seed=seed, amp=step)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    luma = np.where((xs & ys & 1) == 1, e - 1, e) if kind == "three" else e - 1 + (xs & 1) + 0 * ys
    d = noisy[0].astype(np.int64) - clean[0]
    clean[0] = luma.astype(clean[0].dtype)
    noisy[0] = np.clip(luma + d, 0, (1 << bd) - 1).astype(clean[0].dtype)
    return noisy, clean


def extremes_pair(w, h, ss="420"):
    """+4095 everywhere at 12 bits (and its mirror): B = 4^k 4095, whose square leaves 32 bits from k = 3 on."""
    top = [np.full(s, 4095, np.uint16) for s in shapes_of(w, h, ss)]
    zero = [np.zeros(s, np.uint16) for s in shapes_of(w, h, ss)]
    return top, zero


@pytest.mark.parametrize("ss", ["420", "422", "444"])
def test_exact_identities(ss):
    subx, suby = SUBSAMPLINGS[ss]
    bd = 10
    # the number of boxes
    for w, h in ((37, 23), (95, 70), (64, 33)):
        noisy, clean = planes_of(w, h, bd, ss, seed=8, amp=40)
        rec = S.scale_frame(noisy, clean, bd, subx, suby)
        for c, (ph, pw) in enumerate(shapes_of(w, h, ss)):
            for k in range(1, 6):
                assert int(rec["n"][c, k - 1].sum()) == (pw >> k) * (ph >> k)
    # sides that are multiples of 32 (of the chroma planes too): every scale sums every sample, as the plain record does
    w, h = 128, 64
    noisy, clean = planes_of(w, h, bd, ss, seed=9, amp=40)
    rec, own = S.scale_frame(noisy, clean, bd, subx, suby), R.measure_frame(noisy, clean, bd, subx, suby)
    for c in range(3):
        for k in range(5):
            assert int(rec["s1"][c, k].sum()) == int(own["s1"][c].sum()) != 0
    # a constant residual
    clean = [np.full(s, 300, np.uint16) for s in shapes_of(w, h, ss)]
    rec = S.scale_frame([p + 7 for p in clean], clean, bd, subx, suby)
    for c in range(3):
        for k in range(1, 6):
            n = int(rec["n"][c, k - 1].sum())
            assert n and int(rec["s2"][c, k - 1].sum()) == n * (4 ** k * 7) ** 2 and int(rec["s1"][c, k - 1].sum()) == n * 4 ** k * 7


@pytest.mark.parametrize("m", range(6))
def test_each_scale_is_pinned_by_its_own_checkerboard(m):
    """Cells of 2^m: B is +-4^k amp for k <= m and 0 for every k > m.  m = 0, the sample checkerboard: every scale record is
    zero while the plain s2 is not."""
    bd, w, h, amp = 10, 128, 64, 5
    noisy, clean = checkerboard_pair(w, h, bd, "444", m, amp)
    rec, own = S.scale_frame(noisy, clean, bd, 0, 0), R.measure_frame(noisy, clean, bd, 0, 0)
    assert int(own["s2"][0].sum()) == w * h * amp * amp
    for k in range(1, 6):
        n = (w >> k) * (h >> k)
        assert int(rec["n"][0, k - 1].sum()) == n
        assert int(rec["s2"][0, k - 1].sum()) == (n * (4 ** k * amp) ** 2 if k <= m else 0), (m, k)
        assert int(rec["s1"][0, k - 1].sum()) == 0
    assert_same(rec, box_loop(noisy, clean, bd, 0, 0), f"cells of {1 << m}")


def test_each_rule_bites_on_the_designed_content():
    bd, w, h = 10, 70, 66
    # the box binned by one of its samples: boxes in a bin no sample is in
    for ss, on in (("444", "luma"), ("420", "luma"), ("420", "chroma"), ("422", "chroma")):
        subx, suby = SUBSAMPLINGS[ss]
        noisy, clean = alternating_pair(w, h, bd, ss, seed=1, on=on)
        right, wrong = S.scale_frame(noisy, clean, bd, subx, suby), S.scale_frame(noisy, clean, bd, subx, suby, bin_by_sample=True)
        c = 0 if on == "luma" else 1
        sample_bins = set(np.unique(R.intensity(clean, c, subx, suby) >> (bd - 5)).tolist())
        assert sample_bins == {4, 20}, (ss, on, sample_bins)
        for k in range(5):
            assert np.flatnonzero(right["n"][c, k]).tolist() == [12], (ss, on, k)
            assert set(np.flatnonzero(wrong["n"][c, k]).tolist()) <= {4, 20}
        assert_same(right, box_loop(noisy, clean, bd, subx, suby), f"alternating {ss} {on}")
    # the box mean floored, not rounded
    for kind in ("three", "half"):
        noisy, clean = floor_pair(w, h, bd, "420", seed=2, kind=kind)
        right, wrong = S.scale_frame(noisy, clean, bd, 1, 1), S.scale_frame(noisy, clean, bd, 1, 1, rounded_mean=True)
        for k in range(5):
            assert np.flatnonzero(right["n"][0, k]).tolist() == [8] and np.flatnonzero(wrong["n"][0, k]).tolist() == [9], (kind, k)
        assert_same(right, box_loop(noisy, clean, bd, 1, 1), f"floor {kind}")
    # chroma binned by the summed averageLuma, not by a sum of luma samples
    noisy, clean = floor_pair(w, h, bd, "420", seed=3, kind="half")
    right, wrong = S.scale_frame(noisy, clean, bd, 1, 1), S.scale_frame(noisy, clean, bd, 1, 1, luma_sum=True)
    for k in range(5):
        assert np.flatnonzero(right["n"][1, k]).tolist() == [9] and np.flatnonzero(wrong["n"][1, k]).tolist() == [8], k
    # the square in 64 bits
    noisy, clean = extremes_pair(128, 256)
    right, wrong = S.scale_frame(noisy, clean, 12, 1, 1), S.scale_frame(noisy, clean, 12, 1, 1, square32=True)
    for k in range(1, 6):
        n = (128 >> k) * (256 >> k)
        assert int(right["s2"][0, k - 1].sum()) == n * (4 ** k * 4095) ** 2
        assert (int(wrong["s2"][0, k - 1].sum()) != int(right["s2"][0, k - 1].sum())) == (k >= 3), k
    assert int(right["s2"][0, 4, 0]) == 32 * (1024 * 4095) ** 2 > 2 ** 48  # (the clean frame is black: bin 0)


# ---- the host-only entry points ----

def _clip(bd=10, ss="420", frames=3, w=75, h=67, seed=20):
    subx, suby = SUBSAMPLINGS[ss]
    pairs = [planes_of(w, h, bd, ss, seed=seed + k, amp=30 + 10 * k) for k in range(frames)]
    return [R.measure_frame(a, b, bd, subx, suby) for a, b in pairs], [S.scale_frame(a, b, bd, subx, suby) for a, b in pairs]


def test_sum_and_report_equal_the_restatement_byte_for_byte():
    from grav1synth_amd.measure import RECORD, SRECORD, format_scale_profile, sum_scale_records

    for bd, ss, w, h in ((10, "420", 75, 67), (12, "422", 64, 40), (8, "444", 33, 9), (10, "mono", 130, 70), (8, "420", 1, 1)):
        nplanes = 1 if ss == "mono" else 3
        plain, scale = _clip(bd, ss, 3, w, h)
        want_p, want_s = R.sum_records(plain), S.sum_records(scale)
        got = sum_scale_records(np.array([S.to_struct(r, SRECORD) for r in scale], SRECORD))
        assert not S.mismatches(got, want_s, "total")
        text = format_scale_profile(R.to_struct(want_p, RECORD), got, 3, bd, nplanes)
        assert text == S.format_scales(want_p, want_s, 3, bd, nplanes), text.decode()
        assert text.startswith(b"grainscales1\nframes 3 bit_depth %d planes %d\nplane 0\nscale 1 boxes " % (bd, nplanes))
        assert text.count(b"\nscale ") == 5 * nplanes and text.count(b"\ngain_ratio ") == 0
        if w < 32 or h < 32:
            assert b"\nscale 5 boxes 0 - -\n" in text
        # two columns: the second clip is another draw of the same law
        plain2, scale2 = _clip(bd, ss, 2, w, h, seed=40)
        other_p, other_s = R.sum_records(plain2), S.sum_records(scale2)
        two = format_scale_profile(R.to_struct(want_p, RECORD), got, 3, bd, nplanes, synth=R.to_struct(other_p, RECORD),
                                   ssynth=S.to_struct(other_s, SRECORD))
        assert two == S.format_scales(want_p, want_s, 3, bd, nplanes, synth=other_p, ssynth=other_s), two.decode()
        lines = two.decode().splitlines()
        assert all(len(l.split()) == 8 for l in lines if l.startswith("scale ")) and all(len(l.split()) == 6 for l in lines if l.startswith("sbin "))
        assert sum(l.startswith("gain_ratio ") for l in lines) == 5 * nplanes
        # a capacity one byte short, and the exact capacity
        with pytest.raises(_lib.G1SError) as e:
            format_scale_profile(R.to_struct(want_p, RECORD), got, 3, bd, nplanes, cap=len(text) - 1)
        assert e.value.code == _lib.G1S_ERR_CAPACITY
        assert format_scale_profile(R.to_struct(want_p, RECORD), got, 3, bd, nplanes, cap=len(text)) == text


def test_frames_0_and_the_undefined_values():
    from grav1synth_amd.measure import RECORD, SRECORD, format_scale_profile

    def fmt(p, s, frames, bd, nplanes=3, synth=None, ssynth=None):
        got = format_scale_profile(R.to_struct(p, RECORD), S.to_struct(s, SRECORD), frames, bd, nplanes,
                                   synth=None if synth is None else R.to_struct(synth, RECORD),
                                   ssynth=None if ssynth is None else S.to_struct(ssynth, SRECORD))
        assert got == S.format_scales(p, s, frames, bd, nplanes, synth=synth, ssynth=ssynth), got.decode()
        return got.decode()

    zp, zs = R.empty_record(), S.empty_record()
    assert fmt(zp, zs, 0, 10) == "grainscales1\nframes 0 bit_depth 10 planes 3\nplane 0\nplane 1\nplane 2\n" == fmt(zp, zs, 0, 10, synth=zp, ssynth=zs)
    assert fmt(zp, zs, 0, 8, 1) == "grainscales1\nframes 0 bit_depth 8 planes 1\nplane 0\n"
    # no boxes at a scale (m = 0): "-" for both values
    noisy, clean = planes_of(9, 7, 8, "444", seed=1, amp=20)
    p, s = R.measure_frame(noisy, clean, 8, 0, 0), S.scale_frame(noisy, clean, 8, 0, 0)
    text = fmt(p, s, 1, 8)
    assert "scale 3 boxes 0 - -\nscale 4 boxes 0 - -\nscale 5 boxes 0 - -\n" in text and "scale 2 boxes 2 " in text
    # no residual at all (V_0 = 0): sigma 0.0000, gain "-"; beside it as the second column: gain' and gain_ratio "-"
    p0, s0 = R.measure_frame(clean, clean, 8, 0, 0), S.scale_frame(clean, clean, 8, 0, 0)
    assert "scale 1 boxes 12 0.0000 -\n" in fmt(p0, s0, 1, 8)
    text = fmt(p, s, 1, 8, synth=p0, ssynth=s0)
    assert "gain_ratio 1 -\n" in text and all(l.split()[-2:] == ["0.0000", "-"] for l in text.splitlines() if l.startswith(("scale 1 ", "scale 2 ")))
    # the second column has no boxes where the first has: sigma' "-"
    text = fmt(p, s, 1, 8, synth=zp, ssynth=zs)
    assert all(l.split()[-1] == "-" for l in text.splitlines() if l.startswith("sbin ")) and "gain_ratio 2 -\n" in text
    # a gain of exactly 0 (the sample checkerboard): gain 0.0000, gain_ratio "-"
    noisy, clean = checkerboard_pair(64, 64, 10, "444", 0, 5)
    pc, sc = R.measure_frame(noisy, clean, 10, 0, 0), S.scale_frame(noisy, clean, 10, 0, 0)
    text = fmt(pc, sc, 1, 10, synth=pc, ssynth=sc)
    assert "scale 5 boxes 4 0.0000 0.0000 0.0000 0.0000\n" in text and text.count("gain_ratio 5 -\n") == 3
    # one of synth and ssynth alone, and a plane count rule 5 does not have
    L = _lib.lib()
    a, b = R.to_struct(pc, RECORD), S.to_struct(sc, SRECORD)
    buf = C.create_string_buffer(1 << 16)
    assert L.g1s_format_measure_scales(a.ctypes.data, b.ctypes.data, a.ctypes.data, None, 1, 10, 3, buf, len(buf)) == -1
    assert L.g1s_format_measure_scales(a.ctypes.data, b.ctypes.data, None, b.ctypes.data, 1, 10, 3, buf, len(buf)) == -1
    assert L.g1s_format_measure_scales(a.ctypes.data, b.ctypes.data, None, None, 1, 10, 2, buf, len(buf)) == -1
    assert L.g1s_format_measure_scales(a.ctypes.data, None, None, None, 1, 10, 3, buf, len(buf)) == -1


def test_an_overflow_of_the_scale_sum_is_refused():
    from grav1synth_amd.measure import SRECORD, sum_scale_records

    def both(a, b):
        return np.array([S.to_struct(a, SRECORD), S.to_struct(b, SRECORD)], SRECORD)

    for name in ("n", "s2"):
        a, b = S.empty_record(), S.empty_record()
        a[name][1, 4, 4] = b[name][1, 4, 4] = np.uint64(2 ** 63)
        with pytest.raises(OverflowError):
            S.sum_records([a, b])
        with pytest.raises(_lib.G1SError):
            sum_scale_records(both(a, b))
    for at in ((2, 4, 31), (0, 0, 0)):
        for v in (2 ** 62, -2 ** 62 - 1):
            a, b = S.empty_record(), S.empty_record()
            a["s1"][at] = b["s1"][at] = v
            with pytest.raises(OverflowError):
                S.sum_records([a, b])
            with pytest.raises(_lib.G1SError):
                sum_scale_records(both(a, b))
    a, b = S.empty_record(), S.empty_record()  # the largest sums that fit are taken
    a["s2"][0, 4, 0], b["s2"][0, 4, 0] = np.uint64(2 ** 64 - 2), np.uint64(1)
    a["s1"][1, 1, 1], b["s1"][1, 1, 1] = -2 ** 62, -2 ** 62
    got = sum_scale_records(both(a, b))
    assert int(got["s2"][0, 4, 0]) == 2 ** 64 - 1 and int(got["s1"][1, 1, 1]) == -2 ** 63 and not S.mismatches(got, S.sum_records([a, b]), "edge")
    assert not S.mismatches(sum_scale_records(np.zeros(0, SRECORD)), S.empty_record(), "no records")


def test_scale_record_has_the_headers_layout(tmp_path):
    from grav1synth_amd.measure import SRECORD

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = ["n", "s1", "s2"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "g1s_diff.h"', "int main(void) {",
           '  printf("%zu %zu\\n", sizeof(g1s_measure_srecord_t), sizeof(g1s_measure_opts_t));']
    src += [f'  printf("%zu\\n", offsetof(g1s_measure_srecord_t, {f}));' for f in fields]
    src += ['  printf("%zu %zu\\n", sizeof(((g1s_measure_srecord_t *)0)->n[0]), sizeof(((g1s_measure_srecord_t *)0)->n[0][0]));', "  return 0;", "}"]
    (tmp_path / "m.c").write_text("\n".join(src))
    subprocess.check_call([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "m.c"), "-o", str(tmp_path / "m")])
    out = subprocess.check_output([str(tmp_path / "m")], text=True).split()
    assert int(out[0]) == C.sizeof(_lib.G1SMeasureSRecord) == SRECORD.itemsize == 11520
    assert int(out[1]) == C.sizeof(_lib.G1SMeasureOpts) == 12, "g1s_measure_opts_t is not extended"
    for f, off in zip(fields, out[2:5]):
        assert int(off) == getattr(_lib.G1SMeasureSRecord, f).offset == SRECORD.fields[f][1], f
    assert (int(out[5]), int(out[6])) == (5 * 32 * 8, 32 * 8), "[plane][scale][bin]"
    assert SRECORD["n"].shape == (3, 5, 32)


def test_the_2_to_the_30_predicate(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "scales_size_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "scales_size_host.cpp")])

    def ok(bd, w, h):
        out = subprocess.run([str(exe), str(bd), str(w), str(h)], capture_output=True, text=True, check=True).stdout.splitlines()
        assert out[1] == "a scales meter takes 12-bit planes of at most 2^30 samples"
        return out[0] == "1"

    # one value below, on and above the bound, in both orientations
    for w, h in ((32768, 32768), (65536, 16384), (16384, 65536), (32767, 32768), (65535, 16384), (1, 1)):
        assert w * h <= 2 ** 30 and ok(12, w, h), (w, h)
    for w, h in ((32769, 32768), (32768, 32769), (65536, 16385), (16385, 65536), (65536, 65536)):
        assert w * h > 2 ** 30 and not ok(12, w, h), (w, h)
    for bd in (8, 10):
        for w, h in ((32769, 32768), (65536, 65536), (1, 1)):
            assert ok(bd, w, h), (bd, w, h)
    # the bound is the one rule 21 states: 4^5 (2^12 - 1)^2 2^30 stays inside 64 bits, one more row of boxes does not have to
    assert 4 ** 5 * 4095 ** 2 * 2 ** 30 < 2 ** 64 <= 4 ** 5 * 4095 ** 2 * 2 ** 30 * 2


def test_the_scale_symbols_are_bound_and_new_scales_refuses_as_new_modes_before_a_device_is_looked_for():
    L = _lib.lib()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ("g1s_measure_new_scales", "g1s_measure_finish_scales", "g1s_measure_sum_scales", "g1s_format_measure_scales",
                 "g1s_measure_scales_timing", "g1s_measure_y4m_files_scales", "g1s_check_y4m_files_scales"):
        assert name in bound and hasattr(L, name)
    for modes in (4, 7, 0x80000000, 0xfffffffc):  # (bit 4 and above are still unknown; a bad bit depth does not hide it)
        assert not L.g1s_measure_new_scales(10, None, modes) and "unknown mode bits" in L.g1s_last_global_error().decode()
        assert not L.g1s_measure_new_scales(9, None, modes) and "unknown mode bits" in L.g1s_last_global_error().decode()
        assert not L.g1s_measure_new_modes(10, None, modes) and "unknown mode bits" in L.g1s_last_global_error().decode()
    for modes in (0, 1, 2, 3):
        assert not L.g1s_measure_new_scales(9, None, modes) and "8, 10 and 12" in L.g1s_last_global_error().decode()
        bad = _lib.G1SMeasureOpts(4, -1, 0)
        assert not L.g1s_measure_new_scales(9, C.byref(bad), modes) and "8, 10 and 12" in L.g1s_last_global_error().decode()
        assert not L.g1s_measure_new_scales(10, C.byref(bad), modes) and "struct_size" in L.g1s_last_global_error().decode()
    assert L.g1s_measure_finish_scales(None, None, 0, None) == -1 and L.g1s_measure_scales_timing(None, None, None) == -1
    assert L.g1s_measure_sum_scales(None, 1, None) == -1


def test_no_gpu_means_the_scales_meter_refuses():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from grav1synth_amd.measure import GrainMeter

    for kw in ({}, {"temporal": True}, {"cross": True}, {"temporal": True, "cross": True}):
        with pytest.raises(_lib.G1SError) as e:
            GrainMeter(10, scales=True, **kw)
        assert "measure has no CPU fallback" in str(e.value)


def test_scales_output_refusals(tmp_path, caplog):
    from grav1synth_amd import cli

    a, b, t, out, tout, xout, sout = (str(tmp_path / n) for n in ("a.y4m", "b.y4m", "t.tbl", "out.txt", "temporal.txt", "cross.txt", "scales.txt"))
    for p in (a, b):
        open(p, "wb").write(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 C420jpeg\nFRAME\n" + bytes(12))
    open(t, "wb").write(b"x")

    def no(*_):
        return False

    with caplog.at_level(logging.INFO, logger="grav1synth"):
        # PATH equal to an input
        assert cli.measure_command(a, b, out, scales=b) == -1 and cli.check_command(a, b, t, out, scales=t) == -1
        assert caplog.text.count(cli.SAME_AS_OUTPUT) == 2
        # PATH equal to -o's
        assert cli.measure_command(a, b, out, scales=out) == -1 and cli.check_command(a, b, t, out, scales=str(tmp_path) + "//out.txt") == -1
        assert caplog.text.count(cli.SAME_SCALES_OUTPUT) == 2
        # PATH equal to --temporal's
        assert cli.measure_command(a, b, out, temporal=tout, scales=tout) == -1 and cli.check_command(a, b, t, out, temporal=tout, scales=tout) == -1
        assert caplog.text.count(cli.SAME_SCALES_TEMPORAL) == 2
        # PATH equal to --cross's
        assert cli.measure_command(a, b, out, cross=xout, scales=xout) == -1 and cli.check_command(a, b, t, out, cross=xout, scales=xout) == -1
        assert caplog.text.count(cli.SAME_SCALES_CROSS) == 2
        assert cli.SAME_SCALES_OUTPUT == "--scales and -o name the same file: the two reports would overwrite each other. Exiting."
        assert cli.SAME_SCALES_TEMPORAL == "--scales and --temporal name the same file: the two reports would overwrite each other. Exiting."
        assert cli.SAME_SCALES_CROSS == "--scales and --cross name the same file: the two reports would overwrite each other. Exiting."
        # an existing scales output without -y is asked about like -o's
        open(sout, "wb").write(b"kept")
        assert cli.measure_command(a, b, out, confirm=no, scales=sout) == -1 and cli.check_command(a, b, t, out, confirm=no, scales=sout) == -1
        assert caplog.text.count(cli.NOT_OVERWRITING) == 2
    # nothing was opened: the refusals come before a device is looked for or an output is made
    assert open(sout, "rb").read() == b"kept" and not any(os.path.exists(p) for p in (out, tout, xout))
    # through main(): a refusal is logged and the exit status is 0
    assert cli.main(["measure", a, b, "-o", out, "--scales", out]) == 0 and cli.main(["check", a, b, "-g", t, "-o", out, "--scales", a]) == 0
    assert not os.path.exists(out)
    args = cli.build_parser().parse_args(["measure", a, b, "-o", out, "--scales", sout, "--cross", xout, "--temporal", tout, "-y"])
    assert (args.command, args.scales, args.cross, args.temporal, args.overwrite) == ("measure", sout, xout, tout, True)
    args = cli.build_parser().parse_args(["check", a, b, "-g", t, "-o", out, "--scales", sout])
    assert (args.command, args.scales, args.cross, args.temporal, args.grain) == ("check", sout, None, None, t)
    assert cli.build_parser().parse_args(["measure", a, b, "-o", out]).scales is None


# ---- the definition on noise whose gains are known ----
FRAMES, FW, FH = 12, 256, 256


def noise_gains(seed, filtered):
    """The gains of FRAMES flat 10-bit luma frames with rounded white Gaussian noise of sigma 3 (filtered: its 3 x 3 box SUMS, an
    integer filter, taken from a frame one sample larger all round so that every sample has nine taps)."""
    clean = [np.full((FH, FW), 512, np.uint16)]
    plain, scale = [], []
    for f in range(FRAMES):
        rng = np.random.default_rng([seed, f])
        wn = np.rint(rng.normal(0.0, 3.0, (FH + 2, FW + 2))).astype(np.int64)
        d = sum(wn[i:i + FH, j:j + FW] for i in range(3) for j in range(3)) if filtered else wn[1:-1, 1:-1]
        assert np.abs(d).max() < 512
        noisy = [(clean[0] + d).astype(np.uint16)]
        plain.append(R.measure_frame(noisy, clean, 10, 0, 0))
        scale.append(S.scale_frame(noisy, clean, 10, 0, 0))
    return S.column(R.sum_records(plain), S.sum_records(scale), 0)["gain"]


@pytest.mark.parametrize("seed", [7391, 1234, 40000])
def test_white_noise_has_gain_1_at_every_scale(seed):
    """A variance estimated from m boxes has relative standard deviation sqrt(2 / m); m = 12 (256 >> k)^2; within four of those.

    Observed (seed: gain at k = 1 .. 5):
     7391: 0.9999 1.0010 0.9974 1.0349 1.0027
     1234: 0.9995 0.9911 0.9969 0.9913 0.9838
    40000: 0.9997 0.9926 0.9724 0.9635 0.9699
    against 1 +- 0.0128, 0.0255, 0.0510, 0.1021, 0.2041."""
    gains = noise_gains(seed, False)
    print("seed %d white gains %s" % (seed, " ".join("%.4f" % g for g in gains)))
    for k in range(1, 6):
        m = FRAMES * (FW >> k) * (FH >> k)
        assert abs(gains[k - 1] - 1.0) < 4 * math.sqrt(2 / m), (k, gains[k - 1])


@pytest.mark.parametrize("seed", [7391, 1234, 40000])
def test_box_filtered_noise_has_the_gain_its_taps_count_to(seed):
    """A 3 x 3 box filter of white noise: a box of side L sums L + 2 white samples a row with weights 1, 2, 3, .., 3, 2, 1, whose
    squares sum to 9 L - 8 per dimension where L samples of variance 3 would give 3 L: gain = ((9 L - 8) / (3 L))^2, that is
    2.7778, 5.4444, 7.1111, 8.0278, 8.5069 for L = 2 .. 32.  Adjacent boxes share taps and are not independent: m counts as
    half of 12 (256 >> k)^2; within four relative standard deviations sqrt(2 / m).

    Observed (seed: gain at k = 1 .. 5):
     7391: 2.7768 5.4847 7.1798 8.3732 8.7014
     1234: 2.7728 5.4153 7.1279 8.0629 8.4741
    40000: 2.7759 5.4008 6.9273 7.7788 8.2145
    against the expected value times 1 +- 0.0180, 0.0361, 0.0722, 0.1443, 0.2887."""
    gains = noise_gains(seed, True)
    print("seed %d filtered gains %s" % (seed, " ".join("%.4f" % g for g in gains)))
    for k in range(1, 6):
        L = 1 << k
        want = ((9 * L - 8) / (3 * L)) ** 2
        m = FRAMES * (FW >> k) * (FH >> k) / 2
        assert abs(gains[k - 1] / want - 1.0) < 4 * math.sqrt(2 / m), (k, gains[k - 1], want)
