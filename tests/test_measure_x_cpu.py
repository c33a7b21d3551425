"""The cross record of `measure` without a device: tests/measure_x_ref.py against a plain quadruple loop and its exact
identities, rule 12's rounding on negative sums, the host-only entry points (g1s_measure_sum_cross, g1s_format_measure_cross)
against the restatement byte for byte, the record's layout against the C compiler's, the mode bits and the commands' new
refusals, and one statistical test of the definition on tests/grain_ref.py's rendering."""
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
from tests import grain_ref as G
from tests import measure_ref as R
from tests import measure_x_ref as X
from tests.test_grain_cpu import segment
from tests.test_measure_cpu import SUBSAMPLINGS, planes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 3), (5, 5), (9, 7), (13, 10)]  # luma; the odd ones make rule 12's clamp take part


def quadruple_loop(noisy, clean, bd, xdec, ydec):
    """Rules 12 - 16 as written: one pairing, one row, one sample and one offset at a time, in Python integers."""
    rec = X.empty_record()
    H, W = clean[0].shape
    ch, cw = clean[1].shape

    def d(c, x, y):
        return int(noisy[c][y, x]) - int(clean[c][y, x])

    def L(x, y):
        s = 0
        for i in range(ydec + 1):
            for j in range(xdec + 1):
                s += d(0, min((x << xdec) + j, W - 1), min((y << ydec) + i, H - 1))
        sh = xdec + ydec
        return (s + ((1 << sh) >> 1)) >> sh  # (Python's >> on a negative integer is arithmetic)

    value = [(lambda x, y: d(1, x, y), L), (lambda x, y: d(2, x, y), L), (lambda x, y: d(1, x, y), lambda x, y: d(2, x, y))]
    for j, (a, b) in enumerate(value):
        for y in range(ch):
            for x in range(cw):
                ys, xs = y << ydec, x << xdec
                I = int(clean[0][ys, xs])
                if xdec:
                    I = (I + int(clean[0][ys, min(xs + 1, W - 1)]) + 1) >> 1
                k = I >> (bd - 5)
                av, bv = a(x, y), b(x, y)
                rec["n"][j, k] += np.uint64(1)
                rec["x"][j, k] += av * bv
                rec["u"][j, k] += np.uint64(av * av)
                rec["v"][j, k] += np.uint64(bv * bv)
                for i in range(25):
                    dy, dx = i // 5 - 2, i % 5 - 2
                    if 0 <= x + dx < cw and 0 <= y + dy < ch:
                        rec["c"][j, i] += av * b(x + dx, y + dy)
    return rec


def assert_same(a, b, what):
    for name, _dt, _size in X.FIELDS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), f"{what}: {name}"


@pytest.mark.parametrize("ss", ["420", "422", "444"])
@pytest.mark.parametrize("size", SIZES)
def test_restatement_equals_a_quadruple_loop(ss, size):
    w, h = size
    subx, suby = SUBSAMPLINGS[ss]
    for bd in (8, 10, 12):
        noisy, clean = planes_of(w, h, bd, ss, seed=3)
        assert_same(X.cross_frame(noisy, clean, bd, subx, suby), quadruple_loop(noisy, clean, bd, subx, suby), f"{w}x{h} {bd} bit {ss}")
    mono = planes_of(w, h, 8, "mono", seed=3)
    assert_same(X.cross_frame(mono[0], mono[1], 8, 0, 0), X.empty_record(), "one plane: all zeros")


@pytest.mark.parametrize("ss", ["420", "422", "444"])
def test_exact_identities(ss):
    subx, suby = SUBSAMPLINGS[ss]
    bd, w, h = 10, 37, 23
    noisy, clean = planes_of(w, h, bd, ss, seed=7, amp=50)
    own = R.measure_frame(noisy, clean, bd, subx, suby)
    rec = X.cross_frame(noisy, clean, bd, subx, suby)
    for j in range(3):
        assert np.array_equal(rec["n"][j], own["n"][1]), "n[j] is the ordinary record's n[1]"
        assert int(rec["c"][j, 12]) == int(rec["x"][j].sum()), "c[j][12] = sum_k x[j][k]"
    assert np.array_equal(rec["u"][0], own["s2"][1]) and np.array_equal(rec["u"][2], own["s2"][1])
    assert np.array_equal(rec["u"][1], own["s2"][2]) and np.array_equal(rec["v"][2], own["s2"][2])
    assert np.array_equal(rec["v"][0], rec["v"][1]) and rec["v"][0].any()
    # Cb = Cr: pairings 0 and 1 are equal
    same = X.cross_frame([noisy[0], noisy[1], noisy[1]], [clean[0], clean[1], clean[1]], bd, subx, suby)
    for name, _dt, _size in X.FIELDS:
        assert np.array_equal(same[name][0], same[name][1]), name
    assert np.array_equal(same["x"][2].astype(np.uint64), same["u"][2]) and np.array_equal(same["u"][2], same["v"][2])
    if ss == "444":  # Cb = Y: pairing 0 has x = u = v
        y = X.cross_frame([noisy[0], noisy[0], noisy[2]], [clean[0], clean[0], clean[2]], bd, 0, 0)
        assert np.array_equal(y["x"][0].astype(np.uint64), y["u"][0]) and np.array_equal(y["u"][0], y["v"][0]) and y["u"][0].any()
        assert np.array_equal(X.luma_at_chroma(noisy[0].astype(np.int64) - clean[0], w, h, 0, 0), noisy[0].astype(np.int64) - clean[0])


def test_round2_rounds_negative_sums_towards_minus_infinity():
    """Boxes (-1, 0, 0, 0) and (-1, -1, -1, 0) give L = 0 and L = -1; a division that truncates gives 0 and 0.  The
    restatement run with the truncating rounding differs, so the test bites."""
    assert int(X.round2(-1, 2)) == 0 and int(X.round2(-3, 2)) == -1
    assert int(X.round2(-1, 2, truncate=True)) == 0 and int(X.round2(-3, 2, truncate=True)) == 0
    assert [int(X.round2(v, 1)) for v in (-3, -2, -1, 0, 1)] == [-1, -1, 0, 0, 1]
    noisy, clean = negative_boxes(8, 6, 8)
    d_y = noisy[0].astype(np.int64) - clean[0]
    L = X.luma_at_chroma(d_y, 4, 3, 1, 1)
    assert L.tolist() == [[0, -1, 0, -1], [-1, 0, -1, 0], [0, -1, 0, -1]]
    assert not X.luma_at_chroma(d_y, 4, 3, 1, 1, truncate=True).any()
    right, wrong = X.cross_frame(noisy, clean, 8, 1, 1), X.cross_frame(noisy, clean, 8, 1, 1, truncate=True)
    assert int(right["v"][0].sum()) == 6 and int(wrong["v"][0].sum()) == 0
    assert not np.array_equal(right["x"], wrong["x"]) and not np.array_equal(right["c"], wrong["c"])
    assert_same(right, quadruple_loop(noisy, clean, 8, 1, 1), "negative boxes")


def negative_boxes(w, h, bd):
    """A 4:2:0 pair whose 2 x 2 luma boxes hold the residuals (-1, 0, 0, 0) and (-1, -1, -1, 0) in a checkerboard; the chroma
    residuals are -3 and +2, so that the products with L = -1 show."""
    dt = np.uint8 if bd == 8 else np.uint16
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    three = (((xs >> 1) + (ys >> 1)) & 1) == 1
    first, last = ((xs & 1) == 0) & ((ys & 1) == 0), ((xs & 1) == 1) & ((ys & 1) == 1)
    d_y = np.where(three, np.where(last, 0, -1), np.where(first, -1, 0))
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    clean = [np.full((h, w), 100, dt), np.full((ch, cw), 90, dt), np.full((ch, cw), 80, dt)]
    noisy = [(clean[0] + d_y).astype(dt), (clean[1] - 3).astype(dt), (clean[2] + 2).astype(dt)]
    return noisy, clean


def moved_pair(i, w, h, m, bd=8, what="cr"):
    """what = "cr": d_Cr(p + delta_i) = d_Cb(p) on 4:4:4 planes of w x h inside a zero margin m (pairing 2 peaks at delta_i);
    what = "luma": d_Y(p + delta_i) = d_Cb(p) (pairing 0).  Returns (noisy, clean, the sum of d_Cb^2)."""
    dx, dy = X.OFFSETS[i]
    rng = np.random.default_rng(i)
    d = np.zeros((h, w), np.int64)
    d[m:h - m, m:w - m] = rng.integers(-40, 41, (h - 2 * m, w - 2 * m))
    e = np.zeros_like(d)
    e[m + dy:h - m + dy, m + dx:w - m + dx] = d[m:h - m, m:w - m]  # e(p + delta) = d(p)
    other = rng.integers(-5, 6, (h, w))
    clean = [np.full((h, w), 100, np.uint8)] * 3
    res = [other, d, e] if what == "cr" else [e, d, other]
    return [(clean[0] + r).astype(np.uint8) for r in res], clean, int((d * d).sum())


@pytest.mark.parametrize("i", range(25))
def test_a_moved_residual_peaks_at_its_offset(i):
    from grav1synth_amd.measure import XRECORD, format_cross_profile

    dx, dy = X.OFFSETS[i]
    w, h = 21, 17
    for what, j in (("cr", 2), ("luma", 0)):
        noisy, clean, energy = moved_pair(i, w, h, 3, what=what)
        rec = X.cross_frame(noisy, clean, 8, 0, 0)
        assert int(rec["c"][j, i]) == energy == int(rec["u"][j].sum()) == int(rec["v"][j].sum())
        assert int(np.argmax(rec["c"][j])) == i
        for text in (X.format_cross(rec, 1, 8, w, h, 0, 0), format_cross_profile(X.to_struct(rec, XRECORD), 1, 8, w, h, 0, 0)):
            peaks = [line for line in text.decode().splitlines() if line.startswith("peak_rho ")]
            assert len(peaks) == 3 and peaks[j].split()[1:3] == [str(dx), str(dy)], peaks


def _clip_xrecords(bd=10, ss="420", frames=3, w=45, h=31, seed=20):
    subx, suby = SUBSAMPLINGS[ss]
    return [X.cross_frame(*planes_of(w, h, bd, ss, seed=seed + k, amp=30 + 10 * k), bd, subx, suby) for k in range(frames)]


def test_sum_and_report_equal_the_restatement_byte_for_byte():
    from grav1synth_amd.measure import XRECORD, format_cross_profile, sum_cross_records

    # (a chroma plane 1 or 2 samples wide: lags without terms)
    for bd, ss, w, h in ((10, "420", 45, 31), (12, "422", 64, 5), (8, "444", 2, 9), (10, "420", 3, 5), (8, "420", 1, 1)):
        subx, suby = SUBSAMPLINGS[ss]
        recs = _clip_xrecords(bd, ss, 3, w, h)
        want = X.sum_records(recs)
        got = sum_cross_records(np.array([X.to_struct(r, XRECORD) for r in recs], XRECORD))
        assert not X.mismatches(got, want, "total")
        text = format_cross_profile(got, 3, bd, w, h, subx, suby)
        assert text == X.format_cross(want, 3, bd, w, h, subx, suby), text.decode()
        assert text.startswith(b"graincross1\nframes 3 bit_depth %d\npairing cb_luma\n" % bd)
        assert text.count(b"\nlag ") == 75 and text.count(b"\nzero_rho ") == 3 and text.count(b"\npeak_rho ") == 3
        assert text.count(b"\nbeta ") == 3 and text.count(b"\npartial_rho ") == 1 and text.index(b"\npartial_rho ") > text.index(b"pairing cb_cr")
        if (w + subx) >> subx <= 2:
            assert b"lag -2 0 -\n" in text and b"lag 2 2 -\n" in text
        # two columns: the second clip is another draw of the same law
        other = X.sum_records(_clip_xrecords(bd, ss, 2, w, h, seed=40) + [X.empty_record()])
        two = format_cross_profile(got, 3, bd, w, h, subx, suby, synth=X.to_struct(other, XRECORD))
        assert two == X.format_cross(want, 3, bd, w, h, subx, suby, synth=other), two.decode()
        lines = two.decode().splitlines()
        assert all(len(l.split()) == 7 for l in lines if l.startswith(("peak_rho ", "bin ")))
        assert all(len(l.split()) == 3 for l in lines if l.startswith(("zero_rho ", "beta ", "partial_rho ")))
        # a capacity one byte short, and the exact capacity
        with pytest.raises(_lib.G1SError) as e:
            format_cross_profile(got, 3, bd, w, h, subx, suby, cap=len(text) - 1)
        assert e.value.code == _lib.G1S_ERR_CAPACITY
        assert format_cross_profile(got, 3, bd, w, h, subx, suby, cap=len(text)) == text


def test_frames_0_and_the_undefined_values():
    from grav1synth_amd.measure import XRECORD, format_cross_profile

    zero = X.to_struct(X.empty_record(), XRECORD)
    text = format_cross_profile(zero, 0, 10, 16, 8, 1, 1)
    assert text == X.format_cross(X.empty_record(), 0, 10, 16, 8, 1, 1)
    assert text == b"graincross1\nframes 0 bit_depth 10\npairing cb_luma\npairing cr_luma\npairing cb_cr\n"
    assert format_cross_profile(zero, 0, 10, 16, 8, 1, 1, synth=zero) == text == X.format_cross(X.empty_record(), 0, 10, 16, 8, 1, 1, synth=X.empty_record())
    # no luma residual at all: v = 0 in the luma pairings -- every rho and beta of theirs "-", and partial_rho with them
    noisy, clean = planes_of(9, 9, 8, "444", seed=1, amp=20)
    rec = X.cross_frame([clean[0], noisy[1], noisy[2]], clean, 8, 0, 0)
    assert rec["u"][0].any() and not rec["v"][0].any() and rec["v"][2].any()
    text = format_cross_profile(X.to_struct(rec, XRECORD), 1, 8, 9, 9, 0, 0)
    assert text == X.format_cross(rec, 1, 8, 9, 9, 0, 0)
    blocks = text.decode().split("pairing ")[1:]
    for blk in blocks[:2]:
        assert "lag 0 0 -\n" in blk and "zero_rho -\npeak_rho - - -\nbeta -\n" in blk
        assert all(l.split()[3:] == ["-", "-"] for l in blk.splitlines() if l.startswith("bin "))
    assert "zero_rho -" not in blocks[2] and blocks[2].endswith("partial_rho -\n")
    # u = 0 but v != 0 in a bin: rho "-", beta 0.0000; the same bin in the second column
    mixed = X.cross_frame(noisy, clean, 8, 0, 0)
    full = (mixed["u"][0] != 0) & (mixed["v"][0] != 0)
    k = int(np.flatnonzero(full)[0])
    mixed["u"][0, k], mixed["x"][0, k] = 0, 0
    text = format_cross_profile(X.to_struct(mixed, XRECORD), 1, 8, 9, 9, 0, 0, synth=X.to_struct(rec, XRECORD))
    assert text == X.format_cross(mixed, 1, 8, 9, 9, 0, 0, synth=rec)
    first = [l.split() for l in text.decode().split("pairing ")[1].splitlines() if l.startswith("bin ")]
    assert sum(l[1] == str(k) and l[3:] == ["-", "0.0000", "-", "-"] for l in first) == 1
    assert all(l[5:] == ["-", "-"] and (l[3] != "-") == bool(full[int(l[1])] and int(l[1]) != k) for l in first)
    # a factor of partial_rho that is 0: Cb = Y on 4:4:4 makes r0 exactly 1
    one = X.cross_frame([noisy[0], noisy[0], noisy[2]], [clean[0], clean[0], clean[2]], 8, 0, 0)
    p = [X.profile(one, j, X.terms_f64(1, 9, 9, 0, 0)) for j in range(3)]
    assert p[0]["lag"][12] == 1.0 and X.partial_rho(p) == (False, 0.0)
    text = format_cross_profile(X.to_struct(one, XRECORD), 1, 8, 9, 9, 0, 0)
    assert text == X.format_cross(one, 1, 8, 9, 9, 0, 0) and b"zero_rho 1.0000\n" in text and text.endswith(b"partial_rho -\n")
    assert not format_cross_profile(X.to_struct(mixed, XRECORD), 1, 8, 9, 9, 0, 0).endswith(b"partial_rho -\n")
    # a geometry rule 5 does not have
    assert _lib.lib().g1s_format_measure_cross(zero.ctypes.data, None, 1, 8, 9, 9, 0, 1, C.create_string_buffer(64), 64) == -1


def test_an_overflow_of_the_cross_sum_is_refused():
    from grav1synth_amd.measure import XRECORD, sum_cross_records

    def both(a, b):
        return np.array([X.to_struct(a, XRECORD), X.to_struct(b, XRECORD)], XRECORD)

    for name in ("n", "u", "v"):
        a, b = X.empty_record(), X.empty_record()
        a[name][1, 4] = b[name][1, 4] = np.uint64(2 ** 63)
        with pytest.raises(OverflowError):
            X.sum_records([a, b])
        with pytest.raises(_lib.G1SError):
            sum_cross_records(both(a, b))
    for name, at in (("x", (2, 31)), ("c", (2, 24)), ("c", (0, 0))):
        for v in (2 ** 62, -2 ** 62 - 1):
            a, b = X.empty_record(), X.empty_record()
            a[name][at] = b[name][at] = v
            with pytest.raises(OverflowError):
                X.sum_records([a, b])
            with pytest.raises(_lib.G1SError):
                sum_cross_records(both(a, b))
    a, b = X.empty_record(), X.empty_record()  # the largest sums that fit are taken
    a["v"][0, 0], b["v"][0, 0] = np.uint64(2 ** 64 - 2), np.uint64(1)
    a["x"][1, 1], b["x"][1, 1] = -2 ** 62, -2 ** 62
    got = sum_cross_records(both(a, b))
    assert int(got["v"][0, 0]) == 2 ** 64 - 1 and int(got["x"][1, 1]) == -2 ** 63 and not X.mismatches(got, X.sum_records([a, b]), "edge")
    assert not X.mismatches(sum_cross_records(np.zeros(0, XRECORD)), X.empty_record(), "no records")


def test_cross_record_has_the_headers_layout(tmp_path):
    from grav1synth_amd.measure import TRECORD, XRECORD

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = ["n", "x", "u", "v", "c"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "g1s_diff.h"', "int main(void) {",
           '  printf("%zu %zu %zu %u %u\\n", sizeof(g1s_measure_xrecord_t), sizeof(g1s_measure_trecord_t), sizeof(g1s_measure_opts_t),',
           "         G1S_MEASURE_TEMPORAL, G1S_MEASURE_CROSS);"]
    src += [f'  printf("%zu\\n", offsetof(g1s_measure_xrecord_t, {f}));' for f in fields]
    src += ["  return 0;", "}"]
    (tmp_path / "m.c").write_text("\n".join(src))
    subprocess.check_call([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "m.c"), "-o", str(tmp_path / "m")])
    out = subprocess.check_output([str(tmp_path / "m")], text=True).split()
    assert int(out[0]) == int(out[1]) == C.sizeof(_lib.G1SMeasureXRecord) == XRECORD.itemsize == TRECORD.itemsize == 8 * (4 * 96 + 75)
    assert int(out[2]) == C.sizeof(_lib.G1SMeasureOpts) == 12, "g1s_measure_opts_t is not extended"
    assert (int(out[3]), int(out[4])) == (_lib.G1S_MEASURE_TEMPORAL, _lib.G1S_MEASURE_CROSS) == (1, 2)
    for f, off in zip(fields, out[5:10]):
        assert int(off) == getattr(_lib.G1SMeasureXRecord, f).offset == XRECORD.fields[f][1], f


def test_the_cross_symbols_are_bound_and_the_modes_refuse_before_a_device_is_looked_for():
    L = _lib.lib()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ("g1s_measure_new_modes", "g1s_measure_finish_cross", "g1s_measure_sum_cross", "g1s_format_measure_cross",
                 "g1s_measure_cross_timing", "g1s_measure_y4m_files_modes", "g1s_check_y4m_files_modes"):
        assert name in bound and hasattr(L, name)
    for modes in (4, 7, 0x80000000, 0xfffffffc):  # (with and without known bits beside them; a bad bit depth does not hide it)
        assert not L.g1s_measure_new_modes(10, None, modes) and "unknown mode bits" in L.g1s_last_global_error().decode()
        assert not L.g1s_measure_new_modes(9, None, modes) and "unknown mode bits" in L.g1s_last_global_error().decode()
    for modes in (0, 1, 2, 3):
        assert not L.g1s_measure_new_modes(9, None, modes) and "8, 10 and 12" in L.g1s_last_global_error().decode()
        bad = _lib.G1SMeasureOpts(4, -1, 0)
        assert not L.g1s_measure_new_modes(10, C.byref(bad), modes) and "struct_size" in L.g1s_last_global_error().decode()
    assert L.g1s_measure_finish_cross(None, None, 0, None) == -1 and L.g1s_measure_cross_timing(None, None, None) == -1


def test_no_gpu_means_the_cross_meter_refuses():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from grav1synth_amd.measure import GrainMeter

    for temporal in (False, True):
        with pytest.raises(_lib.G1SError) as e:
            GrainMeter(10, cross=True, temporal=temporal)
        assert "measure has no CPU fallback" in str(e.value)


def test_cross_output_refusals(tmp_path, caplog):
    from grav1synth_amd import cli
    from grav1synth_amd.measure import check_y4m_files, measure_y4m_files

    a, b, t, out, tout, xout = (str(tmp_path / n) for n in ("a.y4m", "b.y4m", "t.tbl", "out.txt", "temporal.txt", "cross.txt"))
    for p in (a, b, t):
        open(p, "wb").write(b"x")

    def no(*_):
        return False

    with caplog.at_level(logging.INFO, logger="grav1synth"):
        # PATH equal to an input
        assert cli.measure_command(a, b, out, cross=b) == -1 and cli.check_command(a, b, t, out, cross=t) == -1
        assert caplog.text.count(cli.SAME_AS_OUTPUT) == 2
        # PATH equal to -o's
        assert cli.measure_command(a, b, out, cross=out) == -1 and cli.check_command(a, b, t, out, cross=str(tmp_path) + "//out.txt") == -1
        assert caplog.text.count(cli.SAME_CROSS_OUTPUT) == 2
        # PATH equal to --temporal's
        assert cli.measure_command(a, b, out, temporal=tout, cross=tout) == -1 and cli.check_command(a, b, t, out, temporal=tout, cross=tout) == -1
        assert caplog.text.count(cli.SAME_CROSS_TEMPORAL) == 2
        # a monochrome clip
        for p in (a, b):
            open(p, "wb").write(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
        assert cli.measure_command(a, b, out, cross=xout) == -1 and cli.check_command(a, b, t, out, cross=xout) == -1
        assert caplog.text.count(cli.CROSS_NEEDS_CHROMA) == 2
        assert cli.CROSS_NEEDS_CHROMA == "--cross compares chroma with luma: the clip has no chroma planes"
        # an existing cross output without -y is asked about like -o's
        for p in (a, b):
            open(p, "wb").write(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 C420jpeg\nFRAME\n" + bytes(12))
        open(xout, "wb").write(b"kept")
        assert cli.measure_command(a, b, out, confirm=no, cross=xout) == -1 and cli.check_command(a, b, t, out, confirm=no, cross=xout) == -1
        assert caplog.text.count(cli.NOT_OVERWRITING) == 2
    assert open(xout, "rb").read() == b"kept" and not os.path.exists(out) and not os.path.exists(tout)
    # the library refuses a monochrome clip itself, before a device is looked for and before an output is opened
    for p in (a, b):
        open(p, "wb").write(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
    open(t, "wb").write(b"filmgrn1\n")
    for call in (lambda: measure_y4m_files(a, b, out, cross_output=str(tmp_path / "x2.txt")),
                 lambda: check_y4m_files(a, b, t, out, cross_output=str(tmp_path / "x2.txt"))):
        with pytest.raises(_lib.G1SError) as e:
            call()
        assert cli.CROSS_NEEDS_CHROMA in str(e.value)
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "x2.txt")
    args = cli.build_parser().parse_args(["measure", a, b, "-o", out, "--cross", xout, "--temporal", tout, "-y"])
    assert (args.command, args.cross, args.temporal, args.overwrite) == ("measure", xout, tout, True)
    args = cli.build_parser().parse_args(["check", a, b, "-g", t, "-o", out, "--cross", xout])
    assert (args.command, args.cross, args.temporal, args.grain) == ("check", xout, None, t)
    assert cli.build_parser().parse_args(["measure", a, b, "-o", out]).cross is None


FRAMES, FW, FH = 12, 64, 64


def rendered_record(coef: int, seed: int):
    """The clip's cross record of grain_ref's rendering of a table onto flat mid-grey 10-bit 4:2:0 frames: chroma_scaling_from_luma,
    one flat scaling function (20 at shift 8: the luma grain's sigma is 128 x 20 / 256 = 10 code values), no overlap, lag 0, so
    that the only chroma AR coefficient is the luma one.  The synthesis tiles a frame with windows of ONE 73 x 82 template, so
    the samples of a large frame are not independent draws; FRAMES frames of 2 x 2 blocks, each with a seed (a template) of its
    own, are much nearer to N independent samples.  Returns (record, N, the luma residual's standard deviation)."""
    bd = 10
    clean = [np.full((FH, FW), 512, np.uint16), np.full((FH // 2, FW // 2), 512, np.uint16), np.full((FH // 2, FW // 2), 512, np.uint16)]
    recs, sigma = [], []
    for k in range(FRAMES):
        seg = segment(0, [], [coef], [(0, 20), (255, 20)], [], seed=seed + 101 * k, ar_shift=7, overlap=False, chroma_scaling_from_luma=True)
        noisy = G.add_noise(clean, seg, bd, 1, 1)
        recs.append(X.cross_frame(noisy, clean, bd, 1, 1))
        sigma.append(float(np.std(noisy[0].astype(np.int64) - clean[0])))
    return X.sum_records(recs), FRAMES * (FW // 2) * (FH // 2), min(sigma)


@pytest.mark.parametrize("seed", [7391, 1234, 40000])
def test_the_slope_of_rendered_grain_is_the_tables_luma_coefficient(seed):
    """coef = 0: |zero_rho| of both luma pairings is below 5 / sqrt(N).  coef = 32 at shift 7: |beta - 0.25| is below five
    standard errors of the slope plus 1 % of 0.25 (the bound on the attenuation by the two roundings: 1/12 over a variance of 64
    and of 16), which also floors the tolerance at 1 % of 0.25 when the standard error is small.  The standard error comes from
    the record's own sums: se = sqrt((u / v - beta^2) / N).  N = 12 frames x 32 x 32 = 12288.

    Observed on the CPU (seed: zero_rho cb, cr at coef 0 | beta cb, cr at coef 32, se):
     7391: -0.0148, -0.0040 | 0.2206 (se 0.0181), 0.2409 (se 0.0176)
     1234: -0.0086, +0.0026 | 0.2316 (se 0.0178), 0.2523 (se 0.0183)
    40000: -0.0207, +0.0187 | 0.2079 (se 0.0177), 0.2844 (se 0.0177)
    against the bounds 0.0451 and 5 se + 0.0025 = 0.09; a single 256 x 192 frame (one template, 48 windows of it) gave a
    zero_rho of -0.0573 at seed 7391, which is why the frames are small and many."""
    rec, N, sigma = rendered_record(0, seed)
    assert sigma >= 8.0, "the luma grain's sigma"
    tm = X.terms_f64(FRAMES, FW, FH, 1, 1)
    for j in (0, 1):
        p = X.profile(rec, j, tm)
        print("seed %d coef 0 pairing %d zero_rho %.5f (bound %.5f)" % (seed, j, p["lag"][12], 5 / math.sqrt(N)))
        assert p["has_lag"][12] and abs(p["lag"][12]) < 5 / math.sqrt(N)
    rec, N, _sigma = rendered_record(32, seed)
    for j in (0, 1):
        p = X.profile(rec, j, tm)
        u, v = float(int(rec["u"][j].sum())), float(int(rec["v"][j].sum()))
        se = math.sqrt((u / v - p["beta"] ** 2) / N)
        print("seed %d coef 32 pairing %d beta %.5f se %.5f" % (seed, j, p["beta"], se))
        assert p["has_beta"] and abs(p["beta"] - 0.25) < 5 * se + 0.01 * 0.25
