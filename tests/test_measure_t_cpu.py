"""The temporal record of `measure` without a device: tests/measure_t_ref.py against a plain quadruple loop and its exact
identities, the host-only entry points (g1s_measure_sum_temporal, g1s_format_measure_temporal) against the restatement byte
for byte, the record's layout against the C compiler's, and the commands' new refusals."""
from __future__ import annotations

import ctypes as C
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import measure_ref as R
from tests import measure_t_ref as T
from tests.test_measure_cpu import SUBSAMPLINGS, planes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quadruple_loop(noisy, clean, prev_noisy, prev_clean, bd, xdec, ydec):
    """Rules 7 - 9 as written: one plane, one row, one sample and one offset at a time, in Python integers."""
    rec = T.empty_record()
    W = clean[0].shape[1]
    for c in range(len(clean)):
        ph, pw = clean[c].shape
        for y in range(ph):
            for x in range(pw):
                d = int(noisy[c][y, x]) - int(clean[c][y, x])
                e = int(prev_noisy[c][y, x]) - int(prev_clean[c][y, x])
                if c == 0:
                    I = int(clean[0][y, x])
                else:
                    ys, xs = y << ydec, x << xdec
                    I = int(clean[0][ys, xs])
                    if xdec:
                        I = (I + int(clean[0][ys, min(xs + 1, W - 1)]) + 1) >> 1
                k = I >> (bd - 5)
                rec["n"][c, k] += np.uint64(1)
                rec["x"][c, k] += d * e
                rec["u"][c, k] += np.uint64(d * d)
                rec["v"][c, k] += np.uint64(e * e)
                for i in range(25):
                    dy, dx = i // 5 - 2, i % 5 - 2
                    if 0 <= x + dx < pw and 0 <= y + dy < ph:
                        rec["c"][c, i] += d * (int(prev_noisy[c][y + dy, x + dx]) - int(prev_clean[c][y + dy, x + dx]))
    return rec


def assert_same(a, b, what):
    for name, _dt, _size in T.FIELDS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), f"{what}: {name}"


@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (3, 2), (5, 5), (9, 7), (1, 7), (8, 1)])
def test_restatement_equals_a_quadruple_loop(ss, size):
    w, h = size
    subx, suby = SUBSAMPLINGS[ss]
    for bd in (8, 10, 12):
        noisy, clean = planes_of(w, h, bd, ss, seed=3)
        pn, pc = planes_of(w, h, bd, ss, seed=4)
        assert_same(T.temporal_frame(noisy, clean, pn, pc, bd, subx, suby), quadruple_loop(noisy, clean, pn, pc, bd, subx, suby),
                    f"{w}x{h} {bd} bit {ss}")


def test_offsets_and_term_counts():
    assert T.OFFSETS[12] == (0, 0) and T.OFFSETS[0] == (-2, -2) and T.OFFSETS[4] == (2, -2) and T.OFFSETS[24] == (2, 2)
    assert all(i == (dy + 2) * 5 + (dx + 2) for i, (dx, dy) in enumerate(T.OFFSETS))
    assert T.terms(2, 1) == [0] * 10 + [0, 1, 2, 1, 0] + [0] * 10
    assert T.terms(1, 1) == [0] * 12 + [1] + [0] * 12


@pytest.mark.parametrize("ss", ["420", "444", "mono"])
def test_exact_identities(ss):
    subx, suby = SUBSAMPLINGS[ss]
    bd, w, h = 10, 37, 23
    noisy, clean = planes_of(w, h, bd, ss, seed=7, amp=50)
    pn, pc = planes_of(w, h, bd, ss, seed=8, amp=50)
    own = R.measure_frame(noisy, clean, bd, subx, suby)
    rec = T.temporal_frame(noisy, clean, pn, pc, bd, subx, suby)
    # n and u are the n and s2 of pair t's own record
    assert np.array_equal(rec["n"], own["n"]) and np.array_equal(rec["u"], own["s2"])
    # pair t - 1 equal to pair t: x = u = v, c[12] = r[24], c[i] = r[j] for the offsets both windows have, c(d) = c(-d)
    same = T.temporal_frame(noisy, clean, noisy, clean, bd, subx, suby)
    assert np.array_equal(same["x"].astype(np.uint64), same["u"]) and np.array_equal(same["u"], same["v"])
    assert np.array_equal(same["c"][:, 12], own["r"][:, 24])
    shared = 0
    for i, off in enumerate(T.OFFSETS):
        if off in R.OFFSETS:
            assert np.array_equal(same["c"][:, i], own["r"][:, R.OFFSETS.index(off)]), off
            shared += 1
        assert np.array_equal(same["c"][:, i], same["c"][:, 24 - i]), off
    assert shared == 13  # dy = -2, -1 with dx = -2 .. 2; dy = 0 with dx = -2, -1; (0, 0)


@pytest.mark.parametrize("i", range(25))
def test_a_moved_residual_peaks_at_its_offset(i):
    """d_{t-1} is d_t moved by delta_i inside a zero margin: c[i] is the sum of d_t^2 over the overlap, which is all of d_t's
    support, and the report's peak_rho names delta_i."""
    from grav1synth_amd.measure import TRECORD, format_temporal_profile

    dx, dy = T.OFFSETS[i]
    bd, w, h, m = 8, 21, 17, 3
    rng = np.random.default_rng(i)
    d = np.zeros((h, w), np.int64)
    d[m:h - m, m:w - m] = rng.integers(-40, 41, (h - 2 * m, w - 2 * m))
    e = np.zeros_like(d)
    e[m + dy:h - m + dy, m + dx:w - m + dx] = d[m:h - m, m:w - m]  # e(p + delta) = d(p)
    clean = np.full((h, w), 100, np.uint8)
    rec = T.temporal_frame([(clean + d).astype(np.uint8)], [clean], [(clean + e).astype(np.uint8)], [clean], bd, 0, 0)
    assert int(rec["c"][0, i]) == int((d * d).sum()) == int(rec["u"][0].sum()) == int(rec["v"][0].sum())
    for text in (T.format_temporal(rec, 1, bd, w, h, 0, 0, 1), format_temporal_profile(T.to_struct(rec, TRECORD), 1, bd, w, h, 0, 0, 1)):
        peak = [line for line in text.decode().splitlines() if line.startswith("peak_rho ")]
        assert len(peak) == 1 and peak[0].split()[1:3] == [str(dx), str(dy)], peak


def _clip_trecords(bd=10, ss="420", pairs=3, w=45, h=31, seed=20):
    subx, suby = SUBSAMPLINGS[ss]
    frames = [planes_of(w, h, bd, ss, seed=seed + k, amp=30 + 10 * k) for k in range(pairs + 1)]
    return T.run_records(frames, bd, subx, suby)


def test_sum_and_report_equal_the_restatement_byte_for_byte():
    from grav1synth_amd.measure import TRECORD, format_temporal_profile, sum_temporal_records

    # (a plane 1 or 2 samples wide: lags without terms; 2 x 9 4:4:4, 3 x 2 mono, and the chroma of 3 x 5 4:2:0)
    for bd, ss, w, h in ((10, "420", 45, 31), (8, "mono", 3, 2), (12, "422", 64, 5), (8, "444", 2, 9), (8, "mono", 1, 4), (10, "420", 3, 5)):
        subx, suby = SUBSAMPLINGS[ss]
        nplanes = 1 if ss == "mono" else 3
        recs = _clip_trecords(bd, ss, 3, w, h)
        want = T.sum_records(recs)
        got = sum_temporal_records(np.array([T.to_struct(r, TRECORD) for r in recs], TRECORD))
        assert not T.mismatches(got, want, "total")
        text = format_temporal_profile(got, 3, bd, w, h, subx, suby, nplanes)
        assert text == T.format_temporal(want, 3, bd, w, h, subx, suby, nplanes), text.decode()
        assert text.startswith(b"graintemporal1\npairs 3 bit_depth %d planes %d\nplane 0\n" % (bd, nplanes))
        assert text.count(b"\nlag ") == 25 * nplanes and text.count(b"\ntemporal_rho ") == nplanes and text.count(b"\npeak_rho ") == nplanes
        if w <= 2:
            assert b"lag -2 0 -\n" in text and b"lag 2 2 -\n" in text
        # two columns: the second clip is another draw of the same law
        other = T.sum_records(_clip_trecords(bd, ss, 2, w, h, seed=40) + [T.empty_record()])
        two = format_temporal_profile(got, 3, bd, w, h, subx, suby, nplanes, synth=T.to_struct(other, TRECORD))
        assert two == T.format_temporal(want, 3, bd, w, h, subx, suby, nplanes, synth=other), two.decode()
        assert all(len(line.split()) == 7 for line in two.decode().splitlines() if line.startswith("peak_rho "))
        # a capacity one byte short, and the exact capacity
        with pytest.raises(_lib.G1SError) as e:
            format_temporal_profile(got, 3, bd, w, h, subx, suby, nplanes, cap=len(text) - 1)
        assert e.value.code == _lib.G1S_ERR_CAPACITY
        assert format_temporal_profile(got, 3, bd, w, h, subx, suby, nplanes, cap=len(text)) == text


def test_pairs_0_and_the_undefined_values():
    from grav1synth_amd.measure import TRECORD, format_temporal_profile

    zero = T.to_struct(T.empty_record(), TRECORD)
    for nplanes in (1, 3):
        text = format_temporal_profile(zero, 0, 10, 16, 8, 1, 1, nplanes)
        assert text == T.format_temporal(T.empty_record(), 0, 10, 16, 8, 1, 1, nplanes)
        assert text == b"graintemporal1\npairs 0 bit_depth 10 planes %d\n" % nplanes + b"".join(b"plane %d\n" % c for c in range(nplanes))
    two = format_temporal_profile(zero, 0, 10, 16, 8, 1, 1, 3, synth=zero)
    assert two == T.format_temporal(T.empty_record(), 0, 10, 16, 8, 1, 1, 3, synth=T.empty_record()) and two.count(b"\n") == 5
    # u or v zero in a bin; pair t - 1 without a residual at all: every rho undefined, "- - -"
    noisy, clean = planes_of(9, 9, 8, "mono", seed=1, amp=20)
    rec = T.temporal_frame(noisy, clean, clean, clean, 8, 0, 0)
    assert rec["u"].any() and not rec["v"].any()
    text = format_temporal_profile(T.to_struct(rec, TRECORD), 1, 8, 9, 9, 0, 0, 1)
    assert text == T.format_temporal(rec, 1, 8, 9, 9, 0, 0, 1)
    assert b"lag 0 0 -\n" in text and text.endswith(b"temporal_rho -\npeak_rho - - -\n")
    assert all(line.split()[3] == "-" for line in text.decode().splitlines() if line.startswith("bin "))
    # one bin with v = 0 beside bins that have both: "-" in that line alone; the same in the second column
    mixed = T.temporal_frame(noisy, clean, *planes_of(9, 9, 8, "mono", seed=2, amp=20)[:1], clean, 8, 0, 0)
    k = int(np.flatnonzero(mixed["n"][0])[0])
    mixed["v"][0, k] = 0
    text = format_temporal_profile(T.to_struct(mixed, TRECORD), 1, 8, 9, 9, 0, 0, 1, synth=T.to_struct(rec, TRECORD))
    assert text == T.format_temporal(mixed, 1, 8, 9, 9, 0, 0, 1, synth=rec)
    lines = [line.split() for line in text.decode().splitlines() if line.startswith("bin ")]
    assert lines[0][1] == str(k) and lines[0][3:] == ["-", "-"] and all(l[3] != "-" and l[4] == "-" for l in lines[1:])
    assert text.decode().splitlines()[-1].endswith(" - - -")
    # a geometry rule 5 does not have
    assert _lib.lib().g1s_format_measure_temporal(zero.ctypes.data, None, 1, 8, 9, 9, 0, 1, 3, C.create_string_buffer(64), 64) == -1


def test_an_overflow_of_the_temporal_sum_is_refused():
    from grav1synth_amd.measure import TRECORD, sum_temporal_records

    def both(a, b):
        return np.array([T.to_struct(a, TRECORD), T.to_struct(b, TRECORD)], TRECORD)

    for name in ("n", "u", "v"):
        a, b = T.empty_record(), T.empty_record()
        a[name][1, 4] = b[name][1, 4] = np.uint64(2 ** 63)
        with pytest.raises(OverflowError):
            T.sum_records([a, b])
        with pytest.raises(_lib.G1SError):
            sum_temporal_records(both(a, b))
    for name, at in (("x", (2, 31)), ("c", (2, 24)), ("c", (0, 0))):
        for v in (2 ** 62, -2 ** 62 - 1):
            a, b = T.empty_record(), T.empty_record()
            a[name][at] = b[name][at] = v
            with pytest.raises(OverflowError):
                T.sum_records([a, b])
            with pytest.raises(_lib.G1SError):
                sum_temporal_records(both(a, b))
    a, b = T.empty_record(), T.empty_record()  # the largest sums that fit are taken
    a["v"][0, 0], b["v"][0, 0] = np.uint64(2 ** 64 - 2), np.uint64(1)
    a["x"][1, 1], b["x"][1, 1] = -2 ** 62, -2 ** 62
    got = sum_temporal_records(both(a, b))
    assert int(got["v"][0, 0]) == 2 ** 64 - 1 and int(got["x"][1, 1]) == -2 ** 63 and not T.mismatches(got, T.sum_records([a, b]), "edge")
    assert not T.mismatches(sum_temporal_records(np.zeros(0, TRECORD)), T.empty_record(), "no records")


def test_temporal_record_has_the_headers_layout(tmp_path):
    from grav1synth_amd.measure import TRECORD

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = ["n", "x", "u", "v", "c"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "g1s_diff.h"', "int main(void) {",
           '  printf("%zu %zu\\n", sizeof(g1s_measure_trecord_t), sizeof(g1s_measure_opts_t));']
    src += [f'  printf("%zu\\n", offsetof(g1s_measure_trecord_t, {f}));' for f in fields]
    src += ["  return 0;", "}"]
    (tmp_path / "m.c").write_text("\n".join(src))
    subprocess.check_call([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "m.c"), "-o", str(tmp_path / "m")])
    out = subprocess.check_output([str(tmp_path / "m")], text=True).split()
    assert int(out[0]) == C.sizeof(_lib.G1SMeasureTRecord) == TRECORD.itemsize == 8 * (4 * 96 + 75)
    assert int(out[1]) == C.sizeof(_lib.G1SMeasureOpts) == 12, "g1s_measure_opts_t is not extended"
    for f, off in zip(fields, out[2:7]):
        assert int(off) == getattr(_lib.G1SMeasureTRecord, f).offset == TRECORD.fields[f][1], f


def test_the_temporal_symbols_are_bound_and_refuse_before_a_device_is_looked_for():
    L = _lib.lib()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ("g1s_measure_new_temporal", "g1s_measure_cut", "g1s_measure_finish_temporal", "g1s_measure_sum_temporal",
                 "g1s_format_measure_temporal", "g1s_measure_y4m_files_temporal", "g1s_check_y4m_files_temporal"):
        assert name in bound and hasattr(L, name)
    assert not L.g1s_measure_new_temporal(9, None)
    assert "8, 10 and 12" in L.g1s_last_global_error().decode()
    bad = _lib.G1SMeasureOpts(4, -1, 0)
    assert not L.g1s_measure_new_temporal(10, C.byref(bad))
    assert "struct_size" in L.g1s_last_global_error().decode()
    assert L.g1s_measure_cut(None) == -1 and L.g1s_measure_finish_temporal(None, None, 0, None) == -1


def test_no_gpu_means_the_temporal_meter_refuses():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from grav1synth_amd.measure import GrainMeter

    with pytest.raises(_lib.G1SError) as e:
        GrainMeter(10, temporal=True)
    assert "measure has no CPU fallback" in str(e.value)


def test_temporal_output_refusals(tmp_path, caplog):
    from grav1synth_amd import cli

    a, b, t, out, tout = (str(tmp_path / n) for n in ("a.y4m", "b.y4m", "t.tbl", "out.txt", "temporal.txt"))
    for p in (a, b, t):
        open(p, "wb").write(b"x")

    def no(*_):
        return False

    with caplog.at_level(logging.INFO, logger="grav1synth"):
        # PATH equal to -o's
        assert cli.measure_command(a, b, out, temporal=out) == -1 and cli.check_command(a, b, t, out, temporal=str(tmp_path) + "//out.txt") == -1
        assert caplog.text.count(cli.SAME_OUTPUTS) == 2
        # PATH equal to an input
        assert cli.measure_command(a, b, out, temporal=b) == -1 and cli.check_command(a, b, t, out, temporal=t) == -1
        assert caplog.text.count(cli.SAME_AS_OUTPUT) == 2
        # an existing temporal output without -y is asked about like -o's
        open(tout, "wb").write(b"kept")
        assert cli.measure_command(a, b, out, confirm=no, temporal=tout) == -1 and cli.check_command(a, b, t, out, confirm=no, temporal=tout) == -1
        assert caplog.text.count(cli.NOT_OVERWRITING) == 2
    assert open(tout, "rb").read() == b"kept" and not os.path.exists(out)
    args = cli.build_parser().parse_args(["measure", a, b, "-o", out, "--temporal", tout, "-y"])
    assert (args.command, args.temporal, args.overwrite) == ("measure", tout, True)
    args = cli.build_parser().parse_args(["check", a, b, "-g", t, "-o", out, "--temporal", tout])
    assert (args.command, args.temporal, args.grain) == ("check", tout, t)
    assert cli.build_parser().parse_args(["measure", a, b, "-o", out]).temporal is None
