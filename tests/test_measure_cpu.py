"""`measure` without a device: the numpy reference against a plain triple loop and its exact identities, the host-only
entry points (g1s_measure_sum, g1s_format_measure) against the reference, the record's layout against the C compiler's,
the commands' refusals, and the loud failure without a device."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSAMPLINGS = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "mono": (0, 0)}


def planes_of(w, h, bd, ss, seed, amp=None):
    """(noisy, clean): random clean planes over the whole range, a residual of up to +- amp on them (clipped to the range)."""
    rng = np.random.default_rng([seed, w, h, bd])
    subx, suby = SUBSAMPLINGS[ss]
    top = (1 << bd) - 1
    amp = top if amp is None else amp
    dt = np.uint8 if bd == 8 else np.uint16
    shapes = [(h, w)] + ([] if ss == "mono" else [((h + suby) >> suby, (w + subx) >> subx)] * 2)
    clean = [rng.integers(0, top + 1, s) for s in shapes]
    noisy = [np.clip(p + rng.integers(-amp, amp + 1, p.shape), 0, top) for p in clean]
    return [p.astype(dt) for p in noisy], [p.astype(dt) for p in clean]


def triple_loop(noisy, clean, bd, xdec, ydec):
    """Rules 1 - 5 as written, one sample and one offset at a time, in Python integers."""
    rec = R.empty_record()
    H, W = clean[0].shape
    for c in range(len(clean)):
        ph, pw = clean[c].shape
        d = [[int(noisy[c][y, x]) - int(clean[c][y, x]) for x in range(pw)] for y in range(ph)]
        for y in range(ph):
            for x in range(pw):
                if c == 0:
                    I = int(clean[0][y, x])
                else:
                    ys, xs = y << ydec, x << xdec
                    I = int(clean[0][ys, xs])
                    if xdec:
                        I = (I + int(clean[0][ys, min(xs + 1, W - 1)]) + 1) >> 1
                k = I >> (bd - 5)
                rec["n"][c, k] += np.uint64(1)
                rec["s1"][c, k] += d[y][x]
                rec["s2"][c, k] += np.uint64(d[y][x] * d[y][x])
                for i, (dx, dy) in enumerate(R.OFFSETS):
                    if 0 <= x + dx < pw and 0 <= y + dy < ph:
                        rec["r"][c, i] += d[y][x] * d[y + dy][x + dx]
    return rec


def assert_same(a, b, what):
    for name in ("n", "s1", "s2", "r"):
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), f"{what}: {name}"


@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (3, 2), (4, 4), (7, 5), (13, 9), (1, 11), (12, 1)])
def test_reference_equals_a_triple_loop(ss, size):
    w, h = size
    subx, suby = SUBSAMPLINGS[ss]
    for bd in (8, 10, 12):
        noisy, clean = planes_of(w, h, bd, ss, seed=3)
        assert_same(R.measure_frame(noisy, clean, bd, subx, suby), triple_loop(noisy, clean, bd, subx, suby), f"{w}x{h} {bd} bit {ss}")


def test_term_counts_of_planes_below_the_neighbourhood():
    assert R.terms(3, 2) == [0] * 7 + [0] * 7 + [0, 1 * 1, 2 * 1, 3 * 1, 2 * 1, 1 * 1, 0] + [0, 1 * 2, 2 * 2] + [6]
    noisy, clean = planes_of(3, 2, 8, "mono", seed=1)
    rec = R.measure_frame(noisy, clean, 8, 0, 0)
    assert all(rec["r"][0, i] == 0 for i, t in enumerate(R.terms(3, 2)) if t == 0)


@pytest.mark.parametrize("ss", ["420", "444", "mono"])
def test_exact_identities(ss):
    subx, suby = SUBSAMPLINGS[ss]
    bd, w, h = 10, 37, 23
    _noisy, clean = planes_of(w, h, bd, ss, seed=7)
    zero = R.measure_frame(clean, clean, bd, subx, suby)
    for c, p in enumerate(clean):
        assert int(zero["n"][c].sum()) == p.size
    assert not zero["s1"].any() and not zero["s2"].any() and not zero["r"].any()
    # a = b + k: s1 = k n, s2 = k^2 n, r[i] = k^2 terms_i
    k = 5
    low = [np.minimum(p, (1 << bd) - 1 - k) for p in clean]
    rec = R.measure_frame([p + k for p in low], low, bd, subx, suby)
    for c, p in enumerate(low):
        assert np.array_equal(rec["s1"][c], k * rec["n"][c].astype(np.int64))
        assert np.array_equal(rec["s2"][c], np.uint64(k * k) * rec["n"][c])
        assert rec["r"][c].tolist() == [k * k * t for t in R.terms(p.shape[1], p.shape[0])]
    # swapping a and b while binning by the same clean frame: s1 negated, s2 and r as they were
    noisy, clean = planes_of(w, h, bd, ss, seed=8, amp=40)
    fwd = R.measure_frame(noisy, clean, bd, subx, suby)
    mirrored = [(2 * c_.astype(np.int64) - n_.astype(np.int64)) for n_, c_ in zip(noisy, clean)]  # clean - (noisy - clean)
    back = R.measure_frame(mirrored, clean, bd, subx, suby)
    assert np.array_equal(back["s1"], -fwd["s1"]) and np.array_equal(back["s2"], fwd["s2"]) and np.array_equal(back["r"], fwd["r"])
    assert np.array_equal(back["n"], fwd["n"])


def _clip_records(bd=10, ss="420", frames=3, w=45, h=31):
    subx, suby = SUBSAMPLINGS[ss]
    return [R.measure_frame(*planes_of(w, h, bd, ss, seed=20 + k, amp=30 + 10 * k), bd, subx, suby) for k in range(frames)]


def test_sum_and_report_equal_the_reference_byte_for_byte():
    from grav1synth_amd.measure import RECORD, format_profile, sum_records

    for bd, ss, w, h in ((10, "420", 45, 31), (8, "mono", 3, 2), (12, "422", 64, 5), (8, "444", 2, 9)):
        subx, suby = SUBSAMPLINGS[ss]
        nplanes = 1 if ss == "mono" else 3
        recs = _clip_records(bd, ss, 3, w, h)
        want = R.sum_records(recs)
        got = sum_records(np.array([R.to_struct(r, RECORD) for r in recs], RECORD))
        assert not R.mismatches(got, want, "total")
        text = format_profile(got, 3, bd, w, h, subx, suby, nplanes)
        assert text == R.format_profile(want, 3, bd, w, h, subx, suby, nplanes), text.decode()
        assert text.startswith(b"grainprofile1\nframes 3 bit_depth %d planes %d\nplane 0\n" % (bd, nplanes))
        # two columns: the second clip is another draw of the same law
        other = R.sum_records(_clip_records(bd, ss, 3, w, h)[::-1][:2] + [R.empty_record()])
        two = format_profile(got, 3, bd, w, h, subx, suby, nplanes, synth=R.to_struct(other, RECORD))
        assert two == R.format_profile(want, 3, bd, w, h, subx, suby, nplanes, synth=other), two.decode()
        assert b"max_rho_diff " in two and b"sigma_ratio " in two
    # an all-zero record: every rho undefined, the bins with their counts
    zero = R.measure_frame(*([planes_of(9, 9, 8, "mono", 1)[1]] * 2), 8, 0, 0)
    text = format_profile(R.to_struct(zero, RECORD), 1, 8, 9, 9, 0, 0, 1)
    assert text == R.format_profile(zero, 1, 8, 9, 9, 0, 0, 1) and b"lag -3 -3 -\n" in text


def test_an_overflow_of_the_sum_is_refused():
    from grav1synth_amd.measure import RECORD, sum_records

    a, b = R.empty_record(), R.empty_record()
    a["s2"][1, 4] = np.uint64(2 ** 63)
    b["s2"][1, 4] = np.uint64(2 ** 63)
    with pytest.raises(OverflowError):
        R.sum_records([a, b])
    with pytest.raises(_lib.G1SError):
        sum_records(np.array([R.to_struct(a, RECORD), R.to_struct(b, RECORD)], RECORD))
    for v in (2 ** 62, -2 ** 62 - 1):
        a, b = R.empty_record(), R.empty_record()
        a["r"][2, 24] = b["r"][2, 24] = v
        with pytest.raises(_lib.G1SError):
            sum_records(np.array([R.to_struct(a, RECORD), R.to_struct(b, RECORD)], RECORD))
    b["r"][2, 24] = 0  # the largest sums that fit are taken
    a["n"][0, 0] = np.uint64(2 ** 64 - 2)
    b["n"][0, 0] = np.uint64(1)
    got = sum_records(np.array([R.to_struct(a, RECORD), R.to_struct(b, RECORD)], RECORD))
    assert int(got["n"][0, 0]) == 2 ** 64 - 1 and not R.mismatches(got, R.sum_records([a, b]), "edge")
    assert not R.mismatches(sum_records(np.zeros(0, RECORD)), R.empty_record(), "no records")


def test_record_and_options_have_the_headers_layout(tmp_path):
    from grav1synth_amd.measure import RECORD

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = ["n", "s1", "s2", "r"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "g1s_diff.h"', "int main(void) {",
           '  printf("%zu %zu\\n", sizeof(g1s_measure_record_t), sizeof(g1s_measure_opts_t));']
    src += [f'  printf("%zu\\n", offsetof(g1s_measure_record_t, {f}));' for f in fields]
    src += ['  printf("%zu\\n", offsetof(g1s_measure_opts_t, batch_frames));', "  return 0;", "}"]
    (tmp_path / "m.c").write_text("\n".join(src))
    subprocess.check_call([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "m.c"), "-o", str(tmp_path / "m")])
    out = subprocess.check_output([str(tmp_path / "m")], text=True).split()
    assert int(out[0]) == C.sizeof(_lib.G1SMeasureRecord) == RECORD.itemsize == 8 * (3 * 96 + 75)
    assert int(out[1]) == C.sizeof(_lib.G1SMeasureOpts)
    for f, off in zip(fields, out[2:6]):
        assert int(off) == getattr(_lib.G1SMeasureRecord, f).offset == RECORD.fields[f][1], f
    assert int(out[6]) == _lib.G1SMeasureOpts.batch_frames.offset


def test_no_gpu_means_the_meter_refuses():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from grav1synth_amd.measure import GrainMeter

    L = _lib.lib()
    assert not L.g1s_measure_new(10, None)
    assert L.g1s_last_global_error().decode() == "no HIP device available: measure has no CPU fallback"
    with pytest.raises(_lib.G1SError) as e:
        GrainMeter(10)
    assert "measure has no CPU fallback" in str(e.value)


def test_bad_bit_depth_and_options_are_refused_before_a_device_is_looked_for():
    L = _lib.lib()
    assert not L.g1s_measure_new(9, None)
    assert "8, 10 and 12" in L.g1s_last_global_error().decode()
    bad = _lib.G1SMeasureOpts(4, -1, 0)
    assert not L.g1s_measure_new(10, C.byref(bad))
    assert "struct_size" in L.g1s_last_global_error().decode()


def test_measure_and_check_refuse_like_diff(tmp_path, caplog):
    from grav1synth_amd import cli

    a, b, t, out = (str(tmp_path / n) for n in ("a.y4m", "b.y4m", "t.tbl", "out.txt"))
    for p in (a, b, t):
        open(p, "wb").write(b"x")

    def no(*_):
        return False

    with caplog.at_level(logging.INFO, logger="grav1synth"):
        assert cli.measure_command(a, b, a) == -1 and cli.measure_command(a, b, b + "/") == -1
        assert cli.check_command(a, b, t, t) == -1 and cli.check_command(a, b, t, "./" + a if not a.startswith("/") else a) == -1
        assert caplog.text.count(cli.SAME_AS_OUTPUT) == 4
        assert cli.measure_command(a, a, out) == -1 and cli.check_command(a, tmp_path.as_posix() + "//a.y4m", t, out) == -1
        assert caplog.text.count(cli.SAME_INPUTS) == 2
        open(out, "wb").write(b"kept")
        assert cli.measure_command(a, b, out, confirm=no) == -1 and cli.check_command(a, b, t, out, confirm=no) == -1
        assert caplog.text.count(cli.NOT_OVERWRITING) == 2
    assert open(out, "rb").read() == b"kept"
    args = cli.build_parser().parse_args(["check", a, b, "-g", t, "-o", out, "-y", "--clip-restricted", "--device", "2"])
    assert (args.command, args.grain, args.overwrite, args.clip_restricted, args.device) == ("check", t, True, True, 2)
    args = cli.build_parser().parse_args(["measure", a, b, "-o", out])
    assert (args.command, args.noisy, args.clean, args.overwrite) == ("measure", a, b, False)


# ------------------------------------------------------------------------------ the report code under the sanitizers
def _edge_records(ref, sign):
    """Two records of a kind whose entries sum to within a few hundred of the 64-bit edges, every entry another value; the
    signed fields alternate in sign (from `sign` on)."""
    a, b = ref.empty_record(), ref.empty_record()
    for name in a:
        k = np.arange(a[name].size, dtype=object).reshape(a[name].shape) % 97
        if a[name].dtype == np.uint64:
            a[name][...] = ((2 ** 64 - 1) - 3 * k).astype(np.uint64)
            b[name][...] = (2 * k).astype(np.uint64)
        else:
            s = np.where((k + sign) % 2 == 0, 1, -1).astype(object)
            a[name][...] = (s * ((2 ** 63 - 1) - 5 * k)).astype(np.int64)
            b[name][...] = (s * 4 * k).astype(np.int64)
    return [a, b]


def _report_sets():
    """(name, header fields, the records of the four kinds, the same for the second column or None)"""
    from tests import measure_s_ref as S
    from tests import measure_t_ref as T
    from tests import measure_x_ref as X

    def clip(seed):
        pairs = [planes_of(45, 31, 10, "420", seed=seed + k, amp=30 + 10 * k) for k in range(3)]
        return ([R.measure_frame(n, c, 10, 1, 1) for n, c in pairs], T.run_records(pairs, 10, 1, 1), [X.cross_frame(n, c, 10, 1, 1) for n, c in pairs],
                [S.scale_frame(n, c, 10, 1, 1) for n, c in pairs])

    refs = (R, T, X, S)
    yield "designed", dict(frames=3, pairs=2, bd=10, w=45, h=31, xdec=1, ydec=1, nplanes=3), clip(40), clip(50)
    yield "zero", dict(frames=0, pairs=0, bd=8, w=9, h=7, xdec=0, ydec=0, nplanes=1), tuple([m.empty_record()] for m in refs), None
    yield ("edge", dict(frames=2, pairs=2, bd=12, w=64, h=48, xdec=1, ydec=0, nplanes=3), tuple(_edge_records(m, 0) for m in refs),
           tuple(_edge_records(m, 1)[::-1] for m in refs))


def test_the_report_code_under_the_sanitizers(tmp_path):
    """csrc/measure_report.cpp with tests/measure_report_host.cpp, a program of its own: the sums and the four reports of three
    record sets against the restatements and against the library's bytes, every report into a buffer of exactly its size and
    refused by one a byte shorter, every sum refused on an overflowing pair."""
    from grav1synth_amd import measure as M
    from tests import measure_s_ref as S
    from tests import measure_t_ref as T
    from tests import measure_x_ref as X

    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "measure_report_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tests", "measure_report_host.cpp"), os.path.join(ROOT, "grav1synth_amd", "csrc", "measure_report.cpp")]
    # (the sanitizer's runtime inside the program where the compiler can do that: it then starts under any preloaded library)
    if subprocess.call(cmd + ["-static-libasan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    refs, dtypes = (R, T, X, S), (M.RECORD, M.TRECORD, M.XRECORD, M.SRECORD)
    sums = (M.sum_records, M.sum_temporal_records, M.sum_cross_records, M.sum_scale_records)
    for name, g, first, second in _report_sets():
        columns = [first] + ([second] if second is not None else [])
        blob = np.array([g["frames"], g["pairs"], g["bd"], g["w"], g["h"], g["xdec"], g["ydec"], g["nplanes"]] + [len(k) for k in first] +
                        [second is not None], "<u8").tobytes()
        structs = [[np.array([m.to_struct(r, dt) for r in recs], dt) for m, dt, recs in zip(refs, dtypes, col)] for col in columns]
        blob += b"".join(s.tobytes() for col in structs for s in col)
        path = tmp_path / f"{name}.bin"
        path.write_bytes(blob)
        p = subprocess.run([str(exe), str(path)], env=env, capture_output=True, timeout=600)
        assert p.returncode == 0, (name, p.stderr[-3000:].decode())
        got, rest = {}, p.stdout
        for kind in ("plain", "temporal", "cross", "scales"):
            head, rest = rest.split(b"\n", 1)
            word, k, size = head.split()
            assert (word, k) == (b"report", kind.encode()), head
            got[kind], rest = rest[:int(size)], rest[int(size):]
        assert rest == b"refusals ok\n", rest
        # the restatements, from their own sums
        t = [[m.sum_records(recs) for m, recs in zip(refs, col)] for col in columns]
        syn = t[1] if second is not None else [None] * 4
        geom = (g["bd"], g["w"], g["h"], g["xdec"], g["ydec"])
        want = dict(plain=R.format_profile(t[0][0], g["frames"], *geom, g["nplanes"], synth=syn[0]),
                    temporal=T.format_temporal(t[0][1], g["pairs"], *geom, g["nplanes"], synth=syn[1]),
                    cross=X.format_cross(t[0][2], g["frames"], *geom, synth=syn[2]),
                    scales=S.format_scales(t[0][0], t[0][3], g["frames"], g["bd"], g["nplanes"], synth=syn[0], ssynth=syn[3]))
        # the library's bytes, from its own sums
        lt = [[f(s) for f, s in zip(sums, col)] for col in structs]
        ls = lt[1] if second is not None else [None] * 4
        lib = dict(plain=M.format_profile(lt[0][0], g["frames"], *geom, g["nplanes"], synth=ls[0]),
                   temporal=M.format_temporal_profile(lt[0][1], g["pairs"], *geom, g["nplanes"], synth=ls[1]),
                   cross=M.format_cross_profile(lt[0][2], g["frames"], *geom, synth=ls[2]),
                   scales=M.format_scale_profile(lt[0][0], lt[0][3], g["frames"], g["bd"], g["nplanes"], synth=ls[0], ssynth=ls[3]))
        for kind in got:
            assert got[kind] == want[kind], (name, kind, got[kind][:600], want[kind][:600])
            assert got[kind] == lib[kind], (name, kind)
        assert len(got["plain"]) > 100 and got["cross"].startswith(b"graincross1\n")
