"""The cross meter on the device against tests/measure_x_ref.py: every field of every cross record with array_equal, every
report byte for byte; the ordinary records of the same run against tests/measure_ref.py.  There is no tolerance anywhere."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import content as CT
from tests import grain_ref as G
from tests import measure_ref as R
from tests import measure_t_ref as T
from tests import measure_x_ref as X
from tests import views as V
from tests.test_gpu_grain import _to_dev
from tests.test_measure_cpu import SUBSAMPLINGS, planes_of
from tests.test_measure_x_cpu import moved_pair, negative_boxes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW, TH = 64, 128  # km_measure_x's chroma tile


@pytest.fixture(scope="module")
def meters():
    from grav1synth_amd.measure import GrainMeter

    made = {}

    def get(bd, **kw):
        key = (bd, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = GrainMeter(bd, cross=True, **kw)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def assert_records(got, wants, what):
    assert len(got) == len(wants), f"{what}: {len(got)} cross records, want {len(wants)}"
    for k, want in enumerate(wants):
        for name, _dt, _size in X.FIELDS:
            assert np.array_equal(np.asarray(got[k][name]), want[name]), "\n".join(X.mismatches(got[k], want, f"{what}, record {k}"))


def assert_ordinary(got, pairs, bd, subx, suby, what):
    assert len(got) == len(pairs), what
    for k, (noisy, clean) in enumerate(pairs):
        bad = R.mismatches(got[k], R.measure_frame(noisy, clean, bd, subx, suby), f"{what}, pair {k}")
        assert not bad, "\n".join(bad)


def check_pairs(m, pairs, bd, subx, suby, what, dev=True):
    """The pairs through the meter: the cross and the ordinary records against the restatements.  Returns the reference records."""
    for noisy, clean in pairs:
        m.measure(_to_dev(noisy, bd) if dev else noisy, _to_dev(clean, bd) if dev else clean, subx, suby)
    wants = [X.cross_frame(noisy, clean, bd, subx, suby) for noisy, clean in pairs]
    assert_records(m.finish_cross(), wants, what)
    assert_ordinary(m.finish(), pairs, bd, subx, suby, what)
    return wants


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444"])
def test_formats_on_plane_distinct_content(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    pairs = [CT.make_frames("distinct", 208, 136, bd, subx, suby, frame=k) for k in range(3)]
    wants = check_pairs(meters(bd), pairs, bd, subx, suby, f"{bd} bit {ss}")
    w = wants[0]
    assert w["x"][0].any(), "x[0] is non-zero"
    assert not np.array_equal(w["c"][0], w["c"][1]) and not np.array_equal(w["c"][0], w["c"][2]) and not np.array_equal(w["c"][1], w["c"][2])


# chroma sizes; each is reached from an even and, where the decimation allows, an odd luma size
CHROMA_SIZES = [(1, 1), (2, 3), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW + 2, 2 * TH + 1)]


@pytest.mark.parametrize("csize", CHROMA_SIZES)
def test_sizes_round_the_tile_from_even_and_odd_luma_sizes_in_batches_of_1_2_and_5(meters, csize):
    cw, ch = csize
    for (bd, ss), n in zip(((8, "420"), (10, "422"), (12, "444")), (5, 2, 1)):
        subx, suby = SUBSAMPLINGS[ss]
        lumas = {(cw << subx, ch << suby), ((cw << subx) - subx, (ch << suby) - suby)}
        for w, h in sorted(lumas):
            pairs = [planes_of(w, h, bd, ss, seed=2 + k) for k in range(n)]
            assert pairs[0][1][1].shape == (ch, cw)
            check_pairs(meters(bd), pairs, bd, subx, suby, f"chroma {cw}x{ch} from luma {w}x{h} {bd} bit {ss}")


def test_a_moved_residual_for_each_of_the_25_offsets_one_a_pair(meters):
    """150 x 140 at 4:4:4 is 3 x 2 tiles, so the offsets cross tile borders in both directions."""
    m = meters(8)
    for what, j in (("cr", 2), ("luma", 0)):
        made = [moved_pair(i, 150, 140, 3, what=what) for i in range(25)]
        wants = check_pairs(m, [(n, c) for n, c, _e in made], 8, 0, 0, f"moved {what}")
        for i, want in enumerate(wants):
            assert int(want["c"][j, i]) == made[i][2] and int(np.argmax(want["c"][j])) == i


def test_negative_rounding_boxes_tiled_over_a_plane(meters):
    for w, h in ((2 * TW + 6, 2 * TH + 10), (2 * TW + 5, 2 * TH + 9)):
        noisy, clean = negative_boxes(w, h, 10)
        wants = check_pairs(meters(10), [(noisy, clean)], 10, 1, 1, f"negative boxes {w}x{h}")
        wrong = X.cross_frame(noisy, clean, 10, 1, 1, truncate=True)
        assert wants[0]["v"][0].any() and not np.array_equal(wants[0]["x"][0], wrong["x"][0]), "a truncating division would show"


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_adversarial_bins(meters, bd):
    w, h, step = 300, 270, 1 << (bd - 5)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    cases = {
        "one intensity": np.full((h, w), 11 * step + 3),
        "two bins alternating sample by sample on the chroma grid": np.where(((xs >> 1) + (ys >> 1)) & 1, 7 * step, 8 * step),
        "a ramp through all 32": (((xs >> 1) + 3 * (ys >> 1)) % 32) * step + (ys % step),
    }
    for what, luma in cases.items():
        noisy, clean = planes_of(w, h, bd, "420", seed=bd, amp=60)
        d = noisy[0].astype(np.int64) - clean[0].astype(np.int64)
        clean[0] = luma.astype(clean[0].dtype)
        noisy[0] = np.clip(luma + d, 0, (1 << bd) - 1).astype(clean[0].dtype)
        wants = check_pairs(meters(bd), [(noisy, clean)], bd, 1, 1, f"{bd} bit, {what}")
        bins = np.count_nonzero(wants[0]["n"][0])
        assert bins == (1 if what == "one intensity" else 32 if what.startswith("a ramp") else 2), what
        if bins == 2:
            k = R.intensity(clean, 1, 1, 1) >> (bd - 5)
            assert (k[:, 1:] != k[:, :-1]).all() and (k[1:] != k[:-1]).all()


@pytest.mark.parametrize("ss", ["420", "444"])
def test_extremes_at_12_bits(meters, ss):
    """Every residual is +4095 or -4095.  All of one sign: |L| = 4095 everywhere and every 32-bit sum of a wave (32 rows of
    products of 2^24) at its ceiling.  Sign by (x + y) parity on luma: on 4:4:4 L alternates between the extremes; the 4:2:0
    boxes sum to 0, also the clamped ones along the edges of an odd-sized frame (twice +4095, twice -4095), but for the corner
    box, which is one sample four times: +-16380, L = +-4095."""
    bd = 12
    subx, suby = SUBSAMPLINGS[ss]
    w, h = 2 * (TW << subx) + 3, (TH << suby) + 61
    shapes = [(h, w)] + [((h + suby) >> suby, (w + subx) >> subx)] * 2
    top = [np.full(s, 4095, np.uint16) for s in shapes]
    zero = [np.zeros(s, np.uint16) for s in shapes]
    wants = check_pairs(meters(bd), [(top, zero), (zero, top), ([top[0], zero[1], top[2]], [zero[0], top[1], zero[2]])], bd, subx, suby, "one sign")
    n = shapes[1][0] * shapes[1][1]
    for rec, signs in zip(wants, ((1, 1, 1), (1, 1, 1), (-1, 1, -1))):
        for j in range(3):
            assert int(rec["c"][j, 12]) == signs[j] * 4095 * 4095 * n and abs(int(rec["c"][j, 12])) > 2 ** 32
            assert int(rec["u"][j].sum()) == int(rec["v"][j].sum()) == 4095 * 4095 * n
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    par = ((xs + ys) & 1) == 1
    a = [np.where(par[:s[0], :s[1]], 4095, 0).astype(np.uint16) for s in shapes]
    b = [np.where(par[:s[0], :s[1]], 0, 4095).astype(np.uint16) for s in shapes]
    wants = check_pairs(meters(bd), [(a, b), (b, a)], bd, subx, suby, "sign by parity")
    if ss == "420":
        L = X.luma_at_chroma(a[0].astype(np.int64) - b[0], shapes[1][1], shapes[1][0], 1, 1)
        assert np.count_nonzero(L) == 1 and abs(int(L[-1, -1])) == 4095
        # three samples of a box against one: the boxes sum to -8190 and +8190, L = -2047 (a truncating division: -2048 + 1) and 2048
        one = (((xs & 1) == 1) & ((ys & 1) == 1)) ^ ((((xs >> 1) + (ys >> 1)) & 1) == 1)
        a[0], b[0] = np.where(one, 4095, 0).astype(np.uint16), np.where(one, 0, 4095).astype(np.uint16)
        check_pairs(meters(bd), [(a, b)], bd, subx, suby, "three to one")
        L = X.luma_at_chroma(a[0].astype(np.int64) - b[0], shapes[1][1], shapes[1][0], 1, 1)
        assert {-2047, 2048} <= set(np.unique(L[:-1, :-1]).tolist())


@pytest.mark.parametrize("bd,ss", [(8, "420"), (10, "422"), (12, "444")])
@pytest.mark.parametrize("which", ["noisy", "clean", "both"])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(meters, bd, ss, which):
    subx, suby = SUBSAMPLINGS[ss]
    isz = 1 if bd == 8 else 2
    pairs = [planes_of(147, 139, bd, ss, seed=4 + k, amp=200) for k in range(3)]
    guards, keep = [], []
    m = meters(bd)
    for k, ((extra, base), pair) in enumerate(zip(((6, 2), (34, 14), (130, 250)), pairs)):
        devs = []
        for j, planes in enumerate(pair):
            if which != "both" and which != ("noisy", "clean")[j]:
                devs.append(_to_dev(planes, bd))
                continue
            dev = []
            for c, p in enumerate(planes):
                view, guard = V.device_view(p, pitch_bytes=p.shape[1] * isz + extra * isz, base_offset_bytes=(base + 2 * c * (j + 1)) % 256 & ~(isz - 1),
                                            fill="random" if k & 1 else "max", max_code=(1 << bd) - 1, seed=10 * k + c)
                dev.append(view)
                guards.append(guard)
            devs.append(dev)
        keep.append(devs)
        m.measure(devs[0], devs[1], subx, suby)
    assert_records(m.finish_cross(), [X.cross_frame(n, c, bd, subx, suby) for n, c in pairs], f"views {bd} bit {ss} {which}")
    assert_ordinary(m.finish(), pairs, bd, subx, suby, "views")
    for g in guards:
        g.assert_unchanged("a view")


def test_host_pinned_and_device_frames_in_one_batch():
    import torch

    from grav1synth_amd.measure import GrainMeter

    bd, (subx, suby) = 10, (1, 1)
    m = GrainMeter(bd, batch_frames=8, cross=True)
    pairs, keep = [], []
    for k in range(7):
        noisy, clean = planes_of(150, 90, bd, "420", seed=30 + k, amp=90)
        pairs.append((noisy, clean))
        pair = []
        for kind, planes in zip((k % 3, (k // 3 + k) % 3), (noisy, clean)):
            if kind == 0:
                pair.append(planes)
            elif kind == 1:
                pair.append(_to_dev(planes, bd))
            else:
                pair.append([torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes])
        keep.append(pair)
        m.measure(pair[0], pair[1], subx, suby, async_host=True)
    assert_records(m.finish_cross(), [X.cross_frame(n, c, bd, subx, suby) for n, c in pairs], "mixed")
    assert_ordinary(m.finish(), pairs, bd, subx, suby, "mixed")
    m.close()


def test_batch_frames_1_2_n_and_n_plus_1_and_a_capacity_one_short():
    from grav1synth_amd.measure import XRECORD, GrainMeter

    bd, n = 10, 4
    pairs = [planes_of(150, 90, bd, "420", seed=30 + k, amp=90) for k in range(n)]
    wants = [X.cross_frame(a, b, bd, 1, 1) for a, b in pairs]
    for batch in (1, 2, n, n + 1):
        m = GrainMeter(bd, batch_frames=batch, cross=True)
        for noisy, clean in pairs:
            m.measure(noisy, clean, 1, 1)
        # a buffer one record short: G1S_ERR_CAPACITY, the count, and nothing lost; not sticky
        cnt = C.c_size_t()
        small = np.zeros(n - 1, XRECORD)
        assert m._L.g1s_measure_finish_cross(m._h, small.ctypes.data, n - 1, C.byref(cnt)) == _lib.G1S_ERR_CAPACITY and cnt.value == n
        with pytest.raises(_lib.G1SError):
            m.finish_cross(cap=n - 1)
        assert_ordinary(m.finish(), pairs, bd, 1, 1, f"batch_frames {batch}")
        assert_records(m.finish_cross(), wants, f"batch_frames {batch}")
        assert len(m.finish_cross()) == 0 and len(m.finish()) == 0
        m.close()


def test_a_geometry_change_in_mid_queue_and_a_one_plane_pair_between_three_plane_pairs():
    from grav1synth_amd.measure import GrainMeter

    bd = 8
    m = GrainMeter(bd, batch_frames=8, cross=True)
    a = [planes_of(70, 50, bd, "420", seed=60 + k, amp=25) for k in range(3)]
    b = [planes_of(33, 141, bd, "444", seed=70 + k) for k in range(2)]
    mono = planes_of(33, 141, bd, "mono", seed=80)
    order = [(a[0], 1, 1), (a[1], 1, 1), (b[0], 0, 0), (mono, 0, 0), (b[1], 0, 0), (a[2], 1, 1)]
    for k, ((noisy, clean), subx, suby) in enumerate(order):
        m.measure(_to_dev(noisy, bd) if k & 1 else noisy, clean, subx, suby)
    got = m.finish_cross()
    assert_records(got, [X.cross_frame(p[0], p[1], bd, sx, sy) for p, sx, sy in order], "geometry changes")
    assert not any(got[3][name].any() for name, _dt, _size in X.FIELDS), "a one-plane pair has a zero record in its place"
    ordinary = m.finish()
    for k, ((noisy, clean), subx, suby) in enumerate(order):
        assert not R.mismatches(ordinary[k], R.measure_frame(noisy, clean, bd, subx, suby), f"pair {k}")
    m.close()


def test_modes_3_equal_a_temporal_and_a_plain_meter_and_the_three_finish_calls_interleave():
    from grav1synth_amd.measure import GrainMeter

    bd = 10
    pairs = [planes_of(131, 77, bd, "420", seed=90 + k, amp=70) for k in range(7)]
    xwant = [X.cross_frame(a, b, bd, 1, 1) for a, b in pairs]
    plain, temporal = GrainMeter(bd, batch_frames=3), GrainMeter(bd, batch_frames=3, temporal=True)
    for noisy, clean in pairs:
        plain.measure(noisy, clean, 1, 1)
        temporal.measure(noisy, clean, 1, 1)
    ordinary, trecords = plain.finish(), temporal.finish_temporal()
    assert_ordinary(ordinary, pairs, bd, 1, 1, "plain")
    plain.close(), temporal.close()
    m = GrainMeter(bd, batch_frames=3, temporal=True, cross=True)
    for noisy, clean in pairs:
        m.measure(_to_dev(noisy, bd), clean, 1, 1)
    assert m.finish_temporal().tobytes() == trecords.tobytes() and m.finish().tobytes() == ordinary.tobytes()
    assert_records(m.finish_cross(), xwant, "modes 3")
    m.cut()
    # interleaved: each call keeps the others' records, and the run goes on over a hand-over
    twant = T.run_records(pairs, bd, 1, 1)
    m.measure(*pairs[0], 1, 1), m.measure(_to_dev(pairs[1][0], bd), _to_dev(pairs[1][1], bd), 1, 1)
    assert_records(m.finish_cross(), xwant[:2], "cross first")
    m.measure(*pairs[2], 1, 1)
    got_t = m.finish_temporal()
    assert len(got_t) == 2 and not T.mismatches(got_t[0], twant[0], "t0") and not T.mismatches(got_t[1], twant[1], "t1")
    m.measure(*pairs[3], 1, 1)
    m.cut()
    m.measure(*pairs[4], 1, 1)
    assert_ordinary(m.finish(), pairs[:5], bd, 1, 1, "ordinary last")
    assert_records(m.finish_cross(), xwant[2:5], "cross after the others")
    got_t = m.finish_temporal()
    assert len(got_t) == 1 and not T.mismatches(got_t[0], twant[2], "t2")
    m.close()


def test_a_plain_and_a_temporal_meter_refuse_finish_cross_and_go_on_working():
    from grav1synth_amd.measure import GrainMeter

    bd = 8
    for temporal in (False, True):
        m = GrainMeter(bd, temporal=temporal)
        noisy, clean = planes_of(70, 50, bd, "420", seed=1)
        m.measure(noisy, clean, 1, 1)
        with pytest.raises(_lib.G1SError) as e:
            m.finish_cross()
        assert e.value.code == -1 and "g1s_measure_new_modes" in str(e.value)
        n = C.c_size_t(7)
        assert m._L.g1s_measure_finish_cross(m._h, None, 0, C.byref(n)) == -1
        m.measure(clean, noisy, 1, 1)
        assert_ordinary(m.finish(), [(noisy, clean), (clean, noisy)], bd, 1, 1, "after the refusals")
        assert m.cross_kernel_times() == (0.0, 0)
        m.close()


@pytest.mark.parametrize("w,h", [(65536, 4), (4, 65536)])
def test_limits_65536_samples_a_side_and_one_over(meters, w, h):
    from grav1synth_amd.measure import GrainMeter

    """4:2:0 12-bit; the last column (row) of every plane holds residuals of +4095 and -4095 in turn."""
    bd = 12
    rng = np.random.default_rng([w, h])
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    clean = [rng.integers(0, 4096, s).astype(np.uint16) for s in shapes]
    noisy = [np.clip(c.astype(np.int64) + rng.integers(-300, 301, c.shape), 0, 4095).astype(np.uint16) for c in clean]
    for c, n in zip(clean, noisy):
        edge = (slice(None), -1) if w > h else (-1, slice(None))
        sign = (np.arange(c[edge].size) & 1).astype(bool)
        c[edge], n[edge] = np.where(sign, 0, 4095), np.where(sign, 4095, 0)
    check_pairs(meters(bd), [(noisy, clean)], bd, 1, 1, f"{w}x{h}")
    over = [np.zeros((h + (h > w), w + (w > h)), np.uint16)] + [np.zeros(((h + (h > w) + 1) // 2, (w + (w > h) + 1) // 2), np.uint16)] * 2
    m = GrainMeter(bd, cross=True)
    try:
        with pytest.raises(_lib.G1SError) as e:
            m.measure(_to_dev(over, bd), _to_dev(over, bd), 1, 1)
    finally:
        m.close()
    assert e.value.code == -1 and "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)" in str(e.value)


def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "grav1synth_amd", *args], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT,
                          stdin=subprocess.DEVNULL)


def test_measure_and_check_cross_on_files(tmp_path):
    """`measure --cross`, then `check --cross --temporal` with a table whose Cb luma coefficient is non-zero and whose Cr luma
    coefficient is zero: all reports byte for byte what the restatements make, the rendering from tests/grain_ref.py."""
    from grav1synth_amd.diff import format_tbl
    from grav1synth_amd.ingest import write_y4m
    from grav1synth_amd.measure import check_y4m_files, measure_y4m_files
    from grav1synth_amd.tbl import GrainTable, parse_tbl

    bd, w, h, n = 10, 208, 136, 3
    made = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(n)]
    src, den = [p[0] for p in made], [p[1] for p in made]
    a, b, tbl, out, tout, xout = (tmp_path / name for name in ("src.y4m", "den.y4m", "t.tbl", "fit.txt", "tfit.txt", "xfit.txt"))
    fps = Fraction(24, 1)
    write_y4m(str(a), src, bd, 1, 1, fps)
    write_y4m(str(b), den, bd, 1, 1, fps)
    pairs = list(zip(src, den))
    profile = R.format_profile(R.sum_records([R.measure_frame(s, d, bd, 1, 1) for s, d in pairs]), n, bd, w, h, 1, 1, 3)
    xrec_s = X.sum_records([X.cross_frame(s, d, bd, 1, 1) for s, d in pairs])
    p = _run("measure", str(a), str(b), "-o", str(out), "--cross", str(xout))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Measured {n} frames" in p.stderr and f"wrote cross profile to {xout}" in p.stderr
    assert out.read_bytes() == profile and xout.read_bytes() == X.format_cross(xrec_s, n, bd, w, h, 1, 1)
    # both extra reports in one run (the outputs exist by now: `check ... -y` below covers all three)
    assert measure_y4m_files(str(a), str(b), str(out), temporal_output=str(tout), cross_output=str(xout), batch_frames=2) == (n, False)
    twant = T.format_temporal(T.sum_records(T.run_records(pairs, bd, 1, 1)), n - 1, bd, w, h, 1, 1, 3)
    assert out.read_bytes() == profile and xout.read_bytes() == X.format_cross(xrec_s, n, bd, w, h, 1, 1) and tout.read_bytes() == twant
    # without --cross: the bytes of the existing entry points
    o2, t2 = tmp_path / "p2.txt", tmp_path / "t2.txt"
    assert measure_y4m_files(str(a), str(b), str(o2), temporal_output=str(t2)) == (n, False)
    assert o2.read_bytes() == profile and t2.read_bytes() == twant
    assert measure_y4m_files(str(a), str(b), str(o2)) == (n, False) and o2.read_bytes() == profile

    # the table: `diff`'s, with the luma coefficient of Cb set and that of Cr cleared
    p = _run("diff", str(a), str(b), "-o", str(tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    segs = []
    for s in parse_tbl(tbl.read_bytes()):
        at = 2 * s.ar_coeff_lag * (s.ar_coeff_lag + 1)
        cb, cr = list(s.ar_coeffs_cb), list(s.ar_coeffs_cr)
        cb[at], cr[at] = 48, 0
        segs.append(dataclasses.replace(s, ar_coeffs_cb=cb, ar_coeffs_cr=cr))
    tbl.write_bytes(format_tbl(segs))
    p = _run("check", str(a), str(b), "-g", str(tbl), "-o", str(out), "--cross", str(xout), "--temporal", str(tout), "-y")
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Checked {n} frames" in p.stderr and f"wrote cross profile to {xout}" in p.stderr and f"wrote temporal profile to {tout}" in p.stderr
    table = GrainTable(parse_tbl(tbl.read_bytes()))
    rendered = []
    for k in range(n):
        seg = table.segment_for(k * 10000000 * fps.denominator // fps.numerator)
        assert seg is not None
        rendered.append(G.add_noise(den[k], seg, bd, 1, 1))
    rec_r = R.sum_records([R.measure_frame(rendered[k], den[k], bd, 1, 1) for k in range(n)])
    fit = R.format_profile(R.sum_records([R.measure_frame(s, d, bd, 1, 1) for s, d in pairs]), n, bd, w, h, 1, 1, 3, synth=rec_r)
    xrec_r = X.sum_records([X.cross_frame(rendered[k], den[k], bd, 1, 1) for k in range(n)])
    xwant = X.format_cross(xrec_s, n, bd, w, h, 1, 1, synth=xrec_r)
    tfit = T.format_temporal(T.sum_records(T.run_records(pairs, bd, 1, 1)), n - 1, bd, w, h, 1, 1, 3,
                             synth=T.sum_records(T.run_records(list(zip(rendered, den)), bd, 1, 1)))
    assert out.read_bytes() == fit and tout.read_bytes() == tfit
    assert xout.read_bytes() == xwant, xout.read_text()
    tm = X.terms_f64(n, w, h, 1, 1)
    beta = [X.profile(xrec_r, j, tm) for j in (0, 1)]
    assert beta[0]["has_beta"] and beta[1]["has_beta"] and "%.4f" % beta[0]["beta"] != "%.4f" % beta[1]["beta"], "the rendered column tells Cb from Cr"
    # small groups, and without --cross the bytes of the existing entry points
    o2, t2, x2 = tmp_path / "fit2.txt", tmp_path / "tfit2.txt", tmp_path / "xfit2.txt"
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2), batch_frames=2, cross_output=str(x2)) == (n, False)
    assert o2.read_bytes() == fit and x2.read_bytes() == xwant
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2), temporal_output=str(t2)) == (n, False)
    assert o2.read_bytes() == fit and t2.read_bytes() == tfit
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2)) == (n, False) and o2.read_bytes() == fit
