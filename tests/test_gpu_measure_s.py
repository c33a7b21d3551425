"""The scales meter on the device against tests/measure_s_ref.py: every field of every scale record with array_equal, every
report byte for byte; the other records of the same run against their restatements or against a meter without scales.  There
is no tolerance anywhere."""
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
from tests import measure_ref as R
from tests import measure_s_ref as S
from tests import views as V
from tests.test_gpu_grain import _to_dev
from tests.test_measure_cpu import SUBSAMPLINGS, planes_of
from tests.test_measure_s_cpu import alternating_pair, checkerboard_pair, extremes_pair, floor_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW, TH, SW = 64, 128, 512  # km_measure's tile; the strip of a workgroup of km_measure_s


@pytest.fixture(scope="module")
def meters():
    from grav1synth_amd.measure import GrainMeter

    made = {}

    def get(bd, **kw):
        key = (bd, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = GrainMeter(bd, scales=True, **kw)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def assert_records(got, wants, what):
    assert len(got) == len(wants), f"{what}: {len(got)} scale records, want {len(wants)}"
    for k, want in enumerate(wants):
        for name, _dt in S.FIELDS:
            assert np.array_equal(np.asarray(got[k][name]), want[name]), "\n".join(S.mismatches(got[k], want, f"{what}, record {k}"))


def assert_ordinary(got, pairs, bd, subx, suby, what):
    assert len(got) == len(pairs), what
    for k, (noisy, clean) in enumerate(pairs):
        bad = R.mismatches(got[k], R.measure_frame(noisy, clean, bd, subx, suby), f"{what}, pair {k}")
        assert not bad, "\n".join(bad)


def check_pairs(m, pairs, bd, subx, suby, what, dev=True):
    """The pairs through the meter: the scale and the ordinary records against the restatements.  Returns the reference records."""
    for noisy, clean in pairs:
        m.measure(_to_dev(noisy, bd) if dev else noisy, _to_dev(clean, bd) if dev else clean, subx, suby)
    wants = [S.scale_frame(noisy, clean, bd, subx, suby) for noisy, clean in pairs]
    assert_records(m.finish_scales(), wants, what)
    assert_ordinary(m.finish(), pairs, bd, subx, suby, what)
    return wants


# plane sizes: few or no boxes, round 32, round the tile, several tiles, round the strip of a workgroup
PLANE_SIZES = [(1, 1), (31, 33), (32, 32), (33, 31), (63, 64), (TW, TH), (TW + 1, TH + 1), (96, 160), (130, 257), (SW + 1, 40)]


@pytest.mark.parametrize("size", PLANE_SIZES)
def test_plane_sizes_as_luma_and_as_chroma_from_even_and_odd_luma_sizes(meters, size):
    pw, ph = size
    for (bd, ss), n in zip(((8, "420"), (10, "422"), (12, "444")), (3, 2, 1)):
        subx, suby = SUBSAMPLINGS[ss]
        # the plane as chroma: from an even and, where the decimation allows, an odd luma size
        lumas = {(pw << subx, ph << suby), ((pw << subx) - subx, (ph << suby) - suby)}
        for w, h in sorted(lumas):
            pairs = [planes_of(w, h, bd, ss, seed=2 + k, amp=(1 << bd) // 3) for k in range(n)]
            assert pairs[0][1][1].shape == (ph, pw)
            wants = check_pairs(meters(bd), pairs, bd, subx, suby, f"chroma {pw}x{ph} from luma {w}x{h} {bd} bit {ss}")
            for k in range(1, 6):
                assert int(wants[0]["n"][1, k - 1].sum()) == (pw >> k) * (ph >> k), "zeros where there are no boxes"
    # the plane as luma, every depth
    for bd in (8, 10, 12):
        check_pairs(meters(bd), [planes_of(pw, ph, bd, "420", seed=9)], bd, 1, 1, f"luma {pw}x{ph} {bd} bit")
    check_pairs(meters(8), [planes_of(pw, ph, 8, "mono", seed=9)], 8, 0, 0, f"one plane {pw}x{ph}")


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_checkerboard_of_each_scale(meters, bd):
    w, h = 2 * TW + 32, 2 * TH + 64
    for ss in ("444", "420"):
        subx, suby = SUBSAMPLINGS[ss]
        pairs = [checkerboard_pair(w, h, bd, ss, m, 5 + m) for m in range(6)]
        wants = check_pairs(meters(bd), pairs, bd, subx, suby, f"checkerboards {bd} bit {ss}")
        for m, want in enumerate(wants):
            for k in range(1, 6):
                n = (w >> k) * (h >> k)
                assert int(want["s2"][0, k - 1].sum()) == (n * (4 ** k * (5 + m)) ** 2 if k <= m else 0), (m, k)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_boxes_in_a_bin_no_sample_is_in_and_boxes_on_a_bins_edge(meters, bd):
    w, h = 2 * TW + 6, TH + 34
    for ss, on in (("444", "luma"), ("420", "luma"), ("420", "chroma"), ("422", "chroma")):
        subx, suby = SUBSAMPLINGS[ss]
        noisy, clean = alternating_pair(w, h, bd, ss, seed=bd, on=on)
        want = check_pairs(meters(bd), [(noisy, clean)], bd, subx, suby, f"alternating {ss} {on} {bd} bit")[0]
        c = 0 if on == "luma" else 1
        assert all(np.flatnonzero(want["n"][c, k]).tolist() == [12] for k in range(5))
        assert not np.array_equal(want["n"], S.scale_frame(noisy, clean, bd, subx, suby, bin_by_sample=True)["n"])
    for kind in ("three", "half"):
        noisy, clean = floor_pair(w, h, bd, "420", seed=bd, kind=kind)
        want = check_pairs(meters(bd), [(noisy, clean)], bd, 1, 1, f"floor {kind} {bd} bit")[0]
        assert all(np.flatnonzero(want["n"][0, k]).tolist() == [8] for k in range(5))
        assert not np.array_equal(want["n"][0], S.scale_frame(noisy, clean, bd, 1, 1, rounded_mean=True)["n"][0])
        if kind == "half":
            assert not np.array_equal(want["n"][1], S.scale_frame(noisy, clean, bd, 1, 1, luma_sum=True)["n"][1])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_adversarial_bins(meters, bd):
    """One intensity (a reduction a round), and a ramp whose boxes of every scale spread over many bins."""
    w, h, step = 300, 270, 1 << (bd - 5)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    cases = {"one intensity": np.full((h, w), 11 * step + 3), "a ramp": (((xs >> 1) + 3 * (ys >> 1)) % 32) * step + (ys % step),
             "bins by 2 x 2 box": ((5 * (xs >> 1) + 11 * (ys >> 1)) % 32) * step}
    for what, luma in cases.items():
        noisy, clean = planes_of(w, h, bd, "420", seed=bd, amp=60)
        d = noisy[0].astype(np.int64) - clean[0].astype(np.int64)
        clean[0] = luma.astype(clean[0].dtype)
        noisy[0] = np.clip(luma + d, 0, (1 << bd) - 1).astype(clean[0].dtype)
        want = check_pairs(meters(bd), [(noisy, clean)], bd, 1, 1, f"{bd} bit, {what}")[0]
        assert np.count_nonzero(want["n"][0, 0]) == (1 if what == "one intensity" else 32), what


def test_extremes_at_12_bits_need_the_square_in_64_bits(meters):
    top, zero = extremes_pair(128, 256)
    mixed = ([top[0], zero[1], top[2]], [zero[0], top[1], zero[2]])
    wants = check_pairs(meters(12), [(top, zero), (zero, top), mixed], 12, 1, 1, "+-4095 everywhere")
    wrong = S.scale_frame(top, zero, 12, 1, 1, square32=True)
    assert int(wants[0]["s2"][0, 4].sum()) == 32 * (1024 * 4095) ** 2 and not np.array_equal(wants[0]["s2"], wrong["s2"])
    assert int(wants[1]["s1"][0, 4].sum()) == -32 * 1024 * 4095


@pytest.mark.parametrize("bd,ss", [(8, "420"), (10, "422"), (12, "444")])
def test_views_with_a_pitch_and_an_odd_base_equal_the_aligned_path(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    isz = 1 if bd == 8 else 2
    pairs = [planes_of(147, 139, bd, ss, seed=4 + k, amp=200) for k in range(3)]
    m = meters(bd)
    for noisy, clean in pairs:  # contiguous tensors: rows of 147 samples, so both paths already take part
        m.measure(_to_dev(noisy, bd), _to_dev(clean, bd), subx, suby)
    aligned = m.finish_scales()
    m.finish()
    guards, keep = [], []
    # (pitch extra, base): a pitch that keeps every row 16-byte aligned on an aligned base; odd pitches; an odd base
    for k, ((extra, base), pair) in enumerate(zip(((13 if isz == 1 else 10, 0), (34, 14), (131, 250)), pairs)):
        devs = []
        for j, planes in enumerate(pair):
            dev = []
            for c, p in enumerate(planes):
                pitch = p.shape[1] * isz + extra * isz
                if k == 0:
                    pitch = (pitch + 15) & ~15
                view, guard = V.device_view(p, pitch_bytes=pitch, base_offset_bytes=(base + 2 * c * (j + 1)) % 256 & ~(isz - 1),
                                            fill="random" if k & 1 else "max", max_code=(1 << bd) - 1, seed=10 * k + c)
                dev.append(view)
                guards.append(guard)
            devs.append(dev)
        keep.append(devs)
        m.measure(devs[0], devs[1], subx, suby)
    got = m.finish_scales()
    assert got.tobytes() == aligned.tobytes(), "the unaligned path against the aligned one"
    assert_records(got, [S.scale_frame(n, c, bd, subx, suby) for n, c in pairs], f"views {bd} bit {ss}")
    assert_ordinary(m.finish(), pairs, bd, subx, suby, "views")
    for g in guards:
        g.assert_unchanged("a view")


def test_host_pinned_and_device_frames_in_one_batch():
    import torch

    from grav1synth_amd.measure import GrainMeter

    bd, (subx, suby) = 10, (1, 1)
    m = GrainMeter(bd, batch_frames=8, scales=True)
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
    assert_records(m.finish_scales(), [S.scale_frame(n, c, bd, subx, suby) for n, c in pairs], "mixed")
    assert_ordinary(m.finish(), pairs, bd, subx, suby, "mixed")
    m.close()


def test_batch_frames_1_2_n_and_n_plus_1_and_a_capacity_one_short():
    from grav1synth_amd.measure import SRECORD, GrainMeter

    bd, n = 10, 4
    pairs = [planes_of(150, 90, bd, "420", seed=30 + k, amp=90) for k in range(n)]
    wants = [S.scale_frame(a, b, bd, 1, 1) for a, b in pairs]
    for batch in (1, 2, n, n + 1):
        m = GrainMeter(bd, batch_frames=batch, scales=True)
        for noisy, clean in pairs:
            m.measure(noisy, clean, 1, 1)
        # a buffer one record short: G1S_ERR_CAPACITY, the count, and nothing lost; not sticky
        cnt = C.c_size_t()
        small = np.zeros(n - 1, SRECORD)
        assert m._L.g1s_measure_finish_scales(m._h, small.ctypes.data, n - 1, C.byref(cnt)) == _lib.G1S_ERR_CAPACITY and cnt.value == n
        with pytest.raises(_lib.G1SError):
            m.finish_scales(cap=n - 1)
        assert_ordinary(m.finish(), pairs, bd, 1, 1, f"batch_frames {batch}")
        assert_records(m.finish_scales(), wants, f"batch_frames {batch}")
        assert len(m.finish_scales()) == 0 and len(m.finish()) == 0
        m.close()


def test_a_geometry_change_in_mid_queue_and_a_one_plane_pair_between_three_plane_pairs():
    from grav1synth_amd.measure import GrainMeter

    bd = 8
    m = GrainMeter(bd, batch_frames=8, scales=True)
    a = [planes_of(70, 50, bd, "420", seed=60 + k, amp=25) for k in range(3)]
    b = [planes_of(33, 141, bd, "444", seed=70 + k) for k in range(2)]
    mono = planes_of(33, 141, bd, "mono", seed=80)
    order = [(a[0], 1, 1), (a[1], 1, 1), (b[0], 0, 0), (mono, 0, 0), (b[1], 0, 0), (a[2], 1, 1)]
    for k, ((noisy, clean), subx, suby) in enumerate(order):
        m.measure(_to_dev(noisy, bd) if k & 1 else noisy, clean, subx, suby)
    got = m.finish_scales()
    assert_records(got, [S.scale_frame(p[0], p[1], bd, sx, sy) for p, sx, sy in order], "geometry changes")
    assert got[3]["n"][0].any() and not got[3]["n"][1:].any(), "a one-plane pair: zeros for the planes it does not have"
    ordinary = m.finish()
    for k, ((noisy, clean), subx, suby) in enumerate(order):
        assert not R.mismatches(ordinary[k], R.measure_frame(noisy, clean, bd, subx, suby), f"pair {k}")
    m.close()


@pytest.mark.parametrize("modes", range(4))
def test_new_scales_with_every_mode_leaves_the_other_records_as_they_were_and_the_four_finish_calls_interleave(modes):
    from grav1synth_amd.measure import GrainMeter

    bd = 10
    temporal, cross = bool(modes & 1), bool(modes & 2)
    pairs = [planes_of(131, 77, bd, "420", seed=90 + k, amp=70) for k in range(7)]
    swant = [S.scale_frame(a, b, bd, 1, 1) for a, b in pairs]
    ref = GrainMeter(bd, batch_frames=3, temporal=temporal, cross=cross)
    m = GrainMeter(bd, batch_frames=3, temporal=temporal, cross=cross, scales=True)
    for noisy, clean in pairs:
        ref.measure(noisy, clean, 1, 1)
        m.measure(_to_dev(noisy, bd), clean, 1, 1)
    assert_records(m.finish_scales(), swant, f"modes {modes}")
    assert m.finish().tobytes() == ref.finish().tobytes()
    if temporal:
        assert m.finish_temporal().tobytes() == ref.finish_temporal().tobytes()
        m.cut(), ref.cut()
    if cross:
        assert m.finish_cross().tobytes() == ref.finish_cross().tobytes()
    # interleaved: each call keeps the others' records
    for meter in (m, ref):
        meter.measure(*pairs[0], 1, 1), meter.measure(*pairs[1], 1, 1)
    assert_records(m.finish_scales(), swant[:2], "scales first")
    for meter in (m, ref):
        meter.measure(*pairs[2], 1, 1)
    if temporal:
        assert m.finish_temporal().tobytes() == ref.finish_temporal().tobytes()
    for meter in (m, ref):
        meter.measure(*pairs[3], 1, 1)
    if cross:
        assert m.finish_cross().tobytes() == ref.finish_cross().tobytes()
    for meter in (m, ref):
        meter.measure(*pairs[4], 1, 1)
    got = m.finish()
    assert got.tobytes() == ref.finish().tobytes() and len(got) == 5
    assert_ordinary(got, pairs[:5], bd, 1, 1, "ordinary last")
    assert_records(m.finish_scales(), swant[2:5], "scales after the others")
    if temporal:
        assert m.finish_temporal().tobytes() == ref.finish_temporal().tobytes()
    if cross:
        assert m.finish_cross().tobytes() == ref.finish_cross().tobytes()
    m.close(), ref.close()


def test_meters_without_scales_refuse_finish_scales_and_go_on_working():
    from grav1synth_amd.measure import GrainMeter

    bd = 8
    for kw in ({}, {"temporal": True}, {"cross": True}):
        m = GrainMeter(bd, **kw)
        noisy, clean = planes_of(70, 50, bd, "420", seed=1)
        m.measure(noisy, clean, 1, 1)
        with pytest.raises(_lib.G1SError) as e:
            m.finish_scales()
        assert e.value.code == -1 and "g1s_measure_new_scales" in str(e.value)
        n = C.c_size_t(7)
        assert m._L.g1s_measure_finish_scales(m._h, None, 0, C.byref(n)) == -1
        m.measure(clean, noisy, 1, 1)
        assert_ordinary(m.finish(), [(noisy, clean), (clean, noisy)], bd, 1, 1, "after the refusals")
        assert m.scales_kernel_times() == (0.0, 0)
        m.close()


@pytest.mark.parametrize("w,h", [(65536, 64), (64, 65536)])
def test_limits_65536_samples_a_side(meters, w, h):
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
    want = check_pairs(meters(bd), [(noisy, clean)], bd, 1, 1, f"{w}x{h}")[0]
    assert int(want["n"][0, 4].sum()) == 2 * 2048 and int(want["n"][1, 4].sum()) == 1024


def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "grav1synth_amd", *args], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT,
                          stdin=subprocess.DEVNULL)


def test_measure_and_check_scales_on_files(tmp_path):
    """`measure --scales`, then `check --scales` closed over `diff`'s own table: the reports byte for byte what the restatements
    make, the rendering from tests/grain_ref.py."""
    from grav1synth_amd.ingest import write_y4m
    from grav1synth_amd.measure import check_y4m_files, measure_y4m_files
    from grav1synth_amd.tbl import GrainTable, parse_tbl

    bd, w, h, n = 10, 208, 136, 3
    made = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(n)]
    src, den = [p[0] for p in made], [p[1] for p in made]
    a, b, tbl, out, sout, xout = (tmp_path / name for name in ("src.y4m", "den.y4m", "t.tbl", "fit.txt", "sfit.txt", "xfit.txt"))
    fps = Fraction(24, 1)
    write_y4m(str(a), src, bd, 1, 1, fps)
    write_y4m(str(b), den, bd, 1, 1, fps)
    pairs = list(zip(src, den))
    rec_s = R.sum_records([R.measure_frame(s, d, bd, 1, 1) for s, d in pairs])
    srec_s = S.sum_records([S.scale_frame(s, d, bd, 1, 1) for s, d in pairs])
    profile = R.format_profile(rec_s, n, bd, w, h, 1, 1, 3)
    p = _run("measure", str(a), str(b), "-o", str(out), "--scales", str(sout))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Measured {n} frames" in p.stderr and f"wrote scale profile to {sout}" in p.stderr
    assert out.read_bytes() == profile and sout.read_bytes() == S.format_scales(rec_s, srec_s, n, bd, 3), sout.read_text()
    # with the cross report beside it and small batches; without --scales: the bytes of the existing entry points
    assert measure_y4m_files(str(a), str(b), str(out), cross_output=str(xout), scales_output=str(sout), batch_frames=2) == (n, False)
    assert out.read_bytes() == profile and sout.read_bytes() == S.format_scales(rec_s, srec_s, n, bd, 3)
    xwant = xout.read_bytes()
    o2, x2 = tmp_path / "p2.txt", tmp_path / "x2.txt"
    assert measure_y4m_files(str(a), str(b), str(o2), cross_output=str(x2)) == (n, False)
    assert o2.read_bytes() == profile and x2.read_bytes() == xwant

    p = _run("diff", str(a), str(b), "-o", str(tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    p = _run("check", str(a), str(b), "-g", str(tbl), "-o", str(out), "--scales", str(sout), "-y")
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Checked {n} frames" in p.stderr and f"wrote scale profile to {sout}" in p.stderr
    table = GrainTable(parse_tbl(tbl.read_bytes()))
    rendered = []
    for k in range(n):
        seg = table.segment_for(k * 10000000 * fps.denominator // fps.numerator)
        assert seg is not None
        rendered.append(G.add_noise(den[k], seg, bd, 1, 1))
    rec_r = R.sum_records([R.measure_frame(rendered[k], den[k], bd, 1, 1) for k in range(n)])
    srec_r = S.sum_records([S.scale_frame(rendered[k], den[k], bd, 1, 1) for k in range(n)])
    fit = R.format_profile(rec_s, n, bd, w, h, 1, 1, 3, synth=rec_r)
    swant = S.format_scales(rec_s, srec_s, n, bd, 3, synth=rec_r, ssynth=srec_r)
    assert out.read_bytes() == fit
    assert sout.read_bytes() == swant, sout.read_text()
    assert swant.count(b"\ngain_ratio ") == 15 and b"\ngain_ratio 1 -" not in swant.split(b"plane 1")[0], "the luma column is there"
    # small groups, and without --scales the bytes of the existing entry points
    o2, s2 = tmp_path / "fit2.txt", tmp_path / "sfit2.txt"
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2), batch_frames=2, scales_output=str(s2)) == (n, False)
    assert o2.read_bytes() == fit and s2.read_bytes() == swant
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2)) == (n, False) and o2.read_bytes() == fit
    # all four kinds in one run of either command, small batches: every report the bytes a run with that output alone writes
    kinds = ("temporal_output", "cross_output", "scales_output")
    for name, run in (("measure", lambda o, **kw: measure_y4m_files(str(a), str(b), str(o), **kw)),
                      ("check", lambda o, **kw: check_y4m_files(str(a), str(b), str(tbl), str(o), **kw))):
        plain = tmp_path / f"{name}_all.txt"
        together = {k: tmp_path / f"{name}_all_{k}.txt" for k in kinds}
        assert run(plain, batch_frames=2, **{k: str(v) for k, v in together.items()}) == (n, False)
        assert plain.read_bytes() == (profile if name == "measure" else fit)
        for k in kinds:
            alone, alone_plain = tmp_path / f"{name}_alone_{k}.txt", tmp_path / f"{name}_alone_{k}_plain.txt"
            assert run(alone_plain, **{k: str(alone)}) == (n, False)
            assert alone_plain.read_bytes() == plain.read_bytes(), (name, k)
            assert together[k].read_bytes() == alone.read_bytes() and len(alone.read_bytes()) > 100, (name, k)
