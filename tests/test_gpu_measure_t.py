"""The temporal meter on the device against tests/measure_t_ref.py: every field of every temporal record with array_equal,
every report byte for byte.  There is no tolerance anywhere."""
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
from tests import measure_t_ref as T
from tests import views as V
from tests.test_gpu_grain import _to_dev
from tests.test_measure_cpu import SUBSAMPLINGS, planes_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW, TH = 64, 128  # km_measure_t's tile


@pytest.fixture(scope="module")
def meters():
    from grav1synth_amd.measure import GrainMeter

    made = {}

    def get(bd, **kw):
        key = (bd, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = GrainMeter(bd, temporal=True, **kw)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def assert_records(got, wants, what):
    assert len(got) == len(wants), f"{what}: {len(got)} temporal records, want {len(wants)}"
    for k, want in enumerate(wants):
        for name, _dt, _size in T.FIELDS:
            assert np.array_equal(np.asarray(got[k][name]), want[name]), "\n".join(T.mismatches(got[k], want, f"{what}, record {k}"))


def assert_ordinary(got, pairs, bd, subx, suby, what):
    assert len(got) == len(pairs), what
    for k, (noisy, clean) in enumerate(pairs):
        bad = R.mismatches(got[k], R.measure_frame(noisy, clean, bd, subx, suby), f"{what}, pair {k}")
        assert not bad, "\n".join(bad)


def check_run(m, pairs, bd, subx, suby, what, dev=True):
    """One run (the meter is cut behind it): its temporal records against the restatement.  Returns the reference records."""
    for noisy, clean in pairs:
        m.measure(_to_dev(noisy, bd) if dev else noisy, _to_dev(clean, bd) if dev else clean, subx, suby)
    got = m.finish_temporal()
    wants = T.run_records(pairs, bd, subx, suby)
    assert_records(got, wants, what)
    m.cut()
    assert len(m.finish()) == len(pairs)
    return wants


def with_residual(clean, d, bd):
    """The noisy planes clean + d; the clean planes are moved away from the range's ends first, so that nothing clips."""
    top = (1 << bd) - 1
    out_n, out_c = [], []
    for p, r in zip(clean, d):
        amp = int(np.abs(r).max()) if r.size else 0
        c = np.clip(p.astype(np.int64), amp, top - amp)
        out_c.append(c.astype(p.dtype))
        out_n.append((c + r).astype(p.dtype))
    return out_n, out_c


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
def test_formats_on_plane_distinct_content_with_independent_noise_a_frame(meters, bd, ss):
    mono = ss == "mono"
    subx, suby = (1, 1) if mono else SUBSAMPLINGS[ss]
    pairs = [CT.make_frames("distinct", 208, 136, bd, subx, suby, frame=k) for k in range(3)]
    if mono:
        pairs = [(s[:1], d[:1]) for s, d in pairs]
    wants = check_run(meters(bd), pairs, bd, subx, suby, f"{bd} bit {ss}")
    assert wants[0]["u"][0].any() and wants[0]["x"][0].any()
    assert mono or not np.array_equal(wants[0]["c"][1], wants[0]["c"][2]), "the planes differ"
    assert not np.array_equal(wants[0]["c"][0], wants[1]["c"][0]), "the frames differ"


SIZES = [(1, 1), (2, 3), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW + 2, 2 * TH + 1)]


@pytest.mark.parametrize("size", SIZES)
def test_sizes_round_the_tile_and_below_the_halo_in_runs_of_1_2_and_5(meters, size):
    w, h = size
    for (bd, ss), n in zip(((8, "420"), (10, "422"), (12, "444"), (10, "mono")), (5, 2, 1, 2)):
        subx, suby = SUBSAMPLINGS[ss]
        pairs = [planes_of(w, h, bd, ss, seed=2 + k) for k in range(n)]
        wants = check_run(meters(bd), pairs, bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
        assert len(wants) == n - 1


def test_the_same_residual_in_every_frame(meters):
    bd, w, h, (subx, suby) = 10, 150, 140, (1, 1)
    rng = np.random.default_rng(5)
    d = [rng.integers(-300, 301, s) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    pairs = [with_residual(planes_of(w, h, bd, "420", seed=40 + k)[1], d, bd) for k in range(3)]
    wants = check_run(meters(bd), pairs, bd, subx, suby, "one residual")
    for rec in wants:
        assert np.array_equal(rec["x"].astype(np.uint64), rec["u"]) and np.array_equal(rec["u"], rec["v"]) and rec["u"].any()


def test_a_moved_residual_for_each_of_the_25_offsets(meters):
    """d_{t-1}(p + delta_i) = d_t(p) wherever both lie inside the plane, zero elsewhere: c[i] is the sum of d_t^2 over the
    overlap.  150 x 140 is 3 x 2 tiles, so the offsets cross tile borders in both directions."""
    bd, w, h = 8, 150, 140
    rng = np.random.default_rng(6)
    clean = [np.full((h, w), 100, np.uint8)]
    d = rng.integers(-50, 51, (h, w))
    m = meters(bd)
    for i, (dx, dy) in enumerate(T.OFFSETS):
        e = np.zeros_like(d)
        y0, y1, x0, x1 = max(0, -dy), h - max(0, dy), max(0, -dx), w - max(0, dx)
        e[y0 + dy:y1 + dy, x0 + dx:x1 + dx] = d[y0:y1, x0:x1]
        pairs = [([(clean[0] + e).astype(np.uint8)], clean), ([(clean[0] + d).astype(np.uint8)], clean)]
        wants = check_run(m, pairs, bd, 0, 0, f"offset {dx} {dy}")
        assert int(wants[0]["c"][0, i]) == int((d[y0:y1, x0:x1] ** 2).sum())
        assert int(np.argmax(wants[0]["c"][0])) == i


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_adversarial_bins(meters, bd):
    w, h, step = 200, 150, 1 << (bd - 5)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    cases = {
        "one intensity": [np.full((h, w), 11 * step + 3)] * 2,
        "two alternating bins": [np.where((xs + ys + t) & 1, 7 * step, 8 * step - 1) + 0 * ys for t in (0, 1)],
        "a ramp through all 32 that differs between t and t - 1": [((xs + 5 * t) % 32) * step + ((ys + t) % step) for t in (0, 1)],
        "a ramp down the columns, another across": [((ys % 32) * step + 0 * xs), ((xs % 32) * step + 0 * ys)],
    }
    for what, lumas in cases.items():
        pairs = []
        for t, luma in enumerate(lumas):
            noisy, clean = planes_of(w, h, bd, "420", seed=bd + 3 * t, amp=60)
            d = noisy[0].astype(np.int64) - clean[0].astype(np.int64)
            clean[0] = luma.astype(clean[0].dtype)
            noisy[0] = np.clip(luma + d, 0, (1 << bd) - 1).astype(clean[0].dtype)
            pairs.append((noisy, clean))
        wants = check_run(meters(bd), pairs, bd, 1, 1, f"{bd} bit, {what}")
        if what == "one intensity":
            assert np.count_nonzero(wants[0]["n"][0]) == 1 and np.count_nonzero(wants[0]["n"][1]) == 1
        if what.startswith("a ramp"):
            assert np.count_nonzero(wants[0]["n"][0]) == 32


def test_extremes_at_12_bits(meters):
    """d = +-4095 everywhere in both pairs.  A lane's 32-bit sums take 32 products of 2^24 (2^29) before they go on in 64
    bits; a 64 x 128 tile's sum is 2^37.  192 x 300 is 3 x 3 tiles of luma with partial tiles.  The signs of (d_t, d_{t-1})
    in turn: (-, +), (-, -), (+, -), (+, +)."""
    bd, w, h = 12, 192, 300
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    top = [np.full(s, 4095, np.uint16) for s in shapes]
    zero = [np.zeros(s, np.uint16) for s in shapes]
    plus, minus = (top, zero), (zero, top)
    wants = check_run(meters(bd), [plus, minus, minus, plus, plus], bd, 1, 1, "+-4095")
    for rec, sign in zip(wants, (-1, 1, -1, 1)):
        assert int(rec["c"][0, 12]) == sign * 4095 * 4095 * w * h and abs(int(rec["c"][0, 12])) > 2 ** 32
        assert int(rec["x"][0].sum()) == int(rec["c"][0, 12]) and int(rec["u"][0].sum()) == int(rec["v"][0].sum()) == 4095 * 4095 * w * h
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    sign = ((xs + 2 * ys) % 3 == 0)  # both extremes side by side, against its own mirror image: negative and positive products
    a = [np.where(sign[:s[0], :s[1]], 4095, 0).astype(np.uint16) for s in shapes]
    b = [np.where(sign[:s[0], :s[1]], 0, 4095).astype(np.uint16) for s in shapes]
    check_run(meters(bd), [(a, b), (b, a), (a, b)], bd, 1, 1, "+-4095 mixed")


def test_host_frames_whose_predecessor_lives_in_the_batch_before():
    from grav1synth_amd.measure import GrainMeter

    bd, n = 10, 4
    pairs = [planes_of(150, 90, bd, "420", seed=30 + k, amp=90) for k in range(n)]
    wants = T.run_records(pairs, bd, 1, 1)
    plain = GrainMeter(bd, batch_frames=2)
    for noisy, clean in pairs:
        plain.measure(noisy, clean, 1, 1)
    ordinary = plain.finish()
    assert_ordinary(ordinary, pairs, bd, 1, 1, "plain meter")
    plain.close()
    for batch in (1, 2, n, n + 1):
        m = GrainMeter(bd, batch_frames=batch, temporal=True)
        for rounds in range(2):  # (the second run goes on round the ring where the first stopped)
            for noisy, clean in pairs:
                m.measure(noisy, clean, 1, 1)
            assert_records(m.finish_temporal(), wants, f"batch_frames {batch}, run {rounds}")
            got = m.finish()
            assert got.tobytes() == ordinary.tobytes(), "the ordinary records of a temporal meter are a plain meter's"
            m.cut()
        m.close()


def test_host_pinned_and_device_frames_in_one_run():
    import torch

    from grav1synth_amd.measure import GrainMeter

    bd, (subx, suby) = 10, (1, 1)
    m = GrainMeter(bd, batch_frames=4, temporal=True)
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
    assert_records(m.finish_temporal(), T.run_records(pairs, bd, subx, suby), "mixed")
    assert_ordinary(m.finish(), pairs, bd, subx, suby, "mixed")
    m.close()


@pytest.mark.parametrize("bd,ss", [(8, "420"), (10, "422"), (12, "444")])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    isz = 1 if bd == 8 else 2
    pairs = [planes_of(147, 139, bd, ss, seed=4 + k, amp=200) for k in range(3)]
    guards, keep = [], []
    m = meters(bd)
    for k, ((extra, base), pair) in enumerate(zip(((6, 2), (34, 14), (130, 250)), pairs)):
        devs = []
        for j, planes in enumerate(pair):
            dev = []
            for c, p in enumerate(planes):
                view, guard = V.device_view(p, pitch_bytes=p.shape[1] * isz + extra * isz, base_offset_bytes=(base + 2 * c * (j + 1)) % 256 & ~(isz - 1),
                                            fill="random" if k & 1 else "max", max_code=(1 << bd) - 1, seed=10 * k + c)
                dev.append(view)
                guards.append(guard)
            devs.append(dev)
        keep.append(devs)
        m.measure(devs[0], devs[1], subx, suby)
    assert_records(m.finish_temporal(), T.run_records(pairs, bd, subx, suby), f"views {bd} bit {ss}")
    assert_ordinary(m.finish(), pairs, bd, subx, suby, "views")
    m.cut()
    for g in guards:
        g.assert_unchanged("a view")


def test_a_geometry_change_in_mid_queue_ends_the_run():
    from grav1synth_amd.measure import GrainMeter

    bd = 8
    m = GrainMeter(bd, batch_frames=8, temporal=True)
    a = [planes_of(70, 50, bd, "420", seed=60 + k, amp=25) for k in range(3)]
    b = [planes_of(33, 141, bd, "444", seed=70 + k) for k in range(3)]
    mono = [planes_of(33, 141, bd, "mono", seed=80 + k) for k in range(2)]
    for k, (noisy, clean) in enumerate(a[:2]):
        m.measure(_to_dev(noisy, bd) if k else noisy, clean, 1, 1)
    for noisy, clean in b:
        m.measure(noisy, _to_dev(clean, bd), 0, 0)
    for noisy, clean in mono:  # (the same luma size: the plane count alone is a change of geometry)
        m.measure(noisy, clean, 0, 0)
    m.measure(a[2][0], a[2][1], 1, 1)  # back to the first geometry: no record against a[1]
    wants = T.run_records(a[:2], bd, 1, 1) + T.run_records(b, bd, 0, 0) + T.run_records(mono, bd, 0, 0)
    got = m.finish_temporal()
    assert_records(got, wants, "geometry changes")
    assert not got[3]["n"][1:].any() and not got[3]["c"][1:].any(), "a luma-only frame has zeros for the chroma planes"
    assert len(m.finish()) == 8
    m.close()


def test_cut_finish_and_finish_temporal_in_either_order_between_pairs():
    """The run's last pair survives a hand-over: after finish() or finish_temporal() its device planes may change, and the
    next pair's temporal record is still against what they held."""
    import torch

    from grav1synth_amd.measure import TRECORD, GrainMeter

    bd = 10
    pairs = [planes_of(131, 77, bd, "420", seed=90 + k, amp=70) for k in range(7)]
    want = T.run_records(pairs, bd, 1, 1)
    m = GrainMeter(bd, batch_frames=3, temporal=True)

    def give(k, dev):
        planes = [_to_dev(p, bd) for p in pairs[k]] if dev else pairs[k]
        m.measure(planes[0], planes[1], 1, 1)
        return planes

    give(0, True)
    last = give(1, True)
    assert_ordinary(m.finish(), pairs[:2], bd, 1, 1, "finish first")
    for planes in last:  # (finish handed the planes back)
        for p in planes:
            p.view(torch.int16).fill_(3)
    torch.cuda.synchronize()
    last = give(2, True)
    assert_records(m.finish_temporal(), want[:2], "finish_temporal after finish")
    for planes in last:
        for p in planes:
            p.view(torch.int16).zero_()
    torch.cuda.synchronize()
    give(3, False)
    give(4, False)
    assert_records(m.finish_temporal(), want[2:4], "finish_temporal twice")
    assert len(m.finish_temporal()) == 0
    give(5, True)
    # a buffer too small: G1S_ERR_CAPACITY, the count, and nothing lost; not sticky
    n = C.c_size_t()
    small = np.zeros(1, TRECORD)
    give(6, False)
    assert m._L.g1s_measure_finish_temporal(m._h, small.ctypes.data, 1, C.byref(n)) == _lib.G1S_ERR_CAPACITY and n.value == 2
    with pytest.raises(_lib.G1SError):
        m.finish_temporal(cap=1)
    assert_ordinary(m.finish(), pairs[2:], bd, 1, 1, "finish between")
    assert_records(m.finish_temporal(), want[4:], "after the capacity refusals")
    # cut: the next pair has no record; the run after it has its own
    m.cut()
    give(0, False)
    give(1, True)
    m.cut()
    give(2, True)
    give(3, False)
    assert_records(m.finish_temporal(), [want[0], want[2]], "cut")
    assert len(m.finish()) == 4
    m.close()


def test_a_plain_meter_refuses_cut_and_finish_temporal_and_goes_on_working():
    from grav1synth_amd.measure import GrainMeter

    bd = 8
    m = GrainMeter(bd)
    noisy, clean = planes_of(70, 50, bd, "420", seed=1)
    m.measure(noisy, clean, 1, 1)
    for call in (m.cut, m.finish_temporal):
        with pytest.raises(_lib.G1SError) as e:
            call()
        assert e.value.code == -1 and "g1s_measure_new_temporal" in str(e.value)
    n = C.c_size_t(7)
    assert m._L.g1s_measure_finish_temporal(m._h, None, 0, C.byref(n)) == -1
    m.measure(clean, noisy, 1, 1)
    assert_ordinary(m.finish(), [(noisy, clean), (clean, noisy)], bd, 1, 1, "after the refusals")
    m.close()


def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "grav1synth_amd", *args], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT,
                          stdin=subprocess.DEVNULL)


def _distinct_clip(n, w=200, h=136, bd=10):
    pairs = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(n)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def test_measure_temporal_on_files(tmp_path):
    from grav1synth_amd.ingest import UNEQUAL_WARNING, write_y4m
    from grav1synth_amd.measure import measure_y4m_files

    bd, w, h = 10, 200, 136
    src, den = _distinct_clip(5, w, h, bd)
    a, b, out, tout = tmp_path / "a.y4m", tmp_path / "b.y4m", tmp_path / "profile.txt", tmp_path / "temporal.txt"
    write_y4m(str(a), src, bd, 1, 1, Fraction(24, 1))
    write_y4m(str(b), den[:4], bd, 1, 1, Fraction(24, 1))  # unequal lengths: the shorter file ends the clip
    p = _run("measure", str(a), str(b), "-o", str(out), "--temporal", str(tout))
    assert p.returncode == 0, p.stderr[-2000:]
    assert UNEQUAL_WARNING in p.stderr and "Measured 4 frames" in p.stderr and f"wrote temporal profile to {tout}" in p.stderr
    pairs = list(zip(src[:4], den[:4]))
    profile = R.format_profile(R.sum_records([R.measure_frame(s, d, bd, 1, 1) for s, d in pairs]), 4, bd, w, h, 1, 1, 3)
    want = T.format_temporal(T.sum_records(T.run_records(pairs, bd, 1, 1)), 3, bd, w, h, 1, 1, 3)
    assert out.read_bytes() == profile and tout.read_bytes() == want
    assert b"\npairs 3 " in want and want.count(b"\ntemporal_rho ") == 3
    # an existing temporal output without -y and without a terminal is an error exit; -y covers both outputs
    p = _run("measure", str(a), str(b), "-o", str(tmp_path / "other.txt"), "--temporal", str(tout))
    assert p.returncode == 1 and "not a terminal" in p.stderr and tout.read_bytes() == want
    # batches of 2 and of 1: the predecessor lives in the batch before; the same bytes; without the temporal output, the
    # existing command
    for batch in (1, 2):
        o2, t2 = tmp_path / f"p{batch}.txt", tmp_path / f"t{batch}.txt"
        assert measure_y4m_files(str(a), str(b), str(o2), batch_frames=batch, temporal_output=str(t2)) == (4, True)
        assert o2.read_bytes() == profile and t2.read_bytes() == want
    o3 = tmp_path / "p3.txt"
    assert measure_y4m_files(str(a), str(b), str(o3)) == (4, True) and o3.read_bytes() == profile
    # a clip of one frame: pairs 0
    write_y4m(str(b), den[:1], bd, 1, 1, Fraction(24, 1))
    assert measure_y4m_files(str(a), str(b), str(out), temporal_output=str(tout)) == (1, True)
    assert tout.read_bytes() == b"graintemporal1\npairs 0 bit_depth 10 planes 3\nplane 0\nplane 1\nplane 2\n"
    assert out.read_bytes() == R.format_profile(R.measure_frame(src[0], den[0], bd, 1, 1), 1, bd, w, h, 1, 1, 3)


def test_check_temporal_on_files(tmp_path):
    """`diff` a short plane-distinct clip, then `check --temporal` on that table: both reports equal, byte for byte, what
    the restatements make from tests/grain_ref.py's rendering of the same frames with the table's lookup and seeds."""
    from grav1synth_amd.ingest import write_y4m
    from grav1synth_amd.measure import check_y4m_files
    from grav1synth_amd.tbl import GrainTable, parse_tbl

    bd, w, h, n = 10, 320, 192, 5
    src, den = _distinct_clip(n, w, h, bd)
    a, b, tbl, out, tout = (tmp_path / name for name in ("src.y4m", "den.y4m", "t.tbl", "fit.txt", "tfit.txt"))
    fps = Fraction(24, 1)
    write_y4m(str(a), src, bd, 1, 1, fps)
    write_y4m(str(b), den, bd, 1, 1, fps)
    p = _run("diff", str(a), str(b), "-o", str(tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    p = _run("check", str(a), str(b), "-g", str(tbl), "-o", str(out), "--temporal", str(tout))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Checked {n} frames" in p.stderr and f"wrote temporal profile to {tout}" in p.stderr
    table = GrainTable(parse_tbl(tbl.read_bytes()))
    rendered = []
    for k in range(n):
        seg = table.segment_for(k * 10000000 * fps.denominator // fps.numerator)
        assert seg is not None
        rendered.append(G.add_noise(den[k], seg, bd, 1, 1))
    rec_s = [R.measure_frame(src[k], den[k], bd, 1, 1) for k in range(n)]
    rec_r = [R.measure_frame(rendered[k], den[k], bd, 1, 1) for k in range(n)]
    profile = R.format_profile(R.sum_records(rec_s), n, bd, w, h, 1, 1, 3, synth=R.sum_records(rec_r))
    trec_s = T.sum_records(T.run_records(list(zip(src, den)), bd, 1, 1))
    trec_r = T.sum_records(T.run_records(list(zip(rendered, den)), bd, 1, 1))
    want = T.format_temporal(trec_s, n - 1, bd, w, h, 1, 1, 3, synth=trec_r)
    assert out.read_bytes() == profile and tout.read_bytes() == want
    assert trec_r["u"].any(), "the table put grain on the clip"
    # small groups: the previous rendered and denoised frame come from the group before; the same bytes
    o2, t2 = tmp_path / "fit2.txt", tmp_path / "tfit2.txt"
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2), batch_frames=2, temporal_output=str(t2)) == (n, False)
    assert o2.read_bytes() == profile and t2.read_bytes() == want
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2), batch_frames=3, temporal_output=str(t2)) == (n, False)
    assert o2.read_bytes() == profile and t2.read_bytes() == want
    # a source that is the denoised clip plus one fixed residual: temporal_rho 1.0000 in the first column, on every plane;
    # unequal lengths and a clip of one frame
    rng = np.random.default_rng(11)
    d = [rng.integers(-9, 10, p.shape) for p in den[0]]
    fixed = [with_residual(den[k], d, bd) for k in range(n)]
    write_y4m(str(a), [f[0] for f in fixed], bd, 1, 1, fps)
    write_y4m(str(b), [f[1] for f in fixed[:3]], bd, 1, 1, fps)  # (unequal lengths)
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2), temporal_output=str(t2)) == (3, True)
    lines = t2.read_text().splitlines()
    assert lines[1] == "pairs 2 bit_depth 10 planes 3"
    rho = [line.split() for line in lines if line.startswith("temporal_rho ")]
    assert len(rho) == 3 and all(r[1] == "1.0000" for r in rho), rho
    write_y4m(str(b), [fixed[0][1]], bd, 1, 1, fps)
    assert check_y4m_files(str(a), str(b), str(tbl), str(o2), temporal_output=str(t2)) == (1, True)
    assert t2.read_bytes() == b"graintemporal1\npairs 0 bit_depth 10 planes 3\nplane 0\nplane 1\nplane 2\n"
