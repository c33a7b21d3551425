"""`measure` and `check` on the device against tests/measure_ref.py: every record field by field, every report byte for
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
from tests import measure_ref as R
from tests import views as V
from tests.test_gpu_grain import _to_dev, make_segment
from tests.test_measure_cpu import SUBSAMPLINGS, planes_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW, TH = 64, 128  # km_measure's tile


@pytest.fixture(scope="module")
def meters():
    from grav1synth_amd.measure import GrainMeter

    made = {}

    def get(bd, **kw):
        key = (bd, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = GrainMeter(bd, **kw)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def check_pair(meter, noisy, clean, bd, subx, suby, what, dev=True):
    meter.measure(_to_dev(noisy, bd) if dev else noisy, _to_dev(clean, bd) if dev else clean, subx, suby)
    got = meter.finish()
    assert len(got) == 1
    bad = R.mismatches(got[0], R.measure_frame(noisy, clean, bd, subx, suby), what)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
def test_formats_on_plane_distinct_content_with_rendered_grain(meters, bd, ss):
    mono = ss == "mono"
    subx, suby = (1, 1) if mono else SUBSAMPLINGS[ss]
    _src, den = CT.make_frames("distinct", 208, 136, bd, subx, suby, frame=1)
    grainy = G.add_noise(den, make_segment(3, 50 + bd), bd, subx, suby)
    if mono:
        grainy, den = grainy[:1], den[:1]
    want = R.measure_frame(grainy, den, bd, subx, suby)
    assert want["s2"][0].any() and (mono or not np.array_equal(want["r"][1], want["r"][2])), "the planes differ"
    check_pair(meters(bd), grainy, den, bd, subx, suby, f"{bd} bit {ss}")


SIZES = [(1, 1), (3, 7), (2, 3), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW + 3, 31), (33, 2 * TH + 2), (2, 210), (300, 2), (129, 5)]


@pytest.mark.parametrize("size", SIZES)
def test_sizes_round_the_tile_and_below_the_halo(meters, size):
    w, h = size
    for bd, ss in ((8, "420"), (10, "422"), (12, "444"), (10, "mono")):
        subx, suby = SUBSAMPLINGS[ss]
        noisy, clean = planes_of(w, h, bd, ss, seed=2)
        check_pair(meters(bd), noisy, clean, bd, subx, suby, f"{w}x{h} {bd} bit {ss}")


def _with_clean_luma(w, h, bd, luma, seed):
    """A 4:2:0 pair whose clean luma is `luma`; residuals of up to +- 60."""
    noisy, clean = planes_of(w, h, bd, "420", seed, amp=60)
    d = noisy[0].astype(np.int64) - clean[0].astype(np.int64)
    clean[0] = luma.astype(clean[0].dtype)
    noisy[0] = np.clip(luma + d, 0, (1 << bd) - 1).astype(clean[0].dtype)
    return noisy, clean


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_adversarial_bins(meters, bd):
    w, h, step = 200, 150, 1 << (bd - 5)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    cases = {
        "one intensity": np.full((h, w), 11 * step + 3),
        "two bins, sample by sample": np.where((xs + ys) & 1, 7 * step, 8 * step - 1) + 0 * ys,
        "two bins, column by column": np.where(xs & 1, 30 * step, 2 * step) + 0 * ys,
        "a ramp through every bin within a wave": ((xs % 32) * step + (ys % step)),
        "a ramp down the columns": ((ys % 32) * step + 0 * xs),
    }
    for what, luma in cases.items():
        noisy, clean = _with_clean_luma(w, h, bd, luma, seed=bd)
        want = R.measure_frame(noisy, clean, bd, 1, 1)
        if what == "one intensity":
            assert np.count_nonzero(want["n"][0]) == 1 and np.count_nonzero(want["n"][1]) == 1
        if what.startswith("a ramp"):
            assert np.count_nonzero(want["n"][0]) == 32
        check_pair(meters(bd), noisy, clean, bd, 1, 1, f"{bd} bit, {what}")


def test_extremes_at_12_bits(meters):
    """d = +4095 and d = -4095 everywhere.  The kernel hands a lane's 32-bit sums on after the 32 rows a wave walks
    (32 products of 2^24: 2^29) and adds across the 64 lanes in 64 bits: a wave's sum is 2^35 and a 64 x 128 tile's 2^37,
    so one tile already overflows 32 bits many times over.  640 x 400 is 10 x 4 tiles of luma, with partial tiles."""
    bd, w, h = 12, 640, 400
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    top = [np.full(s, 4095, np.uint16) for s in shapes]
    zero = [np.zeros(s, np.uint16) for s in shapes]
    for noisy, clean, what in ((top, zero, "+4095"), (zero, top, "-4095")):
        want = R.measure_frame(noisy, clean, bd, 1, 1)
        assert int(want["r"][0, 24]) == 4095 * 4095 * w * h > 2 ** 32
        check_pair(meters(bd), noisy, clean, bd, 1, 1, what)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    sign = ((xs + 2 * ys) % 3 == 0)  # both extremes side by side: negative products
    a = [np.where(sign[:s[0], :s[1]], 4095, 0).astype(np.uint16) for s in shapes]
    b = [np.where(sign[:s[0], :s[1]], 0, 4095).astype(np.uint16) for s in shapes]
    check_pair(meters(bd), a, b, bd, 1, 1, "+-4095")


def test_4k_10_bit(meters):
    bd = 10
    _src, den = CT.make_frames("distinct", 3840, 2160, bd, 1, 1, frame=0)
    from grav1synth_amd.grain import GrainSynthesizer

    syn = GrainSynthesizer(bd)
    grainy = [p.cpu().numpy() for p in syn.apply(_to_dev(den, bd), make_segment(3, 77), 1, 1)]
    syn.close()
    check_pair(meters(bd), grainy, den, bd, 1, 1, "4K")


@pytest.mark.parametrize("bd,ss", [(8, "420"), (10, "422"), (12, "444")])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    isz = 1 if bd == 8 else 2
    noisy, clean = planes_of(147, 139, bd, ss, seed=4, amp=200)
    want = R.measure_frame(noisy, clean, bd, subx, suby)
    for k, (extra, base) in enumerate(((6, 2), (34, 14), (0, 250), (130, 6))):
        guards, devs = [], []
        for j, planes in enumerate((noisy, clean)):
            dev = []
            for c, p in enumerate(planes):
                view, guard = V.device_view(p, pitch_bytes=p.shape[1] * isz + extra * isz, base_offset_bytes=(base + 2 * c * (j + 1)) % 256 & ~(isz - 1),
                                            fill="random" if k & 1 else "max", max_code=(1 << bd) - 1, seed=10 * k + c)
                dev.append(view)
                guards.append(guard)
            devs.append(dev)
        meters(bd).measure(devs[0], devs[1], subx, suby)
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
        noisy, clean = planes_of(150, 90, bd, "420", seed=30 + k, amp=90)
        wants.append(R.measure_frame(noisy, clean, bd, subx, suby))
        kinds = [(k >> j) % 3 for j in (0, 1)] if k else [0, 1]
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
    got = m.finish()
    assert len(got) == 6
    for k in range(6):
        bad = R.mismatches(got[k], wants[k], f"pair {k}")
        assert not bad, "\n".join(bad)


def test_batches_capacity_geometry_change_and_reuse():
    from grav1synth_amd.measure import RECORD, GrainMeter

    bd = 8
    m = GrainMeter(bd, batch_frames=4)
    wants = []
    for k in range(11):  # more than two batches; the last three stay queued
        noisy, clean = planes_of(70, 50, bd, "420", seed=60 + k, amp=25)
        wants.append(R.measure_frame(noisy, clean, bd, 1, 1))
        m.measure(_to_dev(noisy, bd) if k & 1 else noisy, clean, 1, 1)
    # another geometry sends the queued pairs out first
    noisy, clean = planes_of(33, 41, bd, "444", seed=80)
    wants.append(R.measure_frame(noisy, clean, bd, 0, 0))
    m.measure(noisy, clean, 0, 0)
    noisy, clean = planes_of(33, 41, bd, "mono", seed=81)
    wants.append(R.measure_frame(noisy, clean, bd, 0, 0))
    m.measure(noisy, clean, 0, 0)
    # a buffer too small: G1S_ERR_CAPACITY, the count, and nothing lost
    n = C.c_size_t()
    small = np.zeros(5, RECORD)
    assert m._L.g1s_measure_finish(m._h, small.ctypes.data, 5, C.byref(n)) == _lib.G1S_ERR_CAPACITY and n.value == 13
    with pytest.raises(_lib.G1SError):
        m.finish(cap=12)
    got = m.finish()
    assert len(got) == 13
    for k in range(13):
        bad = R.mismatches(got[k], wants[k], f"pair {k}")
        assert not bad, "\n".join(bad)
    assert not got[12]["n"][1:].any() and not got[12]["r"][1:].any(), "a luma-only frame has zeros for the chroma planes"
    assert len(m.finish()) == 0
    # the meter used again after finish
    noisy, clean = planes_of(90, 20, bd, "422", seed=82)
    m.measure(noisy, clean, 1, 0)
    got = m.finish()
    assert len(got) == 1 and not R.mismatches(got[0], R.measure_frame(noisy, clean, bd, 1, 0), "after finish")
    m.close()


def test_refusals():
    from grav1synth_amd.diff import Frame
    from grav1synth_amd.measure import GrainMeter

    with pytest.raises(_lib.G1SError) as e:
        GrainMeter(9)
    assert "8, 10 and 12" in str(e.value)
    noisy, clean = planes_of(64, 40, 10, "420", seed=1)
    m = GrainMeter(10)
    with pytest.raises(_lib.G1SError) as e:
        m.measure(noisy, [p[:-1] for p in clean])
    assert e.value.code == -2 and "noisy and clean frame geometry differ" in str(e.value)
    with pytest.raises(_lib.G1SError):  # sticky
        m.measure(noisy, clean)
    m.close()
    m = GrainMeter(8)
    with pytest.raises(_lib.G1SError) as e:
        m.measure(noisy, clean)
    assert "bytes_per_sample" in str(e.value)
    m.close()
    m = GrainMeter(10)
    keep = []
    fa, fb = Frame(noisy, 1, 1).to_c(keep), Frame(clean, 1, 1).to_c(keep)
    fb.stride_bytes[1] = clean[1].shape[1] * 2 - 2
    assert m._L.g1s_measure_frame(m._h, C.byref(fa), C.byref(fb)) == -1
    assert "row stride" in m._L.g1s_measure_last_error(m._h).decode()
    m.close()
    m = GrainMeter(10)
    fb = Frame(clean, 1, 1).to_c(keep)
    fb.stride_bytes[0] = clean[0].shape[1] * 2 + 1  # an odd stride of 16-bit samples
    assert m._L.g1s_measure_frame(m._h, C.byref(fa), C.byref(fb)) == -1
    m.close()


def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "grav1synth_amd", *args], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT,
                          stdin=subprocess.DEVNULL)


def _distinct_clip(n, w=320, h=192, bd=10):
    pairs = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(n)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def test_measure_command_on_files_of_unequal_length(tmp_path):
    from grav1synth_amd.ingest import UNEQUAL_WARNING, write_y4m

    bd, w, h = 10, 320, 192
    src, den = _distinct_clip(5, w, h, bd)
    a, b, out = tmp_path / "a.y4m", tmp_path / "b.y4m", tmp_path / "profile.txt"
    write_y4m(str(a), src, bd, 1, 1, Fraction(24, 1))
    write_y4m(str(b), den[:3], bd, 1, 1, Fraction(24, 1))
    p = _run("measure", str(a), str(b), "-o", str(out))
    assert p.returncode == 0, p.stderr[-2000:]
    assert UNEQUAL_WARNING in p.stderr and "Measured 3 frames" in p.stderr and f"Done, wrote output file to {out}" in p.stderr
    total = R.sum_records([R.measure_frame(src[k], den[k], bd, 1, 1) for k in range(3)])
    assert out.read_bytes() == R.format_profile(total, 3, bd, w, h, 1, 1, 3)
    # equal lengths: no warning; an existing output without -y and without a terminal is an error exit, as diff's
    before = out.read_bytes()
    p = _run("measure", str(a), str(b), "-o", str(out))
    assert p.returncode == 1 and "not a terminal" in p.stderr and out.read_bytes() == before
    write_y4m(str(b), den, bd, 1, 1, Fraction(24, 1))
    p = _run("measure", str(a), str(b), "-o", str(out), "-y")
    assert p.returncode == 0 and UNEQUAL_WARNING not in p.stderr and "Measured 5 frames" in p.stderr
    p = _run("measure", str(a), str(a), "-o", str(out), "-y")
    assert p.returncode == 0 and "Source and denoised paths are the same" in p.stderr


def test_check_command_closes_the_loop(tmp_path):
    """`diff` a short plane-distinct clip, then `check SOURCE DENOISED -g` on that table: the report equals, byte for byte,
    what the reference makes from tests/grain_ref.py's rendering of the same frames with the table's lookup and seeds."""
    from grav1synth_amd.ingest import write_y4m
    from grav1synth_amd.tbl import GrainTable, parse_tbl

    bd, w, h, n = 10, 320, 192, 5
    src, den = _distinct_clip(n, w, h, bd)
    a, b, tbl, out = tmp_path / "src.y4m", tmp_path / "den.y4m", tmp_path / "t.tbl", tmp_path / "fit.txt"
    fps = Fraction(24, 1)
    write_y4m(str(a), src, bd, 1, 1, fps)
    write_y4m(str(b), den, bd, 1, 1, fps)
    p = _run("diff", str(a), str(b), "-o", str(tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    p = _run("check", str(a), str(b), "-g", str(tbl), "-o", str(out))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Checked {n} frames" in p.stderr and f"Done, wrote output file to {out}" in p.stderr
    table = GrainTable(parse_tbl(tbl.read_bytes()))
    rec_s, rec_r = [], []
    for k in range(n):
        seg = table.segment_for(k * 10000000 * fps.denominator // fps.numerator)
        assert seg is not None
        rendered = G.add_noise(den[k], seg, bd, 1, 1)
        rec_s.append(R.measure_frame(src[k], den[k], bd, 1, 1))
        rec_r.append(R.measure_frame(rendered, den[k], bd, 1, 1))
    want = R.format_profile(R.sum_records(rec_s), n, bd, w, h, 1, 1, 3, synth=R.sum_records(rec_r))
    assert out.read_bytes() == want
    assert R.sum_records(rec_r)["s2"].any(), "the table put grain on the clip"
    # small groups: several of them and a shorter last one, the same bytes
    from grav1synth_amd.measure import check_y4m_files

    out2 = tmp_path / "fit2.txt"
    assert check_y4m_files(str(a), str(b), str(tbl), str(out2), batch_frames=2) == (n, False)
    assert out2.read_bytes() == want
