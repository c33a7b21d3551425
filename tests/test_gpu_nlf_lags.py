"""Lagged noise levels on the device against tests/nlf_lags_ref.py: every field of every lag record with array_equal, beside
the ordinary and temporal records against a plain temporal meter's, byte for byte.  There is no tolerance anywhere."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import nlf_lags_ref as LG
from tests import views as V
from tests.test_gpu_grain import _to_dev
from tests.nlf_lags_content import SUBSAMPLINGS, clip_frames, gpu_content

pytestmark = pytest.mark.gpu
TILE_W, TILE_H_LUMA, TILE_H_CHROMA = 64, 32, 16  # k_nlf_lags' tile: the luma launch's and the chroma launch's
FORMATS = ((8, "444"), (10, "mono"), (12, "444"), (10, "420"), (8, "422"), (12, "420"))


@pytest.fixture(scope="module")
def meters():
    from grav1synth_amd.estimate import NoiseLevelMeter

    made = {}

    def get(bd, lags=True, **kw):
        key = (bd, lags, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = NoiseLevelMeter(bd, lags=lags, temporal=True, **kw)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def check_run(meters, frames, bd, subx, suby, what, where="device", wants=None, **kw):
    """One run through a lag meter and a plain temporal meter (cut first): the lag records against the reference, the
    ordinary and temporal records against the temporal meter's."""
    meter, plain = meters(bd, **kw), meters(bd, lags=False, **kw)
    meter.cut()
    plain.cut()
    keep = []
    for k, planes in enumerate(frames):
        dev = where == "device" or (where == "mixed" and k % 2 == 0)
        keep.append(_to_dev(planes, bd) if dev else planes)
        meter.frame(keep[-1], subx, suby)
        plain.frame(planes, subx, suby)
    got, tgot, lgot = meter.finish(), meter.finish_temporal(), meter.finish_lags()
    assert len(got) == len(frames) and len(tgot) == len(lgot) == len(frames) - 1, (what, len(got), len(tgot), len(lgot))
    assert got.tobytes() == plain.finish().tobytes() and tgot.tobytes() == plain.finish_temporal().tobytes(), f"{what}: the other records are a temporal meter's"
    wants = LG.run_records(frames, bd, subx, suby) if wants is None else wants
    bad = []
    for k, want in enumerate(wants):
        bad += LG.mismatches(lgot[k], want, f"{what}: pair {k}")
        for c in range(len(frames[0])):  # L3's identities, on the device's own records
            t = tgot[k]
            assert int(lgot[k]["n"][c, 0]) == int(t["n"][c].sum()) and int(lgot[k]["r"][c, 0]) == int(t["q"][c].sum()) and int(lgot[k]["s"][c]) == int(t["s"][c].sum())
    assert not bad, "\n".join(bad[:40])
    return wants


# ------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
def test_formats(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    frames = gpu_content(bd, ss)
    wants = check_run(meters, frames, bd, subx, suby, f"{bd} bit {ss}")
    w = wants[0]
    assert w["n"][0].min() > 0 and np.unique(w["r"][0]).size > 40 and w["s"][0] != 0
    if ss != "mono":
        assert w["xn"].min() > 0 and w["xr"].any() and w["ln"] > 0 and w["ls"] != 0 and not np.array_equal(w["r"][1], w["r"][2])
    else:
        assert not w["n"][1:].any() and not w["xn"].any() and w["ln"] == 0 and w["l2"] == 0


@pytest.mark.parametrize("w", [TILE_W - 1, TILE_W, TILE_W + 1, TILE_W + 3, TILE_W + 7, 2 * TILE_W, 3 * TILE_W - 1])
def test_sizes_round_the_tile(meters, w):
    """One below, on and above the tile in each direction; a last tile column 1 .. 7 samples wide, a last tile row 1 .. 4
    high, for the luma launch's rows (32) and, at 4:4:4, the chroma launch's (16)."""
    for i, h in enumerate((15, 16, 17, 20, 31, 32, 33, 34, 35, 36, 65)):
        bd, ss = FORMATS[(i + w) % 4]  # (luma and chroma planes of one size)
        subx, suby = SUBSAMPLINGS[ss]
        wants = check_run(meters, clip_frames(w, h, bd, ss, seed=2), bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
        assert wants[0]["n"][0, :20].min() > 0


@pytest.mark.parametrize("w", [1, 2, 3, 4, 6, 7, 9])
def test_planes_narrower_than_the_window(meters, w):
    for h in (1, 2, 3, 4, 5, 37):
        for bd, ss in FORMATS:
            subx, suby = SUBSAMPLINGS[ss]
            wants = check_run(meters, clip_frames(w, h, bd, ss, seed=2, amp=1, fade=0, wild=0), bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
            assert (w >= 3 and h >= 3) or not wants[0]["n"].any()
    for bd, ss in FORMATS:
        subx, suby = SUBSAMPLINGS[ss]
        check_run(meters, clip_frames(130, w, bd, ss, seed=3, amp=1, wild=0), bd, subx, suby, f"130x{w} {bd} bit {ss}")


@pytest.mark.parametrize("size", [(3 * TILE_W - 20, 3 * TILE_H_LUMA - 10), (3 * TILE_W - 21, 3 * TILE_H_LUMA - 11), (2 * TILE_W + 1, 2 * TILE_H_LUMA + 1),
                                  (4 * TILE_W, 4 * TILE_H_CHROMA), (2 * TILE_W + 13, 2 * TILE_H_CHROMA + 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiles_of_luma_over_tiles_of_chroma(meters, size):
    """3 x 3 tiles of luma over 2 x 2 (and, by rows, 2 x 3) of chroma, from even and odd luma sizes."""
    w, h = size
    for bd, ss in ((8, "420"), (10, "422"), (12, "420"), (10, "420")):
        subx, suby = SUBSAMPLINGS[ss]
        wants = check_run(meters, clip_frames(w, h, bd, ss, seed=9, n=3), bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
        assert wants[1]["xn"].min() > 0 and wants[1]["n"][2].min() > 0


# ------------------------------------------------------------------------------------------------------ designed content
def _positions():
    """A sample of every position class of a luma tile (and, at 4:4:4, of a chroma tile): interior, each ring of the window,
    the corners four tiles share."""
    xs = (2, 5, 6, 7, TILE_W - 8, TILE_W - 7, TILE_W - 6, TILE_W - 1, TILE_W, TILE_W + 1, TILE_W + 5, TILE_W + 6, TILE_W + 7, 2 * TILE_W - 1, 2 * TILE_W)
    ys = (2, 3, 4, 5, TILE_H_CHROMA - 3, TILE_H_CHROMA - 1, TILE_H_CHROMA, TILE_H_CHROMA + 1, TILE_H_LUMA - 4, TILE_H_LUMA - 3, TILE_H_LUMA - 1, TILE_H_LUMA,
          TILE_H_LUMA + 1, TILE_H_LUMA + 3, 2 * TILE_H_LUMA)
    return [(x, ys[(3 * i) % len(ys)]) for i, x in enumerate(xs)] + [(xs[(2 * i + 1) % len(xs)], y) for i, y in enumerate(ys)]


@pytest.mark.parametrize("bd", [8, 12])
def test_one_edge_pixel_in_every_position_class_of_a_tile(meters, bd):
    """Flat frames with a little noise, all counting, but for one pixel far off in both frames: its eight neighbours are
    ungated (the pixel's own gradient is zero), and n drops at exactly the lags with a pair that touches them -- which those are
    is the reference's to say; that the lags along the row drop, and most of the others, is asserted here."""
    up = 1 << (bd - 8)
    w, h = 2 * TILE_W + 9, 2 * TILE_H_LUMA + 7
    rng = np.random.default_rng(bd)
    base = [[(100 * up + rng.integers(0, 2 * up, (h, w))).astype(np.uint8 if bd == 8 else np.uint16) for _ in range(3)] for _ in range(2)]
    full = LG.lags_pair(base[1], base[0], bd, 0, 0)
    assert int(full["n"][1, 0]) == (w - 2) * (h - 2)
    for x, y in _positions():
        frames = [[p.copy() for p in f] for f in base]
        for f in frames:
            for p in f:
                p[y, x] = 250 * up
        want = check_run(meters, frames, bd, 0, 0, f"{bd} bit, edge pixel at ({x}, {y})")[0]
        assert (want["n"] <= full["n"]).all() and (want["xn"] <= full["xn"]).all() and int(want["n"][0, 0]) == (w - 2) * (h - 2) - 8
        assert (want["n"][:, :7] < full["n"][:, :7]).all() and (want["xn"][:, 21:] < full["xn"][:, 21:]).all() and np.count_nonzero(want["n"] < full["n"]) > 3 * 30


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_one_differing_sample_at_tile_corners(meters, bd):
    """Otherwise equal frames: one e is not zero, so r[0] is its square and every other sum of products is zero."""
    up = 1 << (bd - 8)
    w, h = 2 * TILE_W + 9, 2 * TILE_H_LUMA + 7
    base = clip_frames(w, h, bd, "444", seed=12, n=1, amp=1, wild=0)[0]
    for x, y in ((1, 1), (TILE_W - 1, TILE_H_LUMA - 1), (TILE_W, TILE_H_LUMA), (TILE_W - 1, TILE_H_CHROMA), (TILE_W, TILE_H_CHROMA - 1), (w - 2, h - 2),
                 (0, 0), (w - 1, h - 1)):
        before = [p.copy() for p in base]
        for p in before:
            p[y, x] = p[y, x] + 3 * up if p[y, x] < (1 << bd) - 3 * up else p[y, x] - 3 * up
        want = check_run(meters, [before, base], bd, 0, 0, f"{bd} bit, ({x}, {y})")[0]
        interior = 1 <= x <= w - 2 and 1 <= y <= h - 2
        assert all(int(v) in (9 * up * up, 0) for v in want["r"][:, 0]) and (interior or not want["r"].any()), "the one difference, where it counts"
        assert not want["r"][:, 1:].any() and abs(int(want["xr"][0, 24])) in (9 * up * up, 0) and not want["xr"][:, :24].any()


def test_the_largest_differences_that_count(meters):
    """12 bit, 200 x 75 at 4:4:4: the spikes of tests/test_gpu_nlf_t.py in every third sample of every tile, e = +- 4088.  A
    lane's 32-bit sum takes several products of nearly 2^24, a wave's leaves 32 bits, and the lag (3, 0) sees them too."""
    w, h = 200, 75
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    spike = (xs % 3 == 1) & (ys % 3 == 1)
    a = np.where(spike, 0, 2048).astype(np.uint16)
    b = np.where(spike, 4088, 2048 - 511).astype(np.uint16)
    wants = check_run(meters, [[a, b, a], [b, a, b], [a, a, a]], 12, 0, 0, "spikes")
    assert int(wants[0]["r"][0, 0]) > 2 ** 32 and int(wants[0]["r"][0, 3]) > 2 ** 32 and int(wants[0]["l2"]) > 2 ** 32
    assert int(wants[0]["xr"][1, 24]) > 2 ** 32 and int(wants[1]["r"][0, 0]) == int(wants[0]["r"][0, 0]) and int(wants[1]["s"][0]) == -int(wants[0]["s"][0])
    assert int(wants[0]["xr"][0, 24]) < -2 ** 32, "luma against a chroma plane that went the other way"


@pytest.mark.parametrize("ss", ["420", "422"])
def test_negative_box_sums_and_a_fade(meters, ss):
    """A fade down: every e is negative, so Round2's arithmetic shift rounds negative box sums."""
    subx, suby = SUBSAMPLINGS[ss]
    bd = 10
    rng = np.random.default_rng(8)
    frames = []
    for t in range(3):
        frames.append([(600 - 9 * t + rng.integers(0, 4, s)).astype(np.uint16) for s in ((75, 151), ((75 + suby) >> suby, 76), ((75 + suby) >> suby, 76))])
    wants = check_run(meters, frames, bd, subx, suby, f"fade {ss}")
    right, wrong = wants[0], LG.lags_pair(frames[1], frames[0], bd, subx, suby, truncate=True)
    assert int(right["ls"]) < -5 * int(right["ln"]) < 0 and int(right["s"][1]) < 0
    # (a box of two: Round2 of a negative odd sum rounds towards zero as truncation does; a box of four tells them apart)
    assert (int(right["ls"]) != int(wrong["ls"])) == (ss == "420")


# ------------------------------------------------------------------------------------------------------------ plumbing
@pytest.mark.parametrize("bd,ss", [(8, "420"), (10, "422"), (12, "444")])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    isz = 1 if bd == 8 else 2
    frames = clip_frames(211, 71, bd, ss, seed=4, n=3)
    wants = LG.run_records(frames, bd, subx, suby)
    m = meters(bd)
    for k, (extra, base) in enumerate(((6, 2), (34, 14), (0, 250), (130, 6))):
        m.cut()
        guards, keep = [], []
        for t, planes in enumerate(frames):
            dev = []
            for c, p in enumerate(planes):  # (the two frames of a pair have pitches of their own)
                view, guard = V.device_view(p, pitch_bytes=p.shape[1] * isz + (extra + 4 * t) * isz, base_offset_bytes=(base + 2 * c + 6 * t) % 256 & ~(isz - 1),
                                            fill="random" if k & 1 else "max", max_code=(1 << bd) - 1, seed=10 * k + c)
                dev.append(view)
                guards.append(guard)
            keep.append(dev)
            m.frame(dev, subx, suby)
        lgot = m.finish_lags()
        bad = []
        for t in range(2):
            bad += LG.mismatches(lgot[t], wants[t], f"view {k} pair {t}")
        assert not bad, "\n".join(bad[:40])
        for g in guards:
            g.assert_unchanged(f"view {k}")
        m.finish(), m.finish_temporal()


def test_host_pinned_and_device_frames_in_one_run(meters):
    import torch

    bd, (subx, suby) = 10, (1, 1)
    frames = clip_frames(150, 90, bd, "420", seed=30, n=9)
    wants = LG.run_records(frames, bd, subx, suby)
    for batch in (4, 16):
        m = meters(bd, batch_frames=batch)
        m.cut()
        keep = []
        for k, planes in enumerate(frames):
            kind = (k + k // 3) % 3  # (every kind follows every kind)
            if kind == 1:
                planes = _to_dev(planes, bd)
            elif kind == 2:
                planes = [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
            keep.append(planes)
            m.frame(planes, subx, suby, async_host=True)
        lgot = m.finish_lags()
        assert len(lgot) == 8 and len(m.finish()) == 9 and len(m.finish_temporal()) == 8
        bad = []
        for k in range(8):
            bad += LG.mismatches(lgot[k], wants[k], f"batch {batch} pair {k}")
        assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("batch", [1, 2, 5, 6])
@pytest.mark.parametrize("where", ["device", "host", "mixed"])
def test_batches_of_one_of_two_of_all_and_of_one_more(batch, where):
    """The predecessor of a batch's first frame is the last frame of the batch before: a device frame the caller has let go
    of by then (its tensor is overwritten here), a host frame whose slot has been handed on."""
    from grav1synth_amd.estimate import NoiseLevelMeter

    bd, n = 8, 5
    frames = clip_frames(70, 50, bd, "420", seed=60, n=n)
    wants = LG.run_records(frames, bd, 1, 1)
    m = NoiseLevelMeter(bd, batch_frames=batch, lags=True)
    plain = NoiseLevelMeter(bd, batch_frames=batch, temporal=True)
    for k, planes in enumerate(frames):
        dev = where == "device" or (where == "mixed" and k & 1)
        handed = _to_dev(planes, bd) if dev else [p.copy() for p in planes]
        m.frame(handed, 1, 1)
        plain.frame(planes, 1, 1)
        if (k + 1) % batch == 0:  # the batch has gone out: the planes are the caller's again
            for p in handed:
                if dev:
                    p.fill_(255)
                else:
                    p[...] = 255
    lgot, tgot, got = m.finish_lags(), m.finish_temporal(), m.finish()  # (the three hand-overs in another order)
    assert len(got) == n and len(tgot) == len(lgot) == n - 1
    assert got.tobytes() == plain.finish().tobytes() and tgot.tobytes() == plain.finish_temporal().tobytes()
    for k in range(n - 1):
        bad = LG.mismatches(lgot[k], wants[k], f"batch {batch} pair {k}")
        assert not bad, "\n".join(bad[:40])
    m.close()
    plain.close()


def test_capacity_a_geometry_change_a_cut_the_hand_overs_interleaved_and_reuse():
    from grav1synth_amd.estimate import NLF_LRECORD, NoiseLevelMeter

    bd = 8
    m = NoiseLevelMeter(bd, batch_frames=4, lags=True)
    a = clip_frames(70, 50, bd, "420", seed=70, n=6)  # a batch and two queued frames
    b = clip_frames(33, 41, bd, "444", seed=80, n=3)  # another geometry in mid-queue sends the queue out and ends the run
    c = clip_frames(33, 41, bd, "444", seed=81, n=2)  # the same geometry after a cut: no pair across it
    wants = LG.run_records(a, bd, 1, 1) + LG.run_records(b, bd, 0, 0) + LG.run_records(c, bd, 0, 0)
    for f in a:
        m.frame(f, 1, 1)
    assert len(m.finish_temporal()) == 5  # (a hand-over of another kind sends the queue out; the lag records stay)
    for f in b:
        m.frame(_to_dev(f, bd), 0, 0)
    m.cut()
    m.cut()
    for f in c:
        m.frame(f, 0, 0)
    n = C.c_size_t()
    small = np.zeros(7, NLF_LRECORD)
    assert m._L.g1s_nlf_finish_lags(m._h, small.ctypes.data, 7, C.byref(n)) == _lib.G1S_ERR_CAPACITY and n.value == 8
    assert m._L.g1s_nlf_finish_lags(m._h, None, 0, C.byref(n)) == _lib.G1S_ERR_CAPACITY and n.value == 8
    with pytest.raises(_lib.G1SError):
        m.finish_lags(cap=7)
    lgot = m.finish_lags()
    assert len(lgot) == 8 == len(wants)
    for k in range(8):
        bad = LG.mismatches(lgot[k], wants[k], f"pair {k}")
        assert not bad, "\n".join(bad[:40])
    assert len(m.finish_lags()) == 0 and len(m.finish()) == 11 and len(m.finish_temporal()) == 3
    # the run goes on over a hand-over: frame c[1] is still the predecessor
    more = clip_frames(33, 41, bd, "444", seed=81, n=3)[2]
    m.frame(more, 0, 0)
    lgot = m.finish_lags()
    assert len(lgot) == 1 and not LG.mismatches(lgot[0], LG.lags_pair(more, c[1], bd, 0, 0), "after a hand-over")
    mono = clip_frames(33, 41, bd, "mono", seed=82, n=2)
    for f in mono:
        m.frame(f, 0, 0)
    lgot = m.finish_lags()
    assert len(lgot) == 1 and not LG.mismatches(lgot[0], LG.run_records(mono, bd, 0, 0)[0], "luma only")
    assert not lgot[0]["n"][1:].any() and not lgot[0]["xn"].any() and lgot[0]["ln"] == 0, "a luma-only pair has zeros for what chroma adds"
    m.close()


@pytest.mark.parametrize("temporal", [False, True])
def test_meters_of_the_other_kinds_refuse_and_go_on(temporal):
    from grav1synth_amd.estimate import NoiseLevelMeter

    m = NoiseLevelMeter(8, temporal=temporal)
    frames = clip_frames(40, 30, 8, "420", seed=1)
    for f in frames:
        m.frame(f, 1, 1)
    with pytest.raises(_lib.G1SError) as e:
        m.finish_lags()
    assert "not a lag meter: make it with g1s_nlf_new_lags" in str(e.value)
    assert m.kernel_times_lags() == (0.0, 0.0, 0)
    assert len(m.finish()) == 2, "the refusal is not sticky"
    m.close()


def test_the_lag_launches_are_timed(meters):
    m = meters(10, batch_frames=3)
    m.kernel_times(True)
    m.cut()
    for f in gpu_content(n=4):
        m.frame(f, 1, 1)
    assert len(m.finish_lags()) == 3
    luma, chroma, pairs = m.kernel_times_lags()
    assert luma > 0 and chroma > 0 and pairs == 3
    m.kernel_times(False)
    m.finish(), m.finish_temporal()


def test_the_longest_side(meters):
    """65 536 samples a side, 8 the other way."""
    bd = 8
    rng = np.random.default_rng(6)
    for w, h in ((65536, 8), (8, 65536)):
        frames = [[(100 + rng.integers(0, 4, (h, w))).astype(np.uint8)] for _ in range(2)]
        want = check_run(meters, frames, bd, 0, 0, f"{w}x{h}")[0]
        assert int(want["n"][0, 0]) == (w - 2) * (h - 2) and int(want["n"][0, 45]) == (max(w - 8, 0)) * (max(h - 5, 0))


# ------------------------------------------------------------------------------------------------------------ commands
def _run(*args):
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, "-m", "grav1synth_amd", *args], env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=900,
                          cwd=root, stdin=subprocess.DEVNULL)


def test_estimate_table_end_to_end(tmp_path):
    """`estimate --table` byte for byte against the host functions on the reference records: all frames, a prefix with another
    lag and Nmin, and beside the two reports; the refusal of a one-frame clip writes nothing; the table is one `denoise
    --grain-prior` accepts."""
    from fractions import Fraction

    from grav1synth_amd.diff import format_tbl
    from grav1synth_amd.estimate import NLF_LRECORD, NLF_TRECORD, noise_table
    from grav1synth_amd.ingest import write_y4m
    from tests import nlf_t_ref as T
    from tests.nlf_lags_content import ar_clip

    bd, n = 10, 5
    frames = ar_clip(n=n, seed=33, w=160, h=96)
    src = tmp_path / "src.y4m"
    write_y4m(str(src), frames, bd, 1, 1, Fraction(24, 1))

    def want(k, lag, nmin):
        t = T.to_struct(T.sum_records(T.run_records(frames[:k], bd, 1, 1)), NLF_TRECORD)
        l = LG.to_struct(LG.sum_records(LG.run_records(frames[:k], bd, 1, 1)), NLF_LRECORD)
        return format_tbl([noise_table(t, l, bd, 1, 1, 3, lag, nmin)])

    out, tbl = tmp_path / "est.txt", tmp_path / "clip.tbl"
    p = _run("estimate", str(src), "-o", str(out), "--table", str(tbl), "--levels-min-count", "1000")
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Done, wrote the clip's grain table to {tbl}" in p.stderr and tbl.read_bytes() == want(n, 3, 1000)
    plain = tmp_path / "plain.txt"
    p = _run("estimate", str(src), "-o", str(plain))
    assert p.returncode == 0 and plain.read_bytes() == out.read_bytes(), "the estimates are what they were"
    out2, tbl2, lev, tlev = tmp_path / "est2.txt", tmp_path / "clip2.tbl", tmp_path / "lev.txt", tmp_path / "tlev.txt"
    p = _run("estimate", str(src), "-o", str(out2), "--table", str(tbl2), "--table-lag", "2", "--profile-frames", "3", "--levels-min-count", "500", "--levels", str(lev),
             "--levels-temporal", str(tlev))
    assert p.returncode == 0, p.stderr[-2000:]
    assert tbl2.read_bytes() == want(3, 2, 500) and tbl2.read_bytes() != tbl.read_bytes()
    # the two level reports are of the whole clip, whatever the table is made from: the bytes of a job without --table
    out4, lev4, tlev4 = tmp_path / "est4.txt", tmp_path / "lev4.txt", tmp_path / "tlev4.txt"
    p = _run("estimate", str(src), "-o", str(out4), "--levels", str(lev4), "--levels-temporal", str(tlev4))
    assert p.returncode == 0 and lev.read_bytes() == lev4.read_bytes() and tlev.read_bytes() == tlev4.read_bytes() and out2.read_bytes() == out4.read_bytes()
    assert b"frames 5 " in lev.read_bytes() and b"pairs 4 " in tlev.read_bytes()
    # --lags: the report of the table's frames, byte for byte the host function's on the reference record
    out5, tbl5, lags5 = tmp_path / "est5.txt", tmp_path / "clip5.tbl", tmp_path / "clip5.lags"
    p = _run("estimate", str(src), "-o", str(out5), "--table", str(tbl5), "--lags", str(lags5), "--profile-frames", "4", "--levels-min-count", "800")
    assert p.returncode == 0 and f"Done, wrote the lag report to {lags5}" in p.stderr, p.stderr[-2000:]
    l4 = LG.sum_records(LG.run_records(frames[:4], bd, 1, 1))
    assert lags5.read_bytes() == LG.format_noise_lags(l4, 3, bd, 3, 3, 800) and tbl5.read_bytes() == want(4, 3, 800)
    p = _run("estimate", str(src), "-o", str(tmp_path / "no.txt"), "--lags", str(tmp_path / "no.lags"))
    assert "they need it. Exiting." in p.stderr and not (tmp_path / "no.txt").exists() and not (tmp_path / "no.lags").exists()
    # the default Nmin of 4096 is above this clip's chroma counts: the host function's refusal, nothing written
    out3, tbl3 = tmp_path / "est3.txt", tmp_path / "clip3.tbl"
    p = _run("estimate", str(src), "-o", str(out3), "--table", str(tbl3), "--profile-frames", "2")
    assert "too few static sample pairs for a table. Exiting." in p.stderr and not out3.exists() and not tbl3.exists()
    one = tmp_path / "one.y4m"
    write_y4m(str(one), frames[:1], bd, 1, 1, Fraction(24, 1))
    p = _run("estimate", str(one), "-o", str(out3), "--table", str(tbl3))
    assert "a table needs two frames. Exiting." in p.stderr and not out3.exists() and not tbl3.exists()
    p = _run("estimate", str(src), "-o", str(out3), "--table", str(tbl3), "--profile-frames", "1")
    assert "a table needs two frames. Exiting." in p.stderr and not out3.exists() and not tbl3.exists()
    den = tmp_path / "den.y4m"
    p = _run("denoise", str(src), "-o", str(den), "--grain-prior", str(tbl))
    assert p.returncode == 0 and den.exists(), p.stderr[-2000:]


def test_the_file_driver(tmp_path):
    """g1s_nlf_y4m_file_table: the table, the lag report and the two level reports of the first max_frames frames, byte for
    byte the host functions' on the reference records and the command's; its refusals write nothing."""
    from fractions import Fraction

    from grav1synth_amd.diff import format_tbl
    from grav1synth_amd.estimate import NLF_LRECORD, NLF_TRECORD, noise_levels_y4m_file, noise_table, noise_table_y4m_file
    from grav1synth_amd.ingest import write_y4m
    from tests import nlf_t_ref as T
    from tests.nlf_lags_content import ar_clip

    bd, n = 10, 5
    frames = ar_clip(n=n, seed=34, w=160, h=96)
    src = tmp_path / "src.y4m"
    write_y4m(str(src), frames, bd, 1, 1, Fraction(24, 1))
    for k, lag, nmin, batch in ((0, 3, 1000, 2), (3, 2, 500, 0)):
        use = frames[:k or n]
        t = T.sum_records(T.run_records(use, bd, 1, 1))
        l = LG.sum_records(LG.run_records(use, bd, 1, 1))
        tbl, lev, tlev, lags = (tmp_path / f"{k}.{ext}" for ext in ("tbl", "lev", "tlev", "lags"))
        got_n, seg = noise_table_y4m_file(str(src), str(tbl), levels=str(lev), levels_temporal=str(tlev), lags=str(lags), batch_frames=batch, max_frames=k, lag=lag,
                                          min_count=nmin)
        want = noise_table(T.to_struct(t, NLF_TRECORD), LG.to_struct(l, NLF_LRECORD), bd, 1, 1, 3, lag, nmin)
        assert got_n == len(use) and seg == want and tbl.read_bytes() == format_tbl([want])
        assert lags.read_bytes() == LG.format_noise_lags(l, len(use) - 1, bd, 3, lag, nmin)
        lev2, tlev2 = tmp_path / f"{k}.lev2", tmp_path / f"{k}.tlev2"
        noise_levels_y4m_file(str(src), str(lev2), max_frames=k, temporal_report=str(tlev2))
        assert lev.read_bytes() == lev2.read_bytes() and tlev.read_bytes() == tlev2.read_bytes()
    got_n, seg = noise_table_y4m_file(str(src), None, min_count=1000)
    assert got_n == n and seg.ar_coeff_lag == 3, "no file at all"
    for kw, text in ((dict(max_frames=1), "a table needs two frames"), (dict(max_frames=2), "too few static sample pairs for a table"), (dict(lag=4), "lag is 1, 2 or 3"),
                     (dict(lag=0), "lag is 1, 2 or 3")):
        tbl, lags = tmp_path / "no.tbl", tmp_path / "no.lags"
        with pytest.raises(_lib.G1SError) as e:
            noise_table_y4m_file(str(src), str(tbl), lags=str(lags), levels=str(tmp_path / "no.lev"), **kw)
        assert text in str(e.value) and not tbl.exists() and not lags.exists() and not (tmp_path / "no.lev").exists()
    with pytest.raises(_lib.G1SError):
        noise_table_y4m_file(str(tmp_path / "missing.y4m"), str(tmp_path / "no.tbl"))
