"""Temporal noise levels on the device against tests/nlf_t_ref.py: every field of every temporal record with array_equal,
beside the ordinary records against tests/nlf_ref.py and a plain meter's; every report byte for byte.  There is no tolerance
anywhere."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import nlf_ref as R
from tests import nlf_t_ref as T
from tests import views as V
from tests.test_gpu_grain import _to_dev
from tests.test_nlf_cpu import SUBSAMPLINGS, smooth_planes
from tests.test_nlf_t_cpu import box_edge_pair, clip_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP_COLS, STRIP_ROWS = 496, 32  # k_nlf_t's strip of a wave


@pytest.fixture(scope="module")
def meters():
    from grav1synth_amd.estimate import NoiseLevelMeter

    made = {}

    def get(bd, **kw):
        key = (bd, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = NoiseLevelMeter(bd, temporal=True, **kw)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def check_run(meter, frames, bd, subx, suby, what, where="device", wants=None):
    """One run through the meter (cut first): the ordinary records and the temporal records against the references."""
    meter.cut()
    keep = []
    for k, planes in enumerate(frames):
        dev = where == "device" or (where == "mixed" and k % 2 == 0)
        keep.append(_to_dev(planes, bd) if dev else planes)
        meter.frame(keep[-1], subx, suby)
    got, tgot = meter.finish(), meter.finish_temporal()
    assert len(got) == len(frames) and len(tgot) == len(frames) - 1, (what, len(got), len(tgot))
    wants = T.run_records(frames, bd, subx, suby) if wants is None else wants
    bad = []
    for k, planes in enumerate(frames):
        bad += R.mismatches(got[k], R.nlf_frame(planes, bd, subx, suby), f"{what}: frame {k}")
    for k, want in enumerate(wants):
        bad += T.mismatches(tgot[k], want, f"{what}: pair {k}")
    assert not bad, "\n".join(bad)
    return wants


# ------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
def test_formats(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    frames = clip_frames(208, 136, bd, ss, seed=3, n=3)
    wants = check_run(meters(bd), frames, bd, subx, suby, f"{bd} bit {ss}")
    assert wants[0]["q"][0].any() and np.count_nonzero(wants[0]["n"][0]) > 3 and (wants[0]["s"][0] < 0).any() and (wants[0]["s"][0] > 0).any()
    assert ss == "mono" or (wants[1]["q"][1].any() and not np.array_equal(wants[1]["q"][1], wants[1]["q"][2])), "the planes differ"


WIDTHS = (495, 496, 497, 498, 993)
HEIGHTS = (31, 32, 33, 34, 65)
FORMATS = ((8, "444"), (10, "mono"), (12, "444"), (10, "420"), (8, "422"))


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_below_and_on_the_stencil(meters, size):
    w, h = size
    for bd, ss in FORMATS:
        subx, suby = SUBSAMPLINGS[ss]
        wants = check_run(meters(bd), clip_frames(w, h, bd, ss, seed=2, amp=1, fade=0), bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
        assert w == 3 or not wants[0]["n"].any()


@pytest.mark.parametrize("w", WIDTHS + (994,))
def test_sizes_round_the_strip(meters, w):
    """A strip's last column and row, and a second strip of one column or row: 496 output columns from column 0 and 32 output
    rows from row 1 (and with 35 and 67 rows the strip after)."""
    for i, h in enumerate(HEIGHTS + (35, 67)):
        bd, ss = FORMATS[(i + w) % len(FORMATS)]
        subx, suby = SUBSAMPLINGS[ss]
        wants = check_run(meters(bd), clip_frames(w, h, bd, ss, seed=2), bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
        assert wants[0]["n"][0].sum() > 0


@pytest.mark.parametrize("size", [(995, 37), (2 * 994 + 1, 5), (37, 131), (5, 5), (7, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_odd_luma_sizes_under_decimated_chroma(meters, size):
    w, h = size
    for bd, ss in ((8, "420"), (10, "422"), (12, "420")):
        subx, suby = SUBSAMPLINGS[ss]
        wants = check_run(meters(bd), clip_frames(w, h, bd, ss, seed=9), bd, subx, suby, f"{w}x{h} {bd} bit {ss}")
        assert w < 9 or wants[0]["n"][1].sum() > 0


# ------------------------------------------------------------------------------------------------- adversarial content
def test_a_checkerboard_against_its_inverse_and_against_itself(meters):
    """0 / 4095, 130 x 70.  Against its inverse every e^2 is at its ceiling and every sample is gated out by T2's third
    condition (the box sums differ by 4095); against itself every interior sample counts with e = 0."""
    w, h = 130, 70
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    board = np.where((xs + ys) & 1, 4095, 0).astype(np.uint16)
    inverse = (4095 - board).astype(np.uint16)
    a, b = [board, board[:, ::-1].copy(), board.copy()], [inverse, inverse[:, ::-1].copy(), inverse.copy()]
    wants = check_run(meters(12), [a, b, b], 12, 0, 0, "checkerboard")
    assert not wants[0]["n"].any() and not wants[0]["q"].any()
    assert int(wants[1]["n"][0].sum()) == (w - 2) * (h - 2) and not wants[1]["q"].any() and not wants[1]["s"].any()


def test_the_largest_differences_that_count(meters):
    """12 bit, 600 x 75: a lattice of isolated samples that go from 0 to 4095 or back while their eight neighbours go the
    other way by an eighth of it: the box sums stay and e^2 is near its ceiling.  A lane adds some thirty of them in a strip
    and a wave some two thousand: the wave's sum leaves 32 bits."""
    w, h = 600, 75
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    spike = (xs % 3 == 1) & (ys % 3 == 1)
    a = np.where(spike, 0, 2048).astype(np.uint16)
    b = np.where(spike, 4088, 2048 - 511).astype(np.uint16)  # (8 x 511 = 4088: the box sums are the same)
    wants = check_run(meters(12), [[a], [b], [a]], 12, 0, 0, "spikes")
    # (a spike's gradient is zero by symmetry: the spikes themselves count, their neighbours' gradients do not pass)
    assert int(wants[0]["q"][0].sum()) >= (w // 3 - 1) * (h // 3 - 1) * 4088 ** 2 and (wants[1]["s"][0] < 0).any()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_adversarial_bins(meters, bd):
    w, h, step, up = 600, 75, 1 << (bd - 5), 1 << (bd - 8)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    rng = np.random.default_rng(bd)
    dt = np.uint8 if bd == 8 else np.uint16
    cases = {
        "one intensity": lambda k: np.full((h, w), 11 * step + 3 + k),
        "one intensity with noise": lambda k: np.full((h, w), 11 * step + step // 2) + rng.integers(-2 * up, 2 * up + 1, (h, w)),
        # (a checkerboard of A = 8 step - 5 and B = 8 step + 4 against itself one code value up: the sum of the two box sums is
        # 18 (8 step) - 9 around an A and 18 (8 step) + 9 around a B)
        "two bins alternating sample by sample": lambda k: np.where((xs + ys) & 1, 8 * step - 5, 8 * step + 4) + k,
        "two bins, column by column": lambda k: np.where(xs & 1, 20 * step - 1 - k, 20 * step + 3 * up) + 0 * ys,
        "a ramp through all 32 bins": lambda k: np.minimum((xs * 32 * step) // w, (1 << bd) - 1) + 0 * ys + rng.integers(0, 2 * up + 1, (h, w)),
        "a ramp down the rows": lambda k: np.minimum((ys * 32 * step) // h, (1 << bd) - 1) + 0 * xs + k * up,
    }
    for what, make in cases.items():
        frames = []
        for k in range(2):
            luma = np.clip(make(k), 0, (1 << bd) - 1).astype(dt)
            frames.append([luma, np.ascontiguousarray(luma[::2, ::2]), np.ascontiguousarray(luma[::2, ::2][:, ::-1])])
        want = check_run(meters(bd), frames, bd, 1, 1, f"{bd} bit, {what}")[0]
        if what == "one intensity":
            assert np.count_nonzero(want["n"][0]) == 1 and int(want["n"][0].sum()) == (w - 2) * (h - 2) == int(want["s"][0].sum()) == int(want["q"][0].sum())
        if what.startswith("a ramp through"):
            assert np.count_nonzero(want["n"][0]) == 32
        if what.startswith("two bins alternating"):
            k = np.flatnonzero(want["n"][0])
            assert len(k) == 2 and abs(int(want["n"][0][k[0]]) - int(want["n"][0][k[1]])) <= 1, want["n"][0]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_a_predecessor_that_differs_in_one_sample_at_a_strips_corner(meters, bd):
    """One sample of frame t - 1 differs, by 3 eight-bit code values: nine box sums and nine gates see it, one e does.  At the
    first and last output sample of the first strip, the first of the strip beside it and of the strip below."""
    up = 1 << (bd - 8)
    w, h = 2 * STRIP_COLS + 9, 2 * STRIP_ROWS + 7
    base = smooth_planes(w, h, bd, "mono", seed=12, amp=1)[0]
    for x, y in ((1, 1), (STRIP_COLS - 1, STRIP_ROWS), (STRIP_COLS, 1), (STRIP_COLS - 1, STRIP_ROWS + 1), (STRIP_COLS, STRIP_ROWS + 1), (w - 2, h - 2),
                 (0, 0), (w - 1, h - 1)):
        before = base.copy()
        before[y, x] = before[y, x] + 3 * up if before[y, x] < (1 << bd) - 3 * up else before[y, x] - 3 * up
        want = check_run(meters(bd), [[before], [base]], bd, 0, 0, f"{bd} bit, ({x}, {y})")[0]
        interior = 1 <= x <= w - 2 and 1 <= y <= h - 2
        assert int(want["q"][0].sum()) in ((9 * up * up, 0) if interior else (0,)), "the one difference, where it counts"


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_box_sum_differences_on_and_one_below_the_gate(meters, bd):
    up = 1 << (bd - 8)
    cur, before = box_edge_pair(64, 40, bd)
    want = check_run(meters(bd), [before, cur], bd, 0, 0, f"{bd} bit box edge")[0]
    loose = T.nlf_pair(cur, before, bd, 0, 0, box_strict=False)
    n = int(want["n"][0].sum())
    assert 0 < n < int(loose["n"][0].sum()) == 62 * 38, "144 2^sh itself does not count, one below does"
    assert int(want["s"][0].sum()) > n * (16 * up - 1)


# ------------------------------------------------------------------------------------------------------------ plumbing
@pytest.mark.parametrize("bd,ss", [(8, "420"), (10, "422"), (12, "444")])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(meters, bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    isz = 1 if bd == 8 else 2
    frames = clip_frames(547, 71, bd, ss, seed=4, n=3)
    wants = T.run_records(frames, bd, subx, suby)
    assert wants[0]["n"][1].sum() > 0
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
        got, tgot = m.finish(), m.finish_temporal()
        bad = []
        for t in range(3):
            bad += R.mismatches(got[t], R.nlf_frame(frames[t], bd, subx, suby), f"view {k} frame {t}")
        for t in range(2):
            bad += T.mismatches(tgot[t], wants[t], f"view {k} pair {t}")
        assert not bad, "\n".join(bad)
        for g in guards:
            g.assert_unchanged(f"view {k}")


def test_host_pinned_and_device_frames_in_one_run(meters):
    import torch

    bd, (subx, suby) = 10, (1, 1)
    frames = clip_frames(150, 90, bd, "420", seed=30, n=9)
    wants = T.run_records(frames, bd, subx, suby)
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
        got, tgot = m.finish(), m.finish_temporal()
        assert len(got) == 9 and len(tgot) == 8
        bad = []
        for k in range(9):
            bad += R.mismatches(got[k], R.nlf_frame(frames[k], bd, subx, suby), f"batch {batch} frame {k}")
        for k in range(8):
            bad += T.mismatches(tgot[k], wants[k], f"batch {batch} pair {k}")
        assert not bad, "\n".join(bad)


@pytest.mark.parametrize("batch", [1, 2, 5, 6])
@pytest.mark.parametrize("where", ["device", "host", "mixed"])
def test_batches_of_one_of_two_of_all_and_of_one_more(batch, where):
    """The predecessor of a batch's first frame is the last frame of the batch before: a device frame the caller has let go
    of by then (its tensor is overwritten here), a host frame whose slot has been handed on."""
    from grav1synth_amd.estimate import NoiseLevelMeter

    bd, n = 8, 5
    frames = clip_frames(70, 50, bd, "420", seed=60, n=n)
    wants = T.run_records(frames, bd, 1, 1)
    m = NoiseLevelMeter(bd, batch_frames=batch, temporal=True)
    plain = NoiseLevelMeter(bd, batch_frames=batch)
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
    got, tgot, pgot = m.finish(), m.finish_temporal(), plain.finish()
    assert len(got) == n and len(tgot) == n - 1
    assert got.tobytes() == pgot.tobytes(), "the ordinary records are a plain meter's, byte for byte"
    for k in range(n - 1):
        bad = T.mismatches(tgot[k], wants[k], f"batch {batch} pair {k}")
        assert not bad, "\n".join(bad)
    m.close()
    plain.close()


def test_the_ordinary_records_of_a_temporal_meter_over_several_strips():
    """Three frames of 499 x 36, 10-bit 4:2:0, at batch_frames = 2: two column strips and two row strips in luma, one strip
    in chroma, a pair across a batch boundary and a last batch that is short.  Host, device, host: the device frame is its
    batch's last, so the meter keeps a copy of it (the tensor is overwritten once the batch has gone out).  The ordinary
    records are a plain meter's byte for byte, and both kinds of record are the references'."""
    from grav1synth_amd.estimate import NoiseLevelMeter

    bd, n = 10, 3
    frames = clip_frames(499, 36, bd, "420", seed=61, n=n)
    assert -(-(499 - 1) // STRIP_COLS) == 2 and -(-(36 - 2) // STRIP_ROWS) == 2
    m = NoiseLevelMeter(bd, batch_frames=2, temporal=True)
    plain = NoiseLevelMeter(bd, batch_frames=2)
    for k, planes in enumerate(frames):
        handed = _to_dev(planes, bd) if k == 1 else [p.copy() for p in planes]
        m.frame(handed, 1, 1)
        plain.frame(planes, 1, 1)
        if k == 1:
            for p in handed:
                p.fill_((1 << bd) - 1)
    got, tgot, pgot = m.finish(), m.finish_temporal(), plain.finish()
    assert len(got) == n and len(tgot) == n - 1 and len(pgot) == n
    assert got.tobytes() == pgot.tobytes(), "the ordinary records are a plain meter's, byte for byte"
    bad = []
    for k in range(n):
        bad += R.mismatches(got[k], R.nlf_frame(frames[k], bd, 1, 1), f"frame {k}")
    for k, want in enumerate(T.run_records(frames, bd, 1, 1)):
        bad += T.mismatches(tgot[k], want, f"pair {k}")
    assert not bad, "\n".join(bad)
    m.close()
    plain.close()


def test_capacity_a_geometry_change_a_cut_and_reuse():
    from grav1synth_amd.estimate import NLF_TRECORD, NoiseLevelMeter

    bd = 8
    m = NoiseLevelMeter(bd, batch_frames=4, temporal=True)
    a = clip_frames(70, 50, bd, "420", seed=70, n=6)  # a batch and two queued frames
    b = clip_frames(33, 41, bd, "444", seed=80, n=3)  # another geometry in mid-queue sends the queue out and ends the run
    c = clip_frames(33, 41, bd, "444", seed=81, n=2)  # the same geometry after a cut: no pair across it
    wants = T.run_records(a, bd, 1, 1) + T.run_records(b, bd, 0, 0) + T.run_records(c, bd, 0, 0)
    for f in a:
        m.frame(f, 1, 1)
    for f in b:
        m.frame(_to_dev(f, bd), 0, 0)
    m.cut()
    m.cut()
    for f in c:
        m.frame(f, 0, 0)
    n = C.c_size_t()
    small = np.zeros(7, NLF_TRECORD)
    assert m._L.g1s_nlf_finish_temporal(m._h, small.ctypes.data, 7, C.byref(n)) == _lib.G1S_ERR_CAPACITY and n.value == 8
    assert m._L.g1s_nlf_finish_temporal(m._h, None, 0, C.byref(n)) == _lib.G1S_ERR_CAPACITY and n.value == 8
    with pytest.raises(_lib.G1SError):
        m.finish_temporal(cap=7)
    tgot = m.finish_temporal()
    assert len(tgot) == 8 == len(wants)
    for k in range(8):
        bad = T.mismatches(tgot[k], wants[k], f"pair {k}")
        assert not bad, "\n".join(bad)
    assert len(m.finish_temporal()) == 0 and len(m.finish()) == 11
    # the run goes on over a hand-over: frame c[1] is still the predecessor
    more = clip_frames(33, 41, bd, "444", seed=81, n=3)[2]
    m.frame(more, 0, 0)
    tgot = m.finish_temporal()
    assert len(tgot) == 1 and not T.mismatches(tgot[0], T.nlf_pair(more, c[1], bd, 0, 0), "after a hand-over")
    mono = clip_frames(33, 41, bd, "mono", seed=82, n=2)
    for f in mono:
        m.frame(f, 0, 0)
    tgot = m.finish_temporal()
    assert len(tgot) == 1 and not T.mismatches(tgot[0], T.run_records(mono, bd, 0, 0)[0], "luma only")
    assert not tgot[0]["n"][1:].any() and not tgot[0]["q"][1:].any(), "a luma-only pair has zeros for the chroma planes"
    m.close()


def test_a_plain_meter_refuses_and_goes_on():
    from grav1synth_amd.estimate import NoiseLevelMeter

    m = NoiseLevelMeter(8)
    planes = smooth_planes(40, 30, 8, "420", seed=1)
    m.frame(planes, 1, 1)
    with pytest.raises(_lib.G1SError) as e:
        m.finish_temporal()
    assert "not a temporal meter: make it with g1s_nlf_new_temporal" in str(e.value)
    m.cut()  # (nothing to end)
    got = m.finish()
    assert len(got) == 1 and not R.mismatches(got[0], R.nlf_frame(planes, 8, 1, 1), "the refusal is not sticky")
    m.close()


def test_the_longest_side(meters):
    """65 536 samples a side, 8 the other way."""
    bd = 8
    rng = np.random.default_rng(6)
    for w, h in ((65536, 8), (8, 65536)):
        frames = []
        for k in range(2):
            y = (100 + rng.integers(0, 4, (h, w))).astype(np.uint8)
            if w > h:  # (another bin in the last strip)
                y[:, -3:] = 180 + rng.integers(0, 4, (h, 3))
            else:
                y[-3:, :] = 180 + rng.integers(0, 4, (3, w))
            frames.append([y])
        want = check_run(meters(bd), frames, bd, 0, 0, f"{w}x{h}")[0]
        assert int(want["n"][0].sum()) > (w - 2) * (h - 2) // 2 and np.count_nonzero(want["n"][0]) >= 2


# ------------------------------------------------------------------------------------------------------------ commands
def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "grav1synth_amd", *args], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT,
                          stdin=subprocess.DEVNULL)


def _still_frame(k, w, h, bd):
    """4:2:0: two intensities side by side that stand still, the brighter one with three times the grain -- 3 x 3 box-filtered
    grain, fresh every frame."""
    rng = np.random.default_rng([13, k])
    up = 1 << (bd - 8)
    out = []
    for ph, pw in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
        xs = np.arange(pw)[None, :]
        base = np.where(xs < pw // 2, 60 * up, 170 * up) + np.zeros((ph, 1), np.int64)
        sg = np.where(xs < pw // 2, 1.0 * up, 3.0 * up)
        g = rng.standard_normal((ph + 2, pw + 2))
        g = sum(g[i:i + ph, j:j + pw] for i in range(3) for j in range(3)) / 3.0
        out.append(np.clip(np.rint(base + g * sg), 0, (1 << bd) - 1).astype(np.uint16))
    return out


@pytest.fixture(scope="module")
def still_clip(tmp_path_factory):
    """A 96 x 64 10-bit 4:2:0 clip of 5 frames as a file; its reference records; and the clip that Denoiser(curve=
    noise_prior(reference temporal record), strength=reference h) makes of it, as a file."""
    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.estimate import NLF_TRECORD, noise_prior
    from grav1synth_amd.ingest import write_y4m

    bd, w, h, n, nmin = 10, 96, 64, 5, 256
    d = tmp_path_factory.mktemp("auto_t")
    frames = [_still_frame(k, w, h, bd) for k in range(n)]
    src, den = d / "src.y4m", d / "den.y4m"
    write_y4m(str(src), frames, bd, 1, 1, Fraction(24, 1))
    ttotal = T.sum_records(T.run_records(frames, bd, 1, 1))
    total = R.sum_records([R.nlf_frame(f, bd, 1, 1) for f in frames])
    fwd, inv = noise_prior(T.to_struct(ttotal, NLF_TRECORD), bd, min_count=nmin, temporal=True)
    assert np.array_equal(fwd, R.curve_from_s(T.sigma(ttotal, bd, nmin), bd)[0])
    hl, hc = T.strength(ttotal, bd, nmin, 0), T.strength(ttotal, bd, nmin, 1)
    assert hl > 1.5 * R.strength(total, bd, nmin, 0), "on correlated grain the temporal strength is well above the Laplacian's"
    dn = Denoiser(bd, curve=(fwd, inv), strength=hl, chroma_strength=hc)
    write_y4m(str(den), [[np.asarray(p) for p in dn.apply(f, 1, 1)] for f in frames], bd, 1, 1, Fraction(24, 1))
    dn.close()
    return dict(src=src, den=den, dir=d, nmin=nmin, n=n, frames=frames, total=total, ttotal=ttotal, bd=bd)


def test_estimate_levels_temporal_command_and_the_file_call(still_clip):
    from grav1synth_amd.estimate import noise_levels_y4m_file

    d, frames, bd, n = still_clip["dir"], still_clip["frames"], still_clip["bd"], still_clip["n"]
    src, out, lev, tlev = still_clip["src"], d / "est.txt", d / "levels.txt", d / "tlevels.txt"
    later = R.sum_records([R.nlf_frame(f, bd, 1, 1) for f in frames[1:]])
    want_t = T.format_noise_levels_temporal(still_clip["ttotal"], n - 1, bd, 3, 0, later)
    want = R.format_noise_levels(still_clip["total"], n, bd, 3)
    p = _run("estimate", str(src), "-o", str(out), "--levels", str(lev), "--levels-temporal", str(tlev))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Done, wrote noise levels to {lev}" in p.stderr and f"Done, wrote temporal noise levels to {tlev}" in p.stderr
    assert tlev.read_bytes() == want_t and lev.read_bytes() == want
    ratio = float(want_t.split(b"ratio ")[1].split()[0])
    assert ratio > 2.0, "3 x 3 box-filtered grain"
    # alone, and without it the command writes what it wrote
    out2, tlev2 = d / "est2.txt", d / "tlevels2.txt"
    p = _run("estimate", str(src), "-o", str(out2), "--levels-temporal", str(tlev2))
    assert p.returncode == 0 and tlev2.read_bytes() == want_t and out2.read_bytes() == out.read_bytes() and "Done, wrote noise levels" not in p.stderr
    # the library's own loop over the file: the same records, the same reports; a prefix of the clip; one frame
    lev3, tlev3 = d / "levels3.txt", d / "tlevels3.txt"
    got_n, got, tgot = noise_levels_y4m_file(str(src), str(lev3), batch_frames=2, temporal_report=str(tlev3))
    assert got_n == n and not R.mismatches(got, still_clip["total"], "file") and not T.mismatches(tgot, still_clip["ttotal"], "file")
    assert lev3.read_bytes() == want and tlev3.read_bytes() == want_t
    got_n, got, tgot = noise_levels_y4m_file(str(src), None, max_frames=3, temporal_report=True)
    assert got_n == 3 and not T.mismatches(tgot, T.sum_records(T.run_records(frames[:3], bd, 1, 1)), "prefix")
    got_n, got, tgot = noise_levels_y4m_file(str(src), None, max_frames=1, temporal_report=str(tlev3))
    assert got_n == 1 and not tgot["n"].any() and tlev3.read_bytes() == T.format_noise_levels_temporal(T.empty_record(), 0, bd, 3, 0, R.empty_record())


def test_denoise_with_auto_temporal_is_the_denoiser_with_the_reference_curve_and_strength(still_clip):
    out = still_clip["dir"] / "auto.y4m"
    p = _run("denoise", str(still_clip["src"]), "-o", str(out), "--auto-prior", "--auto-strength", "--auto-temporal", "--levels-min-count",
             str(still_clip["nmin"]))
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"Denoised {still_clip['n']} frames" in p.stderr
    assert out.read_bytes() == still_clip["den"].read_bytes()
    plain = still_clip["dir"] / "plain.y4m"
    p = _run("denoise", str(still_clip["src"]), "-o", str(plain), "--auto-prior", "--auto-strength", "--levels-min-count", str(still_clip["nmin"]))
    assert p.returncode == 0 and plain.read_bytes() != out.read_bytes(), "the temporal job is not the Laplacian one"


def test_diff_with_auto_temporal_closes_the_loop(still_clip):
    d = still_clip["dir"]
    auto_tbl, ref_tbl, kept = d / "auto.tbl", d / "ref.tbl", d / "kept.y4m"
    p = _run("diff", str(still_clip["src"]), "--denoise", "-o", str(auto_tbl), "--keep-denoised", str(kept), "--auto-prior", "--auto-strength",
             "--auto-temporal", "--levels-min-count", str(still_clip["nmin"]))
    assert p.returncode == 0, p.stderr[-2000:]
    assert kept.read_bytes() == still_clip["den"].read_bytes()
    p = _run("diff", str(still_clip["src"]), str(still_clip["den"]), "-o", str(ref_tbl))
    assert p.returncode == 0, p.stderr[-2000:]
    assert auto_tbl.read_bytes() == ref_tbl.read_bytes() and auto_tbl.read_bytes().startswith(b"filmgrn1")


def test_the_rungs_with_zero_are_the_rungs_below_and_one_frame_is_refused(still_clip):
    from grav1synth_amd.denoise import denoise_opts
    from grav1synth_amd.ingest import write_y4m

    L = _lib.lib()
    d = still_clip["dir"]
    src = str(still_clip["src"]).encode()
    err = C.create_string_buffer(512)
    opts = denoise_opts()
    a, b = d / "below.y4m", d / "zero.y4m"
    args = (C.byref(opts), 0, 0, None, 0, -1, 0, 3, 0, still_clip["nmin"], 0, 0, 0.0)
    assert L.g1s_denoise_y4m_file_levels(src, str(a).encode(), *args, err, len(err)) == still_clip["n"], err.value
    assert L.g1s_denoise_y4m_file_auto_temporal(src, str(b).encode(), *args, 0, err, len(err)) == still_clip["n"], err.value
    assert a.read_bytes() == b.read_bytes()
    g = _lib.G1SOpts(C.sizeof(_lib.G1SOpts), -1, 3, 0, 0, 0)
    frames = C.c_uint64()
    ta, tb = d / "below.tbl", d / "zero.tbl"
    assert L.g1s_diff_y4m_file_denoised_levels(src, str(ta).encode(), None, C.byref(g), *args, C.byref(frames), err, len(err)) == 0, err.value
    assert L.g1s_diff_y4m_file_denoised_auto_temporal(src, str(tb).encode(), None, C.byref(g), *args, 0, C.byref(frames), err, len(err)) == 0, err.value
    assert ta.read_bytes() == tb.read_bytes() and frames.value == still_clip["n"]
    # a pre-pass of one frame: a clip of one, or a profile of one
    one = d / "one.y4m"
    write_y4m(str(one), still_clip["frames"][:1], still_clip["bd"], 1, 1, Fraction(24, 1))
    out = d / "never.y4m"
    for source, profile in ((str(one).encode(), 0), (src, 1)):
        args1 = (C.byref(opts), 0, 0, None, 0, -1, 0, 2, profile, still_clip["nmin"], 0, 0, 0.0)
        assert L.g1s_denoise_y4m_file_auto_temporal(source, str(out).encode(), *args1, 1, err, len(err)) == -1
        assert err.value.decode() == "temporal noise levels need two frames"
        assert L.g1s_diff_y4m_file_denoised_auto_temporal(source, str(out).encode(), None, C.byref(g), *args1, 1, C.byref(frames), err, len(err)) == -1
        assert err.value.decode() == "temporal noise levels need two frames"
    assert not out.exists()
