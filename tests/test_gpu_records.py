"""Whole jobs on plane-distinct content (tests/content.py): EVERY frame's record against the oracle's integers for that
frame -- mask bytes, f32 score bits, S, Sb and nobs of every plane, luma_sum, sum_d and sum_d2 on the blocks the oracle
measured -- wherever the frame sat: inside a batch, in a slot that earlier batches of another kind of content had used, in
the short last batch of a job, in a slot another generator had parked.  Then the table paths (the host and the device half
of the per-frame fold, the shard merge, the reader and `apply`'s lookup) on a table whose three planes differ.

The oracle runs once per geometry and its per-frame shadows are kept, so the batch shapes of a case share it.

Which chain of kernels serves a geometry is the engine's choice (g1s_diff::wide_ok); the cases that are there for a chain
say which one they mean, and test_geometry_runs_the_chain_its_cases_mean holds the engine to it."""
import functools
import os
import subprocess
import sys
from fractions import Fraction
from typing import NamedTuple

import numpy as np
import pytest

from tests.content import make_frames
from tests.helpers import oracle_shadow, record_mismatches
from tests.oracle_binding import OracleDiff, format_tbl as oracle_tbl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = Fraction(24, 1)
SLOTS = 6  # engine.hip kSlots: batch j of a generator runs in slot j % 6


class Geom(NamedTuple):
    w: int
    h: int
    src_bd: int
    den_bd: int
    xd: int
    yd: int
    lag: int
    chroma: bool = True


@functools.lru_cache(maxsize=None)
def _job(geom: Geom, kinds: tuple):
    """Frames 0, 1, ... of the given kinds (host planes), the oracle's shadows of every frame, and its table."""
    o = OracleDiff(FPS.numerator, FPS.denominator, geom.src_bd, geom.den_bd, geom.lag, geom.chroma)
    frames, shadows = [], []
    for k, kind in enumerate(kinds):
        s = make_frames(kind, geom.w, geom.h, geom.src_bd, geom.xd, geom.yd, k)[0]
        d = make_frames(kind, geom.w, geom.h, geom.den_bd, geom.xd, geom.yd, k)[1]
        if not geom.chroma:
            s, d = s[:1], d[:1]
        o.diff_frame(s, d, geom.xd, geom.yd)
        frames.append((s, d))
        shadows.append(oracle_shadow(o, len(s)))
    return frames, shadows, oracle_tbl(o.finish())


def _generator(geom: Geom, batch: int, records_only=False):
    from grav1synth_amd.diff import DiffGenerator

    return DiffGenerator(FPS, geom.src_bd, geom.den_bd, ar_coeff_lag=geom.lag, luma_only=not geom.chroma, batch_frames=batch,
                         records_only=records_only)


def _feed(g, geom: Geom, frames):
    import torch

    from grav1synth_amd.diff import Frame

    for s, d in frames:
        g.diff_frame(Frame([torch.from_numpy(p).cuda() for p in s], geom.xd, geom.yd),
                     Frame([torch.from_numpy(p).cuda() for p in d], geom.xd, geom.yd))


def _job_mismatches(g, geom: Geom, frames, shadows, kinds, batch: int):
    """Feed the frames to `g` (a records_only generator), take the records once at the end, compare every one."""
    from grav1synth_amd.diff import Record

    _feed(g, geom, frames)
    recs, n = g.take_records(geom.w, geom.h, 3 if geom.chroma else 1, len(frames))
    if n != len(frames):
        return [f"{n} records for {len(frames)} frames"]
    out = []
    for i in range(n):
        j = i // batch
        where = f"frame {i} ({kinds[i]}; batch {j}, position {i % batch}, slot {j % SLOTS})"
        out.extend(record_mismatches(shadows[i], Record(recs[i]), where))
    return out


def _check_job(geom: Geom, kinds, batch: int):
    frames, shadows, _ = _job(geom, tuple(kinds))
    g = _generator(geom, batch, records_only=True)
    try:
        bad = _job_mismatches(g, geom, frames, shadows, kinds, batch)
    finally:
        g.close()
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:40])


# ---- which chain --------------------------------------------------------------------------------------------------------

WIDE_8 = Geom(320, 192, 8, 8, 1, 1, 3)     # rows of whole 16-byte words in every plane: the wide chain
STREAM_8 = Geom(326, 198, 8, 8, 1, 1, 2)   # nothing a multiple of 8: the stream chain
JOB_GEOMS = {
    "8b420_320x192_lag3_wide": (WIDE_8, "wide"),
    "8b420_326x198_lag2_stream": (STREAM_8, "stream"),
    "10b422_320x200_lag1": (Geom(320, 200, 10, 10, 1, 0, 1), "wide"),      # the bottom block row cut (6.25 blocks)
    "10b444_256x160_lag3": (Geom(256, 160, 10, 10, 0, 0, 3), "wide"),
    "12b420_320x192_lag2": (Geom(320, 192, 12, 12, 1, 1, 2), "wide"),
    "8b_luma_only_352x208_lag3": (Geom(352, 208, 8, 8, 1, 1, 3, False), "wide"),
}
MIXED_GEOMS = {
    # the wide chain's general residual (engine.hip wide_gen: 4:2:0 and luma-only) ...
    "10_8_420": (Geom(352, 208, 10, 8, 1, 1, 3), "wide"),
    "8_10_420": (Geom(352, 208, 8, 10, 1, 1, 3), "wide"),
    "12_10_420": (Geom(320, 200, 12, 10, 1, 1, 2), "wide"),
    "10_8_luma_only": (Geom(320, 192, 10, 8, 1, 1, 3, False), "wide"),
    "12_10_luma_only": (Geom(384, 192, 12, 10, 1, 1, 3, False), "wide"),
    # ... and the other subsamplings of such a pair: the stream chain
    "10_8_422": (Geom(320, 192, 10, 8, 1, 0, 3), "stream"),
    "10_8_444": (Geom(256, 160, 10, 8, 0, 0, 3), "stream"),
}
CHAIN_KERNEL = {"wide": "k3w_pass", "stream": "k3s_fused"}


@pytest.mark.parametrize("name", list(JOB_GEOMS) + list(MIXED_GEOMS))
def test_geometry_runs_the_chain_its_cases_mean(name):
    """The accumulation kernel a short timed generator of the geometry launches (kernel_times): k3w_pass is the wide chain,
    k3s_fused the stream chain.  A change of the rule that moves a case to the other chain shows here."""
    geom, chain = (JOB_GEOMS.get(name) or MIXED_GEOMS[name])
    frames, _, _ = _job(geom, ("flat", "flat"))
    g = _generator(geom, 2, records_only=True)
    try:
        g.set_timing(True)
        _feed(g, geom, frames)
        g.sync()
        names = set(g.kernel_times())
    finally:
        g.close()
    ran = {c for c, k in CHAIN_KERNEL.items() if any(n.startswith(k) for n in names)}
    assert ran == {chain}, f"{name}: kernels {sorted(names)}"


# ---- 1. slot reuse inside a generator --------------------------------------------------------------------------------------

# the kind of every pair of frames: 15 batches of two (29 frames: the last batch holds one).  By slot (batch mod 6):
#   0: damaged -> flat -> busy        1: busy -> damaged -> distinct     2: flat -> damaged -> flat (the short batch, behind
#   3: distinct -> busy               4: damaged -> flat                    two damaged frames)      5: clamped -> busy
# With 3 and 5 frames a batch (last batches of 2 and 4) the kinds change inside batches, and other kinds meet in a slot.
SCHEDULE = ["damaged", "busy", "flat", "distinct", "damaged", "clamped", "flat", "damaged", "damaged", "busy", "flat", "busy",
            "busy", "distinct", "flat"]
JOB_KINDS = tuple(k for k in SCHEDULE for _ in range(2))[:29]


@pytest.mark.parametrize("batch", [2, 3, 5])
@pytest.mark.parametrize("name", list(JOB_GEOMS))
def test_every_record_of_a_job_that_uses_every_slot_twice(name, batch):
    assert (len(JOB_KINDS) + 1) // 2 >= 2 * SLOTS + 1 and len(JOB_KINDS) % batch, "every slot twice with two frames a batch, a short last batch"
    _check_job(JOB_GEOMS[name][0], JOB_KINDS, batch)


# ---- 2. slot reuse across generators ----------------------------------------------------------------------------------------

def _cross_generator_child():
    """Runs in a fresh interpreter (the slot cache is process-wide, holds eight slots and never evicts: only there is it
    known to be empty).  Per geometry: a generator runs six full batches of one kind -- every slot used -- and is closed: its six
    slots park.  The next generator has the same geometry, depths, lag and batch size, so the cache key matches and it is handed
    those slots (there is no counter to show it: it follows from the key and the empty cache); it runs a shorter job of the
    other kind whose last batch is short.  Then the kinds the other way round, through the same slots.  The last generator of
    the first geometry stays open until the end, so that the second geometry meets an empty cache too."""
    bad, held = [], []
    for geom in (WIDE_8, STREAM_8):
        for first, second in (("damaged", "distinct"), ("distinct", "damaged")):
            for kind, nframes in ((first, 12), (second, 7)):
                kinds = (kind,) * 12
                frames, shadows, _ = _job(geom, kinds)
                g = _generator(geom, 2, records_only=True)
                got = _job_mismatches(g, geom, frames[:nframes], shadows[:nframes], kinds, 2)
                bad += [f"{geom.w}x{geom.h} {first} then {second}, the {kind} job of {nframes}: {m}" for m in got]
                if (first, kind) == ("distinct", "damaged"):
                    held.append(g)
                else:
                    g.close()
                print(f"{geom.w}x{geom.h} {kind} x {nframes}: {len(got)} fields differ", flush=True)
    for g in held:
        g.close()
    print("\n".join(bad[:40]))
    print("RECORDS EQUAL" if not bad else f"MISMATCH {len(bad)}")


def test_every_record_of_a_generator_that_is_handed_parked_slots():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", "from tests.test_gpu_records import _cross_generator_child as f; f()"], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.strip().splitlines()[-1] == "RECORDS EQUAL", p.stdout[-6000:]


# ---- 3. mixed depths ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MIXED_GEOMS))
def test_every_record_of_a_mixed_depth_job(name):
    _check_job(MIXED_GEOMS[name][0], ("distinct",) * 8, 3)


# ---- 4. tuning switches read per call -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("reuse,f_wgs,w_wgs", [("1", "64", "24"), ("0", "64", "264"), ("1", "8", "8")])
@pytest.mark.parametrize("name", ["8b420_320x192_lag3_wide", "8b420_326x198_lag2_stream"])
def test_every_record_with_other_launch_shapes(monkeypatch, name, reuse, f_wgs, w_wgs):
    """Few workgroups a frame and many (G1S_W_WGS[_C]: the wide chain, G1S_F_WGS / G1S_F_REUSE: the stream chain), read when
    the generator sizes its slots and at every launch."""
    monkeypatch.setenv("G1S_F_REUSE", reuse)
    monkeypatch.setenv("G1S_F_WGS", f_wgs)
    monkeypatch.setenv("G1S_W_WGS", w_wgs)
    monkeypatch.setenv("G1S_W_WGS_C", w_wgs)
    _check_job(JOB_GEOMS[name][0], JOB_KINDS, 3)


# ---- 5. the table paths ---------------------------------------------------------------------------------------------------------

TABLE_GEOM = Geom(352, 208, 10, 10, 1, 1, 3)
TABLE_KINDS = ("distinct",) * 4 + ("busy",) * 3 + ("flat",) * 2 + ("distinct",) * 2


def _planes_differ(tbl: bytes):
    from grav1synth_amd.tbl import parse_tbl

    segs = parse_tbl(tbl)
    assert all(s.scaling_points_cb != s.scaling_points_cr and s.ar_coeffs_cb != s.ar_coeffs_cr for s in segs)
    return segs


@pytest.mark.parametrize("where", ["host", "device"])
def test_folding_generator_gives_the_oracles_table(monkeypatch, where):
    from grav1synth_amd.diff import format_tbl

    monkeypatch.setenv("G1S_LATEST", where)
    frames, _, want = _job(TABLE_GEOM, TABLE_KINDS)
    _planes_differ(want)
    g = _generator(TABLE_GEOM, 3)
    g.set_timing(True)
    _feed(g, TABLE_GEOM, frames)
    got = format_tbl(g.finish())
    on_device = "k4_latest" in g.kernel_times()
    g.close()
    assert got == want
    assert on_device == (where == "device")


def _latest_blobs(geom, frames, batch):
    g = _generator(geom, batch, records_only=2)
    _feed(g, geom, frames)
    out = g.take_latest(len(frames) + 8, sync=True).copy()
    g.close()
    return out


@pytest.mark.parametrize("kind", ["distinct", "clamped", "busy"])
def test_device_half_gives_the_host_halfs_blobs_and_the_oracles_table(monkeypatch, kind):
    """records_only = 2: the latest states of the device half equal the host half's byte for byte, and merged in order
    (RecordFold.push_latest_many) they give the oracle's table."""
    from grav1synth_amd.diff import RecordFold, format_tbl

    geom = Geom(1056, 560, 8, 8, 1, 1, 3)  # 594 blocks: the strength pass's chunk of 512 and a short one
    frames, _, want = _job(geom, (kind,) * 3)
    blobs = {}
    for where in ("host", "device"):
        monkeypatch.setenv("G1S_LATEST", where)
        blobs[where] = _latest_blobs(geom, frames, 2)
    assert blobs["host"].shape == blobs["device"].shape and blobs["host"].shape[0] == len(frames)
    for i in range(len(frames)):
        diff = np.flatnonzero(blobs["host"][i] != blobs["device"][i])
        assert diff.size == 0, f"frame {i}: {diff.size} bytes differ, first at {diff[0]} (of {blobs['host'].shape[1]})"
    fold = RecordFold(FPS, geom.lag)
    fold.push_latest_many(blobs["device"])
    assert format_tbl(fold.finish()) == want


def test_unset_switch_at_4096_blocks_runs_the_device_half_and_gives_the_oracles_table(monkeypatch):
    """2048 x 2048: the engine's own choice of the device half (k4_latest in the timed kernels), three frames."""
    from grav1synth_amd.diff import format_tbl

    monkeypatch.delenv("G1S_LATEST", raising=False)
    geom = Geom(2048, 2048, 8, 8, 1, 1, 3)
    frames, _, want = _job(geom, ("distinct",) * 3)
    _planes_differ(want)
    g = _generator(geom, 2)
    g.set_timing(True)
    _feed(g, geom, frames)
    got = format_tbl(g.finish())
    names = set(g.kernel_times())
    g.close()
    assert "k4_latest" in names, sorted(names)
    assert got == want


def test_three_generators_share_a_job_whose_content_changes_kind(tmp_path):
    """g1s_diff_y4m_files_sharded on devices [0, 0, 0], batches of two: the shard merge on a table whose planes differ."""
    from grav1synth_amd.ingest import diff_y4m_files, write_y4m

    frames, _, want = _job(TABLE_GEOM, TABLE_KINDS)
    write_y4m(str(tmp_path / "src.y4m"), [s for s, _ in frames], 10, 1, 1, FPS)
    write_y4m(str(tmp_path / "den.y4m"), [d for _, d in frames], 10, 1, 1, FPS)
    out = tmp_path / "out.tbl"
    n, unequal = diff_y4m_files(str(tmp_path / "src.y4m"), str(tmp_path / "den.y4m"), str(out), batch_frames=2, devices=[0, 0, 0])
    assert (n, unequal) == (len(frames), False)
    assert out.read_bytes() == want


def test_table_from_the_kernels_drives_the_apply_lookup_with_its_own_cb_and_cr():
    """test_hip_table_drives_the_apply_lookup's walk on a two-segment table whose Cb and Cr differ: what the lookup hands back
    for a frame is that segment's Cb under Cb and its Cr under Cr."""
    from grav1synth_amd.diff import format_tbl
    from grav1synth_amd.tbl import GrainTable, parse_tbl_native

    geom = WIDE_8
    kinds = ("distinct",) * 3 + ("damaged",) * 3
    frames, _, want = _job(geom, kinds)
    g = _generator(geom, 4)
    _feed(g, geom, frames)
    out = g.finish()
    g.close()
    text = format_tbl(out)
    assert text == want
    segs = parse_tbl_native(text)
    assert len(segs) >= 2 and segs == _planes_differ(text)
    table = GrainTable(segs)
    for k in range(len(frames)):
        ts = (k * 10_000_000 * FPS.denominator) // FPS.numerator
        i = next(i for i, x in enumerate(segs) if x.start_time <= ts < x.end_time)
        seg = table.segment_for(ts)
        assert seg is not None and seg.start_time == segs[i].start_time
        assert (seg.scaling_points_cb, seg.ar_coeffs_cb) == (out[i].scaling_points_cb, out[i].ar_coeffs_cb), f"frame {k}: Cb"
        assert (seg.scaling_points_cr, seg.ar_coeffs_cr) == (out[i].scaling_points_cr, out[i].ar_coeffs_cr), f"frame {k}: Cr"
        assert (seg.scaling_points_y, seg.ar_coeffs_y) == (out[i].scaling_points_y, out[i].ar_coeffs_y), f"frame {k}: Y"
