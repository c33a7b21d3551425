"""The flat-block finder's strip kernel (k1_moments_strips, csrc/k1f.hip.h): aligned luma rows of whole blocks have their
moments formed by a pass over column strips whose workgroups certify their own blocks; everything else keeps the row-per-lane
kernel and k1_certify, and G1S_K1_ROWS=1 forces that pair.  G1S_K1_KEEP_MB=0 puts the non-temporal hint on every frame's loads.

Through the public API, on tests/content.py (texture, ramps, damage: the certificate leaves blocks open), as device views
with a pitch above the row and a non-zero 16-byte-aligned base, in ONE batch of three different frames (frame-major
indexing).  Per case: every block's mask byte, f32 score bits and luma_sum against the oracle (luma_sum also against the
plane itself for the blocks the oracle does not measure), the whole record against the oracle's shadows, and the records'
bytes against the same job under G1S_K1_ROWS=1.

A wave covers STRIP luma samples of one block row, a workgroup four such tiles in raster order (16 blocks a wave); the
geometries are the smallest at which a part of that can go wrong."""
from __future__ import annotations

import numpy as np
import pytest

from tests.content import make_frames
from tests.helpers import record_mismatches
from tests.oracle_binding import OracleDiff
from tests.test_gpu_records import FPS, Geom, _generator, _job
from tests.test_gpu_views import At, _place_job

pytestmark = pytest.mark.gpu

STRIP = 512  # luma samples across a wave's tile
KINDS = ("distinct", "damaged", "busy")

GEOMS = {
    "one_block": (32, 32),                                 # a nearly empty strip, three idle waves
    "one_strip": (STRIP, 32),                              # a full strip
    "strip_and_a_block": (STRIP + 32, 64),                 # a full strip beside a one-block strip: four tiles, one workgroup
    "ragged_bottom": (2 * STRIP + 32, 136),                # 4.25 block rows: replication, CLIP; 15 tiles: a last workgroup short of a wave
    "1080p_last_rows": (1920, 1080 - 29 * 32),             # the last five block rows of 1920 x 1080 (4.75): the real ragged bottom
}


def _plan(i):
    """A pitch above the row and a non-zero base on a 16-byte boundary, both different from frame to frame."""
    return ([At(("+", 16 * (1 + i)), 16 * (1 + i + c)) for c in range(3)], [At(("+", 32), 16 * (3 + c)) for c in range(3)])


def _luma_sums(plane: np.ndarray, bd: int) -> np.ndarray:
    """get_block_mean's exact sum: the 8-bit samples of every 32 x 32 block that lie inside the plane."""
    p = (plane.astype(np.int64) >> (bd - 8))
    h, w = p.shape
    nbh, nbw = (h + 31) // 32, (w + 31) // 32
    q = np.zeros((nbh * 32, nbw * 32), np.int64)
    q[:h, :w] = p
    return q.reshape(nbh, 32, nbw, 32).sum(axis=(1, 3)).ravel()


def _run(geom: Geom, pairs, timed: bool):
    """(records [n, size], kernel names, literal blocks) of the job as one batch."""
    g = _generator(geom, len(pairs), records_only=True)
    try:
        if timed:
            g.set_timing(True)
        for s, d in pairs:
            g.diff_frame(s, d)
        if timed:
            g.sync()
            return None, set(g.kernel_times()), g.stats().literal_blocks
        recs, n = g.take_records(geom.w, geom.h, 3 if geom.chroma else 1, len(pairs))
        assert n == len(pairs)
        return recs, None, None
    finally:
        g.close()


def _frames_and_shadows(geom: Geom):
    """The job's frames and the oracle's shadows of every frame.  A frame of one block is refused by the oracle's model update
    ("Not enough flat blocks"), which runs BEHIND its finder: the shadow of such a frame is the finder's alone (mask, scores)."""
    try:
        frames, shadows, _ = _job(geom, KINDS)
        return frames, shadows
    except RuntimeError as e:
        if "Not enough flat blocks" not in str(e):
            raise
    frames, shadows = [], []
    for k, kind in enumerate(KINDS):
        s, d = make_frames(kind, geom.w, geom.h, geom.src_bd, geom.xd, geom.yd, k)
        if not geom.chroma:
            s, d = s[:1], d[:1]
        o = OracleDiff(FPS.numerator, FPS.denominator, geom.src_bd, geom.den_bd, geom.lag, geom.chroma)
        with pytest.raises(RuntimeError, match="Not enough flat blocks"):
            o.diff_frame(s, d, geom.xd, geom.yd)
        frames.append((s, d))
        shadows.append(dict(mask=o.flat_mask(), scores=o.scores()))
    return frames, shadows


def _finder_mismatches(shadow: dict, r, where: str):
    out = []
    if not np.array_equal(shadow["mask"], r.flat_mask()):
        out.append(f"{where}: flat mask differs at {np.argwhere(shadow['mask'] != r.flat_mask())[:5].tolist()}")
    if not np.array_equal(shadow["scores"].view(np.uint32), r.scores().view(np.uint32)):
        out.append(f"{where}: score bits differ")
    return out


def _check(monkeypatch, geom: Geom, plan, strips_expected: bool):
    from grav1synth_amd.diff import Record

    frames, shadows = _frames_and_shadows(geom)
    placed = _place_job(geom, frames, plan)
    monkeypatch.delenv("G1S_K1_ROWS", raising=False)
    monkeypatch.delenv("G1S_K1_KEEP_MB", raising=False)
    _, names, literal = _run(geom, placed.pairs, timed=True)
    ran_strips = any(n.startswith("k1_moments_strips") for n in names)
    assert ran_strips == strips_expected, sorted(names)
    assert ("k1_certify" in names) == (not strips_expected), sorted(names)
    recs, _, _ = _run(geom, placed.pairs, timed=False)
    bad = []
    for i in range(len(frames)):
        r = Record(recs[i])
        where = f"frame {i} ({KINDS[i]})"
        # mask bytes, score bits of every block; where the oracle went on to measure, its luma_sum and the sums behind them
        bad.extend(record_mismatches(shadows[i], r, where) if "ar" in shadows[i] else _finder_mismatches(shadows[i], r, where))
        ls = r.block_stats(0)[0]
        want = _luma_sums(frames[i][0][0], geom.src_bd)
        if not np.array_equal(ls, want):
            bad.append(f"{where}: luma_sum differs from the plane's block sums at blocks {np.flatnonzero(ls != want)[:8].tolist()}")
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:40])
    # the same job with the non-temporal hint on every frame's loads (by default only on frames the last-level cache will not keep:
    # none of a batch this small)
    monkeypatch.setenv("G1S_K1_KEEP_MB", "0")
    recs_nt, _, _ = _run(geom, placed.pairs, timed=False)
    monkeypatch.delenv("G1S_K1_KEEP_MB")
    assert np.array_equal(recs, recs_nt), "the records differ with the non-temporal hint on every frame"
    monkeypatch.setenv("G1S_K1_ROWS", "1")
    _, names_rows, literal_rows = _run(geom, placed.pairs, timed=True)
    assert "k1_certify" in names_rows and not any(n.startswith("k1_moments_strips") for n in names_rows), sorted(names_rows)
    recs_rows, _, _ = _run(geom, placed.pairs, timed=False)
    monkeypatch.delenv("G1S_K1_ROWS")
    for i in range(len(frames)):
        assert np.array_equal(recs[i], recs_rows[i]), f"frame {i}: the record differs from the row kernels' at bytes {np.flatnonzero(recs[i] != recs_rows[i])[:8].tolist()}"
    # (the comparison is live: another frame's record is not this one's)
    assert not np.array_equal(recs[0], recs_rows[1]) and not np.array_equal(recs[2], recs_rows[1])
    print(f"{geom.w}x{geom.h} {geom.src_bd}-bit: {literal} literal blocks (row kernels: {literal_rows})")
    assert literal == literal_rows
    for what, guard in placed.guards:
        guard.assert_unchanged(what)
    return literal


@pytest.mark.parametrize("chroma", [True, False], ids=["420", "luma_only"])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", list(GEOMS))
def test_strip_finder_gives_the_oracles_blocks_and_the_row_kernels_records(monkeypatch, name, bd, chroma):
    w, h = GEOMS[name]
    literal = _check(monkeypatch, Geom(w, h, bd, bd, 1, 1, 3, chroma), _plan, strips_expected=True)
    if name == "1080p_last_rows":
        assert literal > 0, "the certificate left no block to the literal kernel: the list path did not run"


@pytest.mark.parametrize("bd", [8, 10])
def test_a_ragged_last_block_column_keeps_the_row_kernels(monkeypatch, bd):
    """W % 32 != 0 on aligned rows: the fallback pair, against the oracle."""
    _check(monkeypatch, Geom(STRIP + 48, 72, bd, bd, 1, 1, 3), _plan, strips_expected=False)


@pytest.mark.parametrize("bd", [8, 10])
def test_an_unaligned_luma_base_keeps_the_row_kernels(monkeypatch, bd):
    """The source luma of the second frame 2 bytes off a 16-byte boundary: fast_rows drops for the batch."""
    def plan(i):
        s, d = _plan(i)
        if i == 1:
            s[0] = At(("+", 16), 2)
        return s, d

    _check(monkeypatch, Geom(STRIP + 32, 64, bd, bd, 1, 1, 3), plan, strips_expected=False)
