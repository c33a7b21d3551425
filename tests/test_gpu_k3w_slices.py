"""The ends of a k3w_pass workgroup's slice, on frames of a handful of units: every frame's record against the oracle's integers
with slices of 1, 2, 3 and 4 units, with and without a flat neighbour in front of the slice (the ghost the workgroup forms from
the entry before its first) and behind it, slices that hold no unit at all, and a residual outside int8 in the last unit of a
slice of odd length (the unit is deferred after its neighbours were staged beside it).

Frames of 256 x 64, 384 x 96 and 640 x 96 (2 x 2, 3 x 3 and 5 x 3 luma units; 1, 2 and 3 chroma units a block row) in 10-bit
4:2:0, 8-bit 4:2:0 and 10-bit luma only, four frames a job: every block flat, whole units flat in a chessboard (a list neighbour that
is no spatial neighbour), every block flat with damage (tests/mask_content.py), every block textured.  G1S_W_WGS / G1S_W_WGS_C
of 1 .. 7 are workgroups a FRAME (engine.hip w_wgs_per_frame), so a frame's list of 4 .. 15 units is cut into slices of those
lengths.

A frame's list is never EMPTY: the finder's percentile rule flags the best tenth of a frame's blocks whatever they hold
(diff_oracle.c: score >= the score at the 90th percentile), so every frame has a flat block and both lists a unit.  What is run
in its place: workgroups whose SLICE is empty (more workgroups than units), and the all-textured frame.

Compared per frame, exactly, as tests/test_gpu_mask_patterns.py does (its helpers: record_mismatches, the generator and the
feed of tests/test_gpu_records.py).  What the oracle's masks of these jobs give -- every slice shape named above, by plane kind
-- is asserted without a device in tests/test_k3w_slices_cpu.py; the oracle runs once per geometry and its shadows are shared
by the cases."""
import functools

import numpy as np
import pytest

from tests import mask_content as MC
from tests.helpers import oracle_shadow, record_mismatches
from tests.oracle_binding import OracleDiff
from tests.test_gpu_records import CHAIN_KERNEL, FPS, SLOTS, Geom, _feed, _generator

pytestmark = pytest.mark.gpu

BATCH = 3  # four frames: a full batch and a short one
SIZES = ((256, 64), (384, 96), (640, 96))
FORMATS = {"10b420": (10, 3, True), "8b420": (8, 2, True), "10b_luma_only": (10, 3, False)}
GEOMS = {f"{f}_{w}x{h}": Geom(w, h, bd, bd, 1, 1, lag, chroma) for f, (bd, lag, chroma) in FORMATS.items() for (w, h) in SIZES}
# workgroups a frame (G1S_W_WGS, G1S_W_WGS_C) by frame size: tests/test_k3w_slices_cpu.py holds what slices they cut
WGS = {
    (256, 64): (("1", "1"), ("4", "3")),
    (384, 96): (("2", "2"), ("4", "4"), ("5", "3")),
    (640, 96): (("4", "2"), ("5", "4"), ("7", "6")),
}
CASES = [(name, wl, wc) for name, g in GEOMS.items() for (wl, wc) in WGS[(g.w, g.h)]]
FRAMES = (("full", False), ("cells", False), ("full", True), ("none", False))  # (design, damage)


def designs(nbh: int, nbw: int):
    by, bx = np.arange(nbh)[:, None], np.arange(nbw)[None, :]
    out = {
        "full": (bx >= 0) & (by >= 0),
        "cells": ((bx >> 2) + by) % 2 == 0,  # whole luma units, every second one; half of every chroma unit
        "none": (bx < 0) & (by < 0),
    }
    return {k: np.ascontiguousarray(np.broadcast_to(v, (nbh, nbw)).astype(np.uint8)) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _job(geom: Geom):
    """The job's frames (host planes), the oracle's shadows of every frame."""
    o = OracleDiff(FPS.numerator, FPS.denominator, geom.src_bd, geom.den_bd, geom.lag, geom.chroma)
    ds = designs((geom.h + 31) // 32, (geom.w + 31) // 32)
    frames, shadows = [], []
    for k, (name, damage) in enumerate(FRAMES):
        s = MC.make_frames(ds[name], geom.w, geom.h, geom.src_bd, geom.xd, geom.yd, k, damage=damage)[0]
        d = MC.make_frames(ds[name], geom.w, geom.h, geom.den_bd, geom.xd, geom.yd, k, damage=damage)[1]
        if not geom.chroma:
            s, d = s[:1], d[:1]
        o.diff_frame(s, d, geom.xd, geom.yd)
        frames.append((s, d))
        shadows.append(oracle_shadow(o, len(s)))
    return frames, shadows


# ---- what k3w_pass makes of a mask (engine.hip w_wgs_per_frame, k3w.hip.h w_build_units and the kernel's own slice) -----------

def unit_list(flat: np.ndarray, ub: int):
    """[(block row, cell, flat left neighbour cell, flat right neighbour cell)] of the units of `ub` blocks with a flat block, in
    raster order: the list k2w_select_units writes."""
    nbh, nbw = flat.shape
    pad = np.zeros((nbh, -(-nbw // ub) * ub), bool)
    pad[:, :nbw] = flat
    cells = pad.reshape(nbh, -1, ub).any(axis=2)
    z = np.pad(cells, ((0, 0), (1, 1)))
    return [(int(by), int(c), bool(z[by, c]), bool(z[by, c + 2])) for by, c in np.argwhere(cells)]


def slices(units, wgs: int):
    """The slice of every workgroup of a frame: units [cnt wg / G, cnt (wg + 1) / G)."""
    cnt = len(units)
    return [units[cnt * wg // wgs:cnt * (wg + 1) // wgs] for wg in range(wgs)]


def slice_shapes(flat: np.ndarray, ub: int, wgs: int):
    """{(units, ghost in front, ghost behind)} over the frame's workgroups; (0, False, False): an empty slice."""
    out = set()
    for sl in slices(unit_list(flat, ub), wgs):
        out.add((len(sl), sl[0][2], sl[-1][3]) if sl else (0, False, False))
    return out


# ---- the device --------------------------------------------------------------------------------------------------------------

def _check(geom: Geom, monkeypatch, wgs_luma: str, wgs_chroma: str):
    from grav1synth_amd.diff import Record

    monkeypatch.setenv("G1S_W_WGS", wgs_luma)
    monkeypatch.setenv("G1S_W_WGS_C", wgs_chroma)
    frames, shadows = _job(geom)
    g = _generator(geom, BATCH, records_only=True)
    try:
        _feed(g, geom, frames)
        recs, n = g.take_records(geom.w, geom.h, 3 if geom.chroma else 1, len(frames))
        assert n == len(frames), f"{n} records for {len(frames)} frames"
        bad = []
        for i in range(n):
            j = i // BATCH
            where = f"frame {i} ({FRAMES[i][0]}{', damaged' if FRAMES[i][1] else ''}; batch {j}, position {i % BATCH}, slot {j % SLOTS})"
            bad.extend(record_mismatches(shadows[i], Record(recs[i]), where))
    finally:
        g.close()
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("name,wgs_luma,wgs_chroma", CASES)
def test_every_record_with_slices_of_a_few_units(monkeypatch, name, wgs_luma, wgs_chroma):
    _check(GEOMS[name], monkeypatch, wgs_luma, wgs_chroma)


@pytest.mark.parametrize("name", [n for n in GEOMS if n.endswith("640x96")])
def test_these_frames_run_the_wide_chain(monkeypatch, name):
    """k3w_pass is among the timed kernels of such a job, with workgroups a frame set as the cases set them."""
    geom = GEOMS[name]
    monkeypatch.setenv("G1S_W_WGS", "5")
    monkeypatch.setenv("G1S_W_WGS_C", "3")
    g = _generator(geom, 2, records_only=True)
    try:
        g.set_timing(True)
        _feed(g, geom, _job(geom)[0][:2])
        g.sync()
        names = set(g.kernel_times())
    finally:
        g.close()
    ran = {c for c, k in CHAIN_KERNEL.items() if any(n.startswith(k) for n in names)}
    assert ran == {"wide"}, f"{name}: kernels {sorted(names)}"
