"""k_estimate_pk at every strip height its launch can choose (`-m gpu`).

The packed estimator's row strips are 8 .. 256 rows high, chosen at every launch from the plane, the batch, the device's
compute units and the kernel's occupancy (csrc/estimate_plan.h; tests/test_estimate_plan_cpu.py).  At the small shapes of the
rest of the suite that choice is 8 rows, always; a production launch (1080p, 4K, 8K in batches of 32) runs 17 to 256.  The
height drives est_strip's three-rows-a-turn loop and its remainder of 0, 1 or 2 rows, the loads two rows ahead of their use
(past the strip, past the plane), the two 16-bit pixel counters of a lane and the 32-bit accum of a lane and of a wave.

Here G1S_ESTIMATE_ROWS pins the height and g1s_estimate_last_launch says what ran: every case first asserts that its launch
was the packed kernel at the height asked for.  What is compared is exact and is the integers: (accum, count) of every
frame against the oracle's (oracle/estimate_oracle.c), the f64 against the oracle's, and the packed run against the 32-bit
kernel (G1S_ESTIMATE=wide) on the same frames.  A ratio alone hides a wrong count on flat content (0.0), wrong sums on
all-edge content (None) and an error that scales both sums alike.

Heights: 8, 9, 10, 11 (full strips leave remainders of 2, 0, 1, 2), the production heights at 8 workgroups a CU (imported
from the CPU test's restatement of the plan, not written here) and, at two widths, at 1 .. 7 (an MI355X has answered 5), 85,
86, 254, 255, 256.  Planes for a height R: H - 2 in
{R - 1, R, 2R + 1, 2R + 2, 2R + 3, 3R} -- one short strip, one exact strip, a last strip of 1, 2, 3 rows under two full ones,
whole strips only; the tallest is 770 rows.  Widths: 504 (fast form, the second column strip 7 columns wide), 16 (fast, one
strip, most lanes idle), 498 (a second strip of one output column; slow form by width), 501 (slow by width), and 504 as a
device view with a pitch above the row and a base 6 bytes past a 16-byte boundary (slow by alignment; hostile margin).
Five frames a batch: uniform noise over the full range, the 0 / max checkerboard (the largest |Laplacian| everywhere: the
largest accum a lane and a wave can reach), a flat field (every pixel counts: the counters' bound), a field one step under
the edge threshold, all-edge content (None; its sums are zeros)."""
from __future__ import annotations

import numpy as np
import pytest

from tests.oracle_binding import estimate_plane_noise, estimate_plane_sums
from tests.test_estimate_plan_cpu import col_strips, plan_strips, production_heights

pytestmark = pytest.mark.gpu

FULL_CROSS = sorted({8, 9, 10, 256, *production_heights(8)})   # every width
# 504 and the view: the other heights asked for, and what the production launches run at 1 .. 7 workgroups a CU
THINNED = sorted({11, 85, 86, 254, 255, *(r for occ in range(1, 8) for r in production_heights(occ))} - set(FULL_CROSS))
WIDTHS = (504, 16, 498, 501, "view")
CASES = [(r, w) for r in FULL_CROSS for w in WIDTHS] + [(r, w) for r in THINNED for w in (504, "view")]
BATCH = 5


def plane_heights(r: int):
    return [rows + 2 for rows in ([r - 1] if r > 1 else []) + [r, 2 * r + 1, 2 * r + 2, 2 * r + 3, 3 * r]]


def frames_of(h: int, w: int, bd: int):
    """The five frames of a batch and what each must sum to where that has a closed form (None where it has not)."""
    rng = np.random.default_rng([h, w, bd])
    dt = np.uint8 if bd == 8 else np.uint16
    mx, sh = (1 << bd) - 1, bd - 8
    half = (1 << sh) >> 1
    ys, xs = np.indices((h, w))
    interior = (h - 2) * (w - 2)
    planes = [rng.integers(0, mx + 1, (h, w)).astype(dt),
              (((ys + xs) & 1) * mx).astype(dt),
              np.full((h, w), mx // 3, dt),
              (rng.integers(0, 2, (h, w)) * (5 << sh)).astype(dt),
              ((xs // 2 % 2) * mx).astype(dt)]
    closed = [None, (interior * ((8 * mx + half) >> sh), interior), (0, interior), None, (0, 0)]
    return planes, closed


def run(monkeypatch, planes, bd, *, rows=None, wide=False, view=False, batch=BATCH):
    """The frames through one estimator: (estimates, last_launch).  view: every frame a pitched, misplaced device view whose
    margin is looked at afterwards."""
    import torch

    from grav1synth_amd.estimate import NoiseEstimator
    from tests.views import device_view

    for name, value in (("G1S_ESTIMATE", "wide" if wide else None), ("G1S_ESTIMATE_ROWS", None if rows is None else str(rows))):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    est = NoiseEstimator(bd, batch_frames=batch)
    keep = []
    try:
        for k, p in enumerate(planes):
            if view:
                row = p.shape[1] * p.dtype.itemsize
                t, guard = device_view(p, pitch_bytes=row + 16, base_offset_bytes=6, fill="random", max_code=(1 << bd) - 1, seed=k)
                assert t.data_ptr() & 15 == 6
            else:
                t, guard = torch.from_numpy(p).cuda(), None
            keep.append((t, guard))
            est.estimate_frame(t)
        got = est.finish()
        info = est.last_launch()
    finally:
        est.close()
    for k, (_, guard) in enumerate(keep):
        if guard is not None:
            guard.assert_unchanged(f"frame {k}")
    return got, info


def check(got, info, want, want_sums, what):
    sums = info["sums"]
    assert len(sums) == len(want_sums) == len(got), what
    bad = [f"frame {k}: (accum, count) {sums[k]}, the oracle's {want_sums[k]}" for k in range(len(sums)) if sums[k] != want_sums[k]]
    assert not bad, what + "\n" + "\n".join(bad)
    assert got == want, what   # floats compared exactly; None where the oracle has None


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("r,w", CASES, ids=lambda v: str(v))
def test_packed_estimator_at_a_pinned_strip_height(monkeypatch, r, w, bd):
    view = w == "view"
    width = 504 if view else w
    for h in plane_heights(r):
        assert h <= 770
        planes, closed = frames_of(h, width, bd)
        want = [estimate_plane_noise(p, bd) for p in planes]
        want_sums = [estimate_plane_sums(p, bd) for p in planes]
        for k, c in enumerate(closed):   # the oracle against arithmetic done by hand, where there is some
            assert c is None or want_sums[k] == c, (k, want_sums[k], c)
        assert want[2] == 0.0 and want[4] is None and want[1] is not None
        what = f"{width} x {h} at {bd} bits, strips of {r} rows" + (", pitched view at base + 6" if view else "")
        got, info = run(monkeypatch, planes, bd, rows=r, view=view)
        # the height asked for is the height that ran: without this everything below could pass at 8 rows
        assert info["packed"] and info["launched"], (what, info)
        assert info["strip_rows"] == r and info["row_strips"] == -(-(h - 2) // r), (what, info)
        check(got, info, want, want_sums, what + ", packed")
        if r == 256:
            print(f"{what}: largest accum {max(s[0] for s in info['sums'])}, largest count {max(s[1] for s in info['sums'])}, "
                  f"a wave's at most {496 * min(r, h - 2) * ((8 * ((1 << bd) - 1) + ((1 << (bd - 8)) >> 1)) >> (bd - 8))} and {496 * min(r, h - 2)}")
        wgot, winfo = run(monkeypatch, planes, bd, rows=r, wide=True, view=view)
        assert not winfo["packed"] and winfo["strip_rows"] == 32, (what, winfo)
        check(wgot, winfo, want, want_sums, what + ", 32-bit kernel")
        assert wgot == got and winfo["sums"] == info["sums"]


def test_a_height_outside_the_range_is_clamped(monkeypatch):
    planes, _ = frames_of(40, 64, 10)
    want_sums = [estimate_plane_sums(p, 10) for p in planes]
    for asked, ran in ((3, 8), (8, 8), (256, 256), (300, 256), (-1, 8)):
        got, info = run(monkeypatch, planes, 10, rows=asked)
        assert info["packed"] and info["strip_rows"] == ran and info["row_strips"] == -(-38 // ran), (asked, info)
        assert info["sums"] == want_sums, asked
    got, info = run(monkeypatch, planes, 10, rows=0)   # 0: the plan's own
    assert info["strip_rows"] == plan_strips(40, 1, BATCH, info["cus"], info["wgs_per_cu"])[0] and info["sums"] == want_sums


def test_the_unforced_plan_on_a_tall_batch(monkeypatch):
    """8 x 65536 at 10 bits, 32 frames a batch (1 MiB a frame): one column strip a frame, so the plan's own choice is tall
    strips whatever the occupancy, over more than one resident round where the occupancy is below 8.  The height that ran is
    the one the plan's restatement gives for the device's compute units and the occupancy the launch was planned with."""
    import torch

    w, h, bd, batch = 8, 65536, 10, 32
    rng = np.random.default_rng(65536)
    mx = (1 << bd) - 1
    ys, xs = np.indices((h, w))
    kinds = [lambda: rng.integers(0, mx + 1, (h, w)), lambda: ((ys + xs) & 1) * mx, lambda: np.full((h, w), int(rng.integers(0, mx + 1))),
             lambda: rng.integers(0, 2, (h, w)) * 20, lambda: (xs // 2 % 2) * mx, lambda: 300 + rng.integers(0, 9, (h, w))]
    planes = [kinds[k % len(kinds)]().astype(np.uint16) for k in range(batch)]
    want = [estimate_plane_noise(p, bd) for p in planes]
    want_sums = [estimate_plane_sums(p, bd) for p in planes]
    got, info = run(monkeypatch, planes, bd, batch=batch)
    assert info["packed"] and info["launched"], info
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert info["cus"] == cus, (info, cus)
    planned = plan_strips(h, col_strips(w), batch, info["cus"], info["wgs_per_cu"])
    any_occupancy = {plan_strips(h, col_strips(w), batch, cus, occ)[0] for occ in range(1, 9)}
    what = (f"ran strips of {info['strip_rows']} rows, {info['row_strips']} a frame, on {info['cus']} CUs at {info['wgs_per_cu']} workgroups a CU; "
            f"the plan: {planned[0]} rows, {planned[1]} strips, k = {planned[2]}; for occupancy 1 .. 8 it gives {sorted(any_occupancy)}")
    print(what)
    assert (info["strip_rows"], info["row_strips"]) == planned[:2], what
    assert 8 <= info["strip_rows"] <= 256 and info["strip_rows"] in any_occupancy, what
    assert min(any_occupancy) > 32, "taller than anything a small case runs, for every occupancy: " + what
    check(got, info, want, want_sums, what)


@pytest.mark.parametrize("wide", [False, True], ids=["packed", "wide"])
@pytest.mark.parametrize("bd", [8, 10])
def test_fifteen_and_sixteen_interior_pixels(monkeypatch, bd, wide):
    """The estimate exists from 16 smooth pixels on: a flat 17 x 3 plane has 15 (None, and the count says 15), a flat 18 x 3
    plane has 16 (0.0)."""
    dt = np.uint8 if bd == 8 else np.uint16
    for w, want, sums in ((17, None, (0, 15)), (18, 0.0, (0, 16))):
        p = np.full((3, w), 9 << (bd - 8), dt)
        assert estimate_plane_noise(p, bd) == want and estimate_plane_sums(p, bd) == sums
        got, info = run(monkeypatch, [p, p], bd, wide=wide, batch=2)
        assert info["launched"] and info["packed"] == (not wide) and info["row_strips"] == 1, info
        assert got == [want, want] and info["sums"] == [sums, sums], (w, got, info)
