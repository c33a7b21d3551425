"""tests/mask_content.py gives what tests/test_gpu_mask_patterns.py needs, without a device: over every geometry's list of
designs the ORACLE's masks (not the designs) reach every pattern of flat neighbours at every position in a unit, the unit
boundaries and list gaps the accumulation kernels have to tell apart, the ragged edges and the percentile-only blocks; the
damaged jobs defer units beside units that stay; the content is deterministic; and tests/content.py, whose frame body
mask_content shares, still returns the bytes committed goldens were made from.  A design list or a seed that stops reaching
something fails here by name."""
import hashlib
import itertools

import numpy as np
import pytest

from tests import content, mask_content as MC
from tests.test_gpu_mask_patterns import GEOMS, STREAM, WIDE, _job, job_designs


def _masks(geom, damage=False):
    nbh, nbw = (geom.h + 31) // 32, (geom.w + 31) // 32
    return [sh["mask"].reshape(nbh, nbw) for sh in _job(geom, damage)[1]]


def _cells(flat, unit):
    """(nbh, cells) flat bits of the units of `unit` blocks, bit k = block k of the unit."""
    nbh, nbw = flat.shape
    pad = np.zeros((nbh, -(-nbw // unit) * unit), bool)
    pad[:, :nbw] = flat
    return (pad.reshape(nbh, -1, unit) * (1 << np.arange(unit))).sum(axis=2)


def _keys(flat, period):
    """{(block column mod period, left flat, right flat, up flat)} of the flat blocks."""
    z = np.pad(flat, 1)
    by, bx = np.nonzero(flat)
    return set(zip((bx % period).tolist(), z[by + 1, bx].tolist(), z[by + 1, bx + 2].tolist(), z[by, bx + 1].tolist()))


def _events(m, geom):
    """The names of the single cases the mask `m` holds."""
    flat, out = m != 0, set()
    nbh, nbw = flat.shape
    for unit in (4, 8):
        cells = _cells(flat, unit)
        if ((cells[:, :-1] == 1 << (unit - 1)) & (cells[:, 1:] == 1)).any():
            out.add(f"a flat pair across a boundary of {unit}-block units, nothing else in either")
    for unit in (2, 4, 8):
        listed = np.argwhere(_cells(flat, unit) != 0)  # raster order
        same_row = listed[1:, 0] == listed[:-1, 0]
        if (same_row & (listed[1:, 1] > listed[:-1, 1] + 1)).any():
            out.add(f"a listed {unit}-block unit behind a gap in its block row")
        if (listed[1:, 0] == listed[:-1, 0] + 1).any():
            out.add(f"a listed {unit}-block unit whose predecessor lies in the row above")
    if geom.w % 32 and flat[:, -1].any():
        out.add("a flat block in the ragged last block column")
    if geom.h % 32 and flat[-1].any():
        out.add("a flat block in the ragged last block row")
    if (m == 1).any():
        out.add("mask value 1")
    return out


def _wanted_events(geom):
    out = {f"a flat pair across a boundary of {u}-block units, nothing else in either" for u in (4, 8)}
    # (a gap needs three units in a block row: 512 samples are two units of 8 blocks, and no kernel forms such units at 4:4:4)
    out |= {f"a listed {u}-block unit behind a gap in its block row" for u in (2, 4, 8) if -(-geom.w // (32 * u)) >= 3}
    out |= {f"a listed {u}-block unit whose predecessor lies in the row above" for u in (2, 4, 8)}
    out |= {"a flat block in the ragged last block column"} if geom.w % 32 else set()
    out |= {"a flat block in the ragged last block row"} if geom.h % 32 else set()
    return out | {"mask value 1"}


def coverage(geom):
    """What the oracle's masks of the geometry's job reach: the keys by column mod 4 and mod 8, the four-block patterns of whole luma
    units, the single cases."""
    k4, k8, pats, events = set(), set(), set(), set()
    for m in _masks(geom):
        flat = m != 0
        k4 |= _keys(flat, 4)
        k8 |= _keys(flat, 8)
        whole = _cells(flat[:, :flat.shape[1] // 4 * 4], 4)
        pats |= set(whole[whole != 0].tolist())
        events |= _events(m, geom)
    return k4, k8, pats, events


@pytest.mark.parametrize("name", list(GEOMS))
def test_oracle_masks_of_a_geometrys_designs_reach_every_pattern(name):
    geom = GEOMS[name][0]
    k4, k8, pats, events = coverage(geom)
    print(f"{name}: {len(k4)} of 32, {len(k8)} of 64, {len(pats)} of 15, {len(events)} of {len(_wanted_events(geom))} single cases")
    bits = list(itertools.product((False, True), repeat=3))
    for period, have in ((4, k4), (8, k8)):
        missing = sorted({(p,) + b for p in range(period) for b in bits} - have)
        assert not missing, f"{name}: no flat block with (column mod {period}, left, right, up flat) in {missing}"
    missing = sorted(set(range(1, 16)) - pats)
    assert not missing, f"{name}: no whole luma unit with the flat bits {[format(p, '04b') for p in missing]}"
    missing = sorted(_wanted_events(geom) - events)
    assert not missing, f"{name}: no mask holds {missing}"
    values = set(np.unique(np.concatenate([m.ravel() for m in _masks(geom)])).tolist())
    assert values == {0, 1, 255}, f"{name}: mask values {sorted(values)}"


def _damage_grid(s, d, bw, bh, shape):
    """(nbh, nbw) bool: the blocks (bh x bw samples) with a residual outside int8."""
    bad = np.abs(s.astype(np.int64) - d.astype(np.int64)) > 127
    h, w = bad.shape
    pad = np.zeros((shape[0] * bh, shape[1] * bw), bool)
    pad[:h, :w] = bad
    return pad.reshape(shape[0], bh, shape[1], bw).any(axis=(1, 3))


@pytest.mark.parametrize("name", [WIDE, STREAM])
def test_damaged_jobs_defer_units_beside_units_that_stay(name):
    """In one frame: damage in a flat block of a unit with another flat block (the unit goes as a whole), damage in a flat block
    whose left or right neighbour unit is flat and whole, and a flat unit of 8 blocks (a chroma unit) whole in all three planes."""
    geom = GEOMS[name][0]
    assert geom.src_bd == geom.den_bd == 8
    frames, masks = _job(geom, True)[0], _masks(geom, True)
    hits = {}
    for unit in (2, 4):
        for k, ((s, d), m) in enumerate(zip(frames, masks)):
            flat = m != 0
            dmg = [_damage_grid(s[c], d[c], 32 >> (geom.xd if c else 0), 32 >> (geom.yd if c else 0), flat.shape) for c in range(3)]
            cells, hurt = _cells(flat, unit), _cells(dmg[0], unit) != 0
            hit_flat = _cells(dmg[0] & flat, unit)
            shared = (hit_flat != 0) & (cells & ~hit_flat != 0)
            whole = (cells != 0) & ~hurt
            beside = (hit_flat[:, 1:] != 0) & whole[:, :-1] | (hit_flat[:, :-1] != 0) & whole[:, 1:]
            chroma_whole = (_cells(flat, 8) != 0) & (_cells(dmg[0] | dmg[1] | dmg[2], 8) == 0)
            if shared.any() and beside.any() and chroma_whole.any() and hurt.any():
                hits.setdefault(unit, []).append(k)
    print(f"{name}: frames with all three, by unit size: {hits}")
    assert set(hits) == {2, 4}, f"{name}: no frame defers a shared unit beside a whole one (units of {sorted({2, 4} - set(hits))} blocks)"
    undamaged = _job(geom, False)[0]
    assert any(not np.array_equal(a[1][0], b[1][0]) for a, b in zip(frames, undamaged))
    assert all(np.array_equal(a[0][c], b[0][c]) for a, b in zip(frames, undamaged) for c in range(3)), "damage is on the denoised side only"


def test_texture_lies_on_the_blocks_marked_0_and_nowhere_else():
    """The denoised luma of a designed frame differs from the all-flat frame's on every sample of the blocks marked 0 (the checker
    is never zero and the ramp stays clear of 0 and 255) and on no other."""
    w, h = 646, 342
    nbh, nbw = (h + 31) // 32, (w + 31) // 32
    design = MC.designs(nbh, nbw)["rand50a"]
    d = MC.make_frames(design, w, h, 8, 1, 1, 0)[1]
    d0 = MC.make_frames(np.ones_like(design), w, h, 8, 1, 1, 0)[1]
    changed = d[0] != d0[0]
    tex = np.repeat(np.repeat(design == 0, 32, axis=0), 32, axis=1)[:h, :w]
    assert not (changed & ~tex).any() and changed[tex].all()
    assert all(np.array_equal(d[c], d0[c]) for c in (1, 2))
    flat = content.make_frames("flat", w, h, 8, 1, 1, 0)
    ones = MC.make_frames(np.ones_like(design), w, h, 8, 1, 1, 0)
    assert all(np.array_equal(a, b) for x, y in zip(flat, ones) for a, b in zip(x, y)), "an all-1 design is content's `flat` frame"


def test_make_frames_and_designs_are_deterministic():
    for (w, h, bd, xd, yd) in ((646, 342, 8, 1, 1), (512, 256, 10, 0, 0)):
        nbh, nbw = (h + 31) // 32, (w + 31) // 32
        a, b = MC.designs(nbh, nbw), MC.designs(nbh, nbw)
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) and a[k].shape == (nbh, nbw) for k in a)
        assert all(set(np.unique(v).tolist()) <= {0, 1} for v in a.values())
        assert a["sparse"].mean() < 0.1 < a["rand25"].mean() < a["rand50a"].mean() < a["rand85"].mean()
        assert not np.array_equal(a["rand50a"], a["rand50b"])
        for damage in (False, True):
            x = MC.make_frames(a["rand50a"], w, h, bd, xd, yd, 3, seed=2, damage=damage)
            y = MC.make_frames(a["rand50a"], w, h, bd, xd, yd, 3, seed=2, damage=damage)
            assert all(np.array_equal(p, q) and p.dtype == q.dtype and p.flags.c_contiguous for s, t in zip(x, y) for p, q in zip(s, t))
            assert [p.shape for p in x[0]] == [(h, w), (h >> yd, w >> xd), (h >> yd, w >> xd)]
        other = MC.make_frames(a["rand50a"], w, h, bd, xd, yd, 3, seed=3)
        assert not np.array_equal(other[0][0], MC.make_frames(a["rand50a"], w, h, bd, xd, yd, 3, seed=2)[0][0])
    with pytest.raises(ValueError):
        MC.make_frames(np.ones((3, 3), np.uint8), 646, 342, 8, 1, 1, 0)


def test_designs_are_what_their_names_say():
    nbh, nbw = 11, 20
    d = {k: v.astype(bool) for k, v in MC.designs(nbh, nbw).items()}
    z = {k: np.pad(v, 1) for k, v in d.items()}
    left, right, up = (lambda k: z[k][1:-1, :-2][d[k]]), (lambda k: z[k][1:-1, 2:][d[k]]), (lambda k: z[k][:-2, 1:-1][d[k]])
    for k in ("checker0", "checker1"):
        assert not left(k).any() and not right(k).any() and not up(k).any()
    assert not np.array_equal(d["checker0"], d["checker1"])
    for k in ("cols2", "cols3"):
        assert not left(k).any() and not right(k).any() and d[k][1:][d[k][:-1]].all()
    assert not up("rows2").any() and d["rows2"][1].all() and not d["rows2"][0].any()
    for unit, k in ((4, "straddle4"), (8, "straddle8")):
        rows = d[k][~d[k].all(axis=1)]  # (straddle8 has whole flat rows between)
        cells = _cells(rows, unit)
        assert set(np.unique(cells).tolist()) <= {0, 1, 1 << (unit - 1)}, "one flat block a unit"
        pairs = (cells[:, :-1] == 1 << (unit - 1)) & (cells[:, 1:] == 1)
        assert pairs.any(axis=0).all(), "every boundary between units is straddled in some row"
        assert rows.sum() == 2 * pairs.sum() and d[k].mean() > 0.15
    cells = _cells(d["cells8"], 8)
    assert set(np.unique(cells).tolist()) <= {0, 15, 255} and (cells[:, 0] != 0).any() and (cells[:, 0] == 0).any()
    for unit, k in ((4, "single4"), (8, "single8")):
        cells = _cells(d[k][:, :nbw // unit * unit], unit)
        assert set(np.unique(cells).tolist()) == {1 << p for p in range(unit)}


# sha256 over (dtype, shape, bytes) of the six planes, computed at the commit before content.make_frames was split in two
PARENT_DIGESTS = {
    ("distinct", 320, 192, 8, 1, 1, 0, 1): "d045106dd0d01b8d34a7e5192a3083e1beb0b277f44721ab5610013d664456a4",
    ("flat", 326, 198, 10, 1, 1, 1, 1): "ff7acd41ef6421d399ab56db5b2f59b49acbb0d97d61ea9f80aadc8e9d8a3c58",
    ("busy", 256, 160, 10, 0, 0, 2, 3): "637a25bca7c8712b0280263fd160d7a1f383e836ffdb368a30bc5fa91e5ebdb6",
    ("damaged", 320, 200, 12, 1, 0, 3, 1): "d5a18531a45caa089d84faac2d9e98515005e3f99b28fe88642020844c8eb763",
    ("clamped", 352, 208, 8, 1, 1, 4, 2): "c6b96ea24857232ab31d3ac4852afbbb8263f75de933d8e334964af5f6ec4650",
}


def test_content_kinds_return_the_bytes_they_returned_before():
    assert {k[0] for k in PARENT_DIGESTS} == set(content.KINDS)
    for case, want in PARENT_DIGESTS.items():
        s, d = content.make_frames(*case[:7], seed=case[7])
        h = hashlib.sha256()
        for p in s + d:
            h.update(str((p.dtype.str, p.shape)).encode())
            h.update(p.tobytes())
        assert h.hexdigest() == want, case


def test_every_job_has_a_short_last_batch_and_distinct_designs():
    for name, (geom, _) in GEOMS.items():
        ds = job_designs(geom)
        assert len(ds) % 5 and len(ds) > 10, name
        assert len({v.tobytes() for _, v in ds}) == len(ds), name
