"""tests/test_gpu_k3w_slices.py cuts the slices it means to, without a device: from the ORACLE's masks of its jobs (not from the
designs) and the workgroups a frame its cases set, the luma and the chroma lists are cut into slices of 1, 2, 3 and 4 units, each
length with and without a flat neighbour in front of the slice and with and without one behind it; some workgroups get no unit; a
damaged frame has a residual outside int8 in a flat block of the last unit of a slice of odd length.  A design, a size or a count
that stops giving one of them fails here by name."""
import numpy as np
import pytest

from tests.test_gpu_k3w_slices import FORMATS, FRAMES, GEOMS, WGS, _job, slice_shapes, slices, unit_list


def _masks(geom):
    nbh, nbw = (geom.h + 31) // 32, (geom.w + 31) // 32
    return [sh["mask"].reshape(nbh, nbw) != 0 for sh in _job(geom)[1]]


def _shapes(fmt, kind):
    """{(units, ghost in front, ghost behind)} over the format's geometries, frames and cases; kind 0: luma (4 blocks a unit)."""
    out = set()
    for name, geom in GEOMS.items():
        if not name.startswith(fmt + "_"):
            continue
        for flat in _masks(geom):
            for wgs in WGS[(geom.w, geom.h)]:
                out |= slice_shapes(flat, 8 if kind else 4, int(wgs[kind]))
    return out


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_the_cases_cut_every_slice_shape(fmt):
    chroma = FORMATS[fmt][2]
    for kind in ((0, 1) if chroma else (0,)):
        have = _shapes(fmt, kind)
        print(f"{fmt}, {'chroma' if kind else 'luma'} list: {sorted(have)}")
        front = {(n, f) for n, f, _ in have}
        behind = {(n, b) for n, _, b in have}
        want = {(n, g) for n in (1, 2, 3, 4) for g in (False, True)}
        assert want <= front, f"{fmt}, kind {kind}: no slice of (units, ghost in front) {sorted(want - front)}"
        assert want <= behind, f"{fmt}, kind {kind}: no slice of (units, ghost behind) {sorted(want - behind)}"
        assert (0, False, False) in have, f"{fmt}, kind {kind}: no workgroup without a unit"


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_a_damaged_frame_defers_the_last_unit_of_an_odd_slice(fmt):
    """Luma: |source - denoised| > 127 inside a flat block of the last unit of a slice of 1 or 3 units that has a unit before it in
    the list's row or a ghost in front (the deferred unit was staged beside a neighbour)."""
    hits = []
    for name, geom in GEOMS.items():
        if not name.startswith(fmt + "_"):
            continue
        frames, masks = _job(geom)[0], _masks(geom)
        for k, ((s, d), flat) in enumerate(zip(frames, masks)):
            if not FRAMES[k][1]:
                continue
            bad = np.abs(s[0].astype(np.int64) - d[0].astype(np.int64)) > 127
            nbh, nbw = flat.shape
            pad = np.zeros((nbh * 32, nbw * 32), bool)
            pad[:bad.shape[0], :bad.shape[1]] = bad
            hurt = pad.reshape(nbh, 32, nbw, 32).any(axis=(1, 3)) & flat
            for wgs in WGS[(geom.w, geom.h)]:
                for sl in slices(unit_list(flat, 4), int(wgs[0])):
                    if len(sl) % 2 == 0:
                        continue
                    by, c = sl[-1][0], sl[-1][1]
                    if hurt[by, 4 * c:4 * c + 4].any() and (len(sl) > 1 or sl[0][2]):
                        hits.append((name, k, wgs[0], len(sl)))
    print(f"{fmt}: (geometry, frame, workgroups, units) {hits}")
    assert any(n == 1 for *_, n in hits) and any(n == 3 for *_, n in hits), f"{fmt}: {hits}"


def test_a_frames_list_is_never_empty():
    """The all-textured frame still has flat blocks (the percentile rule): the reason the GPU test runs empty slices and not an
    empty list."""
    for name, geom in GEOMS.items():
        none = _masks(geom)[[d for d, _ in FRAMES].index("none")]
        assert none.any(), name
        assert all(len(unit_list(m, 4)) > 0 for m in _masks(geom)), name
