"""k4_latest's strength pass as a two-stage pipeline and its pivot search by cross-lane moves (csrc/latest.hip).

The pass takes a frame's blocks a STAGE of 512 at a time.  Eight partition waves place stage t + 1's terms into list buffer
(t + 1) & 1 and measure stage t + 2 into registers while two chain waves add the lists of stage t from buffer t & 1; one barrier
a stage.  What such a pipeline can get wrong is what the cases here are made of: a buffer used a second and a third time (three
to five stages, a last stage of one block, a last stage one block short), a stage with no measured block at all between, before
or behind full ones (a stale list bound, stale terms of stage t - 2), lists that are long in one stage, empty in the next and
long again, every list filled inside every stage, blocks that sit exactly on the last bin -- with 4:2:0 chroma, luma only, 4:4:4,
a ragged right and bottom edge and at 10 bits.  The solves' pivot search (a suffix arg-max with "the smaller position wins a tie")
meets residual fields of exact symmetry, whose normal equations have columns of equal magnitude or are singular.

Every case compares the device half's blobs with the host half's, byte for byte (tests/test_gpu_latest_wide.py and
tests/test_gpu_latest_lists.py hold the stage edges block by block, one-bin lists and the "not enough flat blocks" refusal).
What the host half makes of a design -- status, text, ties -- is read from the HOST half's blobs."""
from fractions import Fraction

import numpy as np
import pytest

from grav1synth_amd.diff import DiffGenerator, format_tbl
from grav1synth_amd.synth import SynthSpec, make_pair
from tests import mask_content

pytestmark = pytest.mark.gpu

STAGE = 512  # blocks a stage (kStage in csrc/latest.hip)
W = 1024     # 32 blocks a block row: a stage is 16 block rows, 512 luma rows


def _blobs(monkeypatch, where, frames, bit_depth=8, lag=3, chroma=True, xdec=1, ydec=1, batch=None):
    monkeypatch.setenv("G1S_LATEST", where)
    g = DiffGenerator(Fraction(24, 1), bit_depth, bit_depth, ar_coeff_lag=lag, luma_only=not chroma,
                      batch_frames=batch or len(frames), records_only=2)
    for s, d in frames:
        g.diff_frame(s, d, xdec, ydec)
    out = g.take_latest(len(frames) + 8, sync=True).copy()
    g.close()
    return out


def _same(host, dev, n):
    assert host.shape == dev.shape and host.shape[0] == n
    for i in range(n):
        if not np.array_equal(host[i], dev[i]):
            bad = np.flatnonzero(host[i] != dev[i])
            raise AssertionError(f"frame {i}: {bad.size} bytes differ, first at {bad[0]} (of {host.shape[1]})")


def _status(blob):
    return int(np.frombuffer(blob.tobytes()[12:16], np.int32)[0])


def _text(blob):
    return blob.tobytes()[24:128].split(b"\0")[0].decode()


def _measured(blob):
    """Blocks that went into the luma strength system (num_equations of plane 0's head, behind the 128-byte header)."""
    return int(np.frombuffer(blob.tobytes()[144:148], np.int32)[0])


def _luma_ar(blob, lag):
    """Plane 0's AR normal equations as the blob holds them: n x n packed at the front of the field behind the plane's head."""
    n = 2 * lag * (lag + 1)
    return np.frombuffer(blob.tobytes()[160:160 + 8 * n * n], np.float64).reshape(n, n).copy()


def _luma_strength_diag(blob, lag):
    """The diagonal of plane 0's 20 x 20 strength matrix: which bins the measured blocks fell into."""
    ncm = 2 * lag * (lag + 1) + 1
    off = 160 + 8 * (ncm * ncm + 2 * ncm)
    return np.frombuffer(blob.tobytes()[off:off + 8 * 400], np.float64).reshape(20, 20).diagonal().copy()


def _level_pair(level, seed, amp=3, chroma=(1, 1)):
    """A frame pair of flat blocks whose intensity is designed: `level` is the luma plane's grey per sample.  Source = level + a
    little noise, denoised = level; where level is 255 the SOURCE is exactly 255 (a block mean of 255 sits exactly on bin 19) and
    the denoised plane carries the noise below it.  Chroma planes: the level map decimated, the same law."""
    rng = np.random.default_rng(seed)
    xdec, ydec = chroma
    src, den = [], []
    for lv in (level, level[::1 << ydec, ::1 << xdec], level[::1 << ydec, ::1 << xdec]):
        lv = lv.astype(np.int64)
        n = rng.integers(-amp, amp + 1, lv.shape)
        top = lv >= 255
        s = np.where(top, 255, np.clip(lv + n, 0, 254))
        d = np.where(top, 255 - np.abs(n) - (n == 0), lv)
        src.append(np.ascontiguousarray(s.astype(np.uint8)))
        den.append(np.ascontiguousarray(d.astype(np.uint8)))
    return src, den


def _bands(h, levels):
    """(h, W) level map: one grey a stage (16 block rows), in the order given."""
    rows = np.repeat(np.asarray(levels), STAGE // (W // 32) * 32)[:h]
    assert rows.size == h
    return np.broadcast_to(rows[:, None], (h, W))


def _every_bin(h):
    """(h, W) level map whose 32 block columns run through all 20 bins in every block row, the last column exactly 255."""
    cols = np.repeat(np.concatenate([np.linspace(4, 250, 31).round(), [255]]), 32)
    return np.broadcast_to(cols[None, :], (h, W))


def _check(monkeypatch, frames, bit_depth=8, lag=3, chroma=True, xdec=1, ydec=1):
    host = _blobs(monkeypatch, "host", frames, bit_depth, lag, chroma, xdec, ydec)
    dev = _blobs(monkeypatch, "device", frames, bit_depth, lag, chroma, xdec, ydec)
    _same(host, dev, len(frames))
    return host


# ---- a buffer used again: three, four, five stages; a last stage of one block; a last stage one block short ----
@pytest.mark.parametrize("chroma", [True, False], ids=["420", "luma_only"])
@pytest.mark.parametrize("w,h,blocks", [
    (W, 1536, 3 * STAGE),
    (W, 2048, 4 * STAGE),
    (W, 2560, 5 * STAGE),
    (928, 1696, 3 * STAGE + 1),  # 29 x 53 blocks: the fourth stage holds one block
    (736, 2848, 4 * STAGE - 1),  # 23 x 89 blocks: the fourth stage is one block short
], ids=lambda v: str(v))
def test_three_to_five_stages_give_the_host_halfs_bytes(monkeypatch, w, h, blocks, chroma):
    spec = SynthSpec(w, h, 8, textured=False)
    assert ((w + 31) // 32) * ((h + 31) // 32) == blocks
    frames = [make_pair(spec, k, device="cuda") for k in range(2)]
    host = _check(monkeypatch, frames, chroma=chroma)
    assert all(_status(b) == 0 for b in host)
    assert min(_measured(b) for b in host) > blocks // 2  # (all flat: nearly every block is measured)


# ---- stages without a measured block ----
def _stage_design(flat_stages, stages=4):
    """(16 * stages, 32) design: the block rows of the stages named are flat, the others textured."""
    d = np.zeros((16 * stages, W // 32), np.uint8)
    for s in flat_stages:
        d[16 * s:16 * (s + 1)] = 1
    return d


EMPTY = {
    "middle_stage_empty": (0, 2, 3),
    "first_stage_empty": (1, 2, 3),
    "last_stage_empty": (0, 1, 2),
    "only_the_last_stage": (3,),
}


@pytest.mark.parametrize("chroma", [True, False], ids=["420", "luma_only"])
@pytest.mark.parametrize("name", list(EMPTY))
def test_empty_stages_give_the_host_halfs_bytes(monkeypatch, name, chroma):
    """1024 x 2048 = four stages; texture on exactly the blocks of the stages a design leaves out.  (The finder's mask is the
    design but for a few designed-flat blocks it rejects -- by the oracle's mask no textured block of these designs is taken --
    and the count of measured blocks is held to the design's from both sides.)"""
    design = _stage_design(EMPTY[name])
    frames = [mask_content.make_frames(design, W, 2048, 8, 1, 1, k) for k in range(2)]
    host = _check(monkeypatch, frames, chroma=chroma)
    assert all(_status(b) == 0 for b in host), [(_status(b), _text(b)) for b in host]
    want = int(design.sum())
    assert all(0.9 * want <= _measured(b) <= want for b in host), ([_measured(b) for b in host], want)


# ---- bins that change from stage to stage, every bin in every stage, blocks exactly on bin 19 ----
def _bin_frames(kind, chroma=(1, 1)):
    if kind == "one_bin_a_stage":    # list 1 long in buffer 0, nothing of it in buffer 1, long again in buffer 0
        maps = [_bands(2560, lv) for lv in ([20, 130, 20, 250, 130], [250, 20, 130, 250, 20])]
    elif kind == "every_bin_in_every_stage":
        maps = [_every_bin(2048), _every_bin(1536)[:, ::-1]]
    elif kind == "exactly_on_bin_19":  # every block's mean is 255 (beside noisier blocks the finder does not take a plain one)
        maps = [_bands(1536, [255, 255, 255]), _bands(2048, [255, 255, 255, 255])]
    else:
        raise ValueError(kind)
    return [_level_pair(np.ascontiguousarray(m), 11 + i, chroma=chroma) for i, m in enumerate(maps)]


@pytest.mark.parametrize("chroma", [True, False], ids=["420", "luma_only"])
@pytest.mark.parametrize("kind", ["one_bin_a_stage", "every_bin_in_every_stage", "exactly_on_bin_19"])
def test_bins_that_change_between_stages_give_the_host_halfs_bytes(monkeypatch, kind, chroma):
    frames = _bin_frames(kind)
    # (frames of different heights cannot share a generator: one launch each)
    hosts = []
    for f in frames:
        hosts.append(_check(monkeypatch, [f, f], chroma=chroma)[0])
    diags = [_luma_strength_diag(b, 3) for b in hosts]
    if kind == "one_bin_a_stage":
        assert all(_status(b) == 0 for b in hosts), [(_status(b), _text(b)) for b in hosts]
        # levels 20 / 130 / 250: bins 1, 9 and 18 and their upper neighbours, nothing else
        assert all(set(np.flatnonzero(d)) == {1, 2, 9, 10, 18, 19} for d in diags), diags
    elif kind == "every_bin_in_every_stage":
        assert all(_status(b) == 0 for b in hosts), [(_status(b), _text(b)) for b in hosts]
        assert all((d > 0).all() for d in diags), diags
    else:
        # a frame whose every block has mean 255 fills entry (19, 19) alone, with a 1 a block
        assert all(_status(b) == 0 for b in hosts), [(_status(b), _text(b)) for b in hosts]
        assert all(set(np.flatnonzero(d)) == {19} for d in diags), diags
        assert all(d[19] == _measured(b) > 2 * STAGE for d, b in zip(diags, hosts)), diags


def test_444_gives_the_host_halfs_bytes(monkeypatch):
    """4:4:4: the chroma pass measures the luma pass' blocks at the luma geometry."""
    frames = _bin_frames("one_bin_a_stage", chroma=(0, 0))[:1] * 2
    host = _check(monkeypatch, frames, xdec=0, ydec=0)
    assert all(_status(b) == 0 for b in host)


def test_ragged_edges_give_the_host_halfs_bytes(monkeypatch):
    """1002 x 1750: 32 x 55 = 1 760 blocks in four stages; the right column is 10 luma / 5 chroma samples wide and the bottom row
    22 / 11 high, so the chroma pass' `sw * shh > 32` test drops blocks (5 x 16, 5 x 11 samples) that the luma pass measured."""
    spec = SynthSpec(1002, 1750, 8, textured=False)
    frames = [make_pair(spec, k, device="cuda") for k in range(2)]
    host = _check(monkeypatch, frames)
    assert all(_status(b) == 0 for b in host)
    assert min(_measured(b) for b in host) > 3 * STAGE


def test_10_bit_gives_the_host_halfs_bytes(monkeypatch):
    spec = SynthSpec(W, 1536, 10, textured=False)
    frames = [make_pair(spec, k, device="cuda") for k in range(2)]
    host = _check(monkeypatch, frames, bit_depth=10)
    assert all(_status(b) == 0 for b in host)
    assert min(_measured(b) for b in host) > 2 * STAGE


# ---- pivot ties ----
def _ties_on_the_way(A):
    """gauss_solve of csrc/fold.cpp on a copy of A, step for step in f64 (multiply, then subtract: no contraction): how many of
    the bubble pass' comparisons met two equal magnitudes that were not both zero, and whether the elimination went through."""
    n = A.shape[0]
    R = [[float(v) for v in row] for row in A]
    ties = 0
    for k in range(n - 1):
        for i in range(n - 1, k, -1):
            up, lo = abs(R[i - 1][k]), abs(R[i][k])
            if up == lo and up != 0.0:
                ties += 1
            if up < lo:
                R[i - 1], R[i] = R[i], R[i - 1]
        pivot = R[k]
        if abs(pivot[k]) < 1e-16:
            return ties, False
        for i in range(k, n - 1):
            row = R[i + 1]
            c = row[k] / pivot[k]
            for j in range(k + 1, n):
                row[j] = row[j] - c * pivot[j]
    return ties, all(abs(R[i][i]) >= 1e-16 for i in range(n))


def _residual_pair(kind, w=256, h=256, level=100, c=4):
    """An all-flat frame (plain grey, denoised) and a source = grey + a residual field of exact symmetry."""
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    if kind == "constant":
        r = np.full((h, w), c)
    elif kind == "checker":
        r = c * (1 - 2 * ((xs + ys) & 1))
    elif kind == "column_stripes":
        r = c * (1 - 2 * (xs & 1)) + 0 * ys
    elif kind == "row_stripes":
        r = c * (1 - 2 * (ys & 1)) + 0 * xs
    elif kind == "zero":
        r = np.zeros((h, w), np.int64)
    elif kind == "tile8":  # an 8 x 8 tile of noise, repeated: the autocorrelation has the tile's period and its mirror symmetry
        r = np.tile(np.random.default_rng(8).integers(-c, c + 1, (8, 8)), (h // 8, w // 8))
    elif kind == "checker_and_tile":  # the checkerboard with the tile on top, at half the weight
        r = 2 * c * (1 - 2 * ((xs + ys) & 1)) + np.tile(np.random.default_rng(9).integers(-c, c + 1, (8, 8)), (h // 8, w // 8))
    elif kind in ("checker_one_off", "constant_one_off", "column_stripes_one_off"):
        # the symmetric field with ONE sample perturbed: every off-diagonal entry of the normal equations keeps one magnitude, the
        # diagonal moves away from it -- columns of equal magnitudes in a system that is no longer singular
        r = np.array(np.broadcast_to({"checker": c * (1 - 2 * ((xs + ys) & 1)), "constant": np.full((h, w), c),
                                      "column_stripes": c * (1 - 2 * (xs & 1)) + 0 * ys}[kind[:-8]], (h, w)))
        r[h // 2 + 5, w // 2 + 6] += 3
    else:
        raise ValueError(kind)
    planes = [r, r[::2, ::2], r[::2, ::2]]
    src = [np.ascontiguousarray((level + p).astype(np.uint8)) for p in planes]
    den = [np.full(p.shape, level, np.uint8) for p in planes]
    return src, den


SYMMETRIC = ["constant", "checker", "column_stripes", "row_stripes", "zero", "tile8", "checker_and_tile", "checker_one_off",
             "constant_one_off", "column_stripes_one_off"]


def test_pivot_ties_give_the_host_halfs_bytes(monkeypatch):
    """Every symmetric design beside a good frame in one launch.  Which designs the host half refuses is read from its blobs; the
    designs must give both a solve that went through with ties on its way and the AR refusal of plane 0."""
    good = _level_pair(np.full((256, 256), 100), 3)
    frames = []
    for kind in SYMMETRIC:
        frames += [_residual_pair(kind), good]
    host = _check(monkeypatch, frames, chroma=False)
    seen = {}
    for i, kind in enumerate(SYMMETRIC):
        b = host[2 * i]
        ties, through = _ties_on_the_way(_luma_ar(b, 3))
        seen[kind] = (_status(b), _text(b), ties, through)
        assert _status(host[2 * i + 1]) == 0
    print(seen)
    assert any(st == 0 and ties > 0 and through for st, _, ties, through in seen.values()), seen
    assert any(st == -4 and tx == "Solving latest noise equation system failed 0!" for st, tx, _, _ in seen.values()), seen
    # with chroma: the same fields in all three planes (the chroma systems carry the luma regressor as one more column)
    host = _check(monkeypatch, frames[:8])
    assert [_status(b) for b in host[1::2]] == [0] * 4


# ---- the job ----
def test_job_table_of_a_five_stage_geometry_is_the_host_halfs(monkeypatch):
    spec = SynthSpec(W, 2560, 8)
    pairs = [make_pair(spec, k, device="cuda") for k in range(4)]
    tables = {}
    for where in ("host", "device"):
        monkeypatch.setenv("G1S_LATEST", where)
        g = DiffGenerator(Fraction(24, 1), 8, 8, batch_frames=4)
        for k in range(10):
            s, d = pairs[k % len(pairs)]
            g.diff_frame(s, d, spec.xdec, spec.ydec)
        tables[where] = format_tbl(g.finish())
        g.close()
    assert tables["device"] == tables["host"] and len(tables["host"]) > 100
