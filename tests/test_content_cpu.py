"""CPU suite, part 4: the asymmetric content family (tests/content.py) stays discriminating, and the host side gives the
oracle's table on it.

tests/test_gpu_records.py compares the kernels with the oracle on this content; what that proves depends on the content
telling Cb from Cr, left from right and rows from columns -- in the oracle's own table, where a table test can see it.  These
checks hold that, wherever the oracle runs."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch.multiprocessing as mp

from grav1synth_amd.diff import RecordFold, format_tbl, latest_from_records
from grav1synth_amd.tbl import GrainTable, parse_tbl, parse_tbl_native
from tests.content import KINDS, make_frames
from tests.helpers import record_from_oracle
from tests.oracle_binding import OracleDiff, format_tbl as oracle_tbl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = Fraction(24, 1)


def _oracle_table(kinds, w, h, bd, xd, yd, lag=3, transform=None, records=None):
    """The oracle's table for frames 0, 1, ... of the given kinds; `transform` maps a list of planes to the list that goes in;
    `records`: a list that takes every frame's record as the product would have written it."""
    o = OracleDiff(FPS.numerator, FPS.denominator, bd, bd, lag, True)
    for k, kind in enumerate(kinds):
        s, d = make_frames(kind, w, h, bd, xd, yd, k)
        if transform:
            s, d = transform(s), transform(d)
        o.diff_frame(s, d, xd, yd)
        if records is not None:
            records.append(record_from_oracle(o, (s[0].shape[1], s[0].shape[0], xd, yd), lag, 3).buf.copy())
    return oracle_tbl(o.finish())


def _swap_chroma(planes):
    return [planes[0], planes[2], planes[1]]


def _mirror(planes):
    return [np.ascontiguousarray(p[:, ::-1]) for p in planes]


def _transpose(planes):
    return [np.ascontiguousarray(p.T) for p in planes]


def test_every_kind_is_deterministic_and_has_the_layout_of_np_pair():
    for kind in KINDS:
        for bd, xd, yd in ((8, 1, 1), (10, 1, 0), (12, 0, 0)):
            a, b = make_frames(kind, 166, 100, bd, xd, yd, 3), make_frames(kind, 166, 100, bd, xd, yd, 3)
            other = make_frames(kind, 166, 100, bd, xd, yd, 4)
            for side in (0, 1):
                assert [p.shape for p in a[side]] == [(100, 166), (100 >> yd, 166 >> xd), (100 >> yd, 166 >> xd)]
                assert all(p.dtype == (np.uint8 if bd == 8 else np.uint16) and p.flags["C_CONTIGUOUS"] for p in a[side])
                assert all(np.array_equal(p, q) for p, q in zip(a[side], b[side]))
                assert all(int(p.max()) < (1 << bd) for p in a[side])
            assert not np.array_equal(a[0][0], other[0][0])
    with pytest.raises(ValueError):
        make_frames("nothing", 64, 64, 8, 1, 1, 0)


def test_kinds_are_what_they_say():
    """flat: (nearly) every block accepted; distinct: the textured part refused; busy: a few left, and at least two; damaged:
    the mask of distinct (the finder reads the source) and residuals outside int8 in many blocks of every plane, at both ends of
    64-sample runs; clamped: residuals cut at both ends of the range."""
    w, h, bd = 640, 384, 10
    masks = {}
    for kind in KINDS:
        o = OracleDiff(24, 1, bd, bd, 3, True)
        s, d = make_frames(kind, w, h, bd, 1, 1, 0)
        o.diff_frame(s, d, 1, 1)
        masks[kind] = o.flat_mask() != 0
    nb = masks["flat"].size
    assert masks["flat"].sum() >= nb * 9 // 10
    assert nb // 2 <= masks["distinct"].sum() <= nb * 8 // 10
    assert not masks["distinct"][6:, 14:].any() and masks["distinct"][:3].sum() >= 3 * 20 * 8 // 10
    assert 12 <= masks["busy"].sum() <= nb // 4  # (fewer than two is the refusal that ends a job)
    assert np.array_equal(masks["damaged"], masks["distinct"])
    s, d = make_frames("damaged", w, h, bd, 1, 1, 0)
    for c in range(3):
        big = np.abs(s[c].astype(np.int64) - d[c]) > 127 << 2
        ys, xs = np.nonzero(big)
        assert len({(y // 32, x // 32) for y, x in zip(ys, xs)}) >= 20, f"plane {c}"
        assert (xs % 64 >= 61).any() and (xs % 64 <= 2).any(), f"plane {c}"
    s, d = make_frames("clamped", w, h, bd, 1, 1, 0)
    for c in range(3):
        assert (s[c][:, : 4] == 0).any() and (s[c][:, -4:] == 1023).any(), f"plane {c}"


@pytest.mark.parametrize("bd,xd,yd", [(8, 1, 1), (10, 1, 1), (8, 0, 0), (10, 0, 0)])
def test_distinct_content_gives_three_different_planes(bd, xd, yd):
    segs = parse_tbl(_oracle_table(["distinct"] * 3, 320, 192, bd, xd, yd))
    assert len(segs) == 1
    t = segs[0]
    assert t.scaling_points_cb != t.scaling_points_cr
    assert len(t.scaling_points_cb) > 2 and len(t.scaling_points_cr) > 2 and len(t.scaling_points_y) > 2
    far = lambda a, b: sum(abs(x - y) >= 4 for x, y in zip(a, b))  # (zip: the 24 spatial coefficients when one side is luma)
    assert far(t.ar_coeffs_y, t.ar_coeffs_cb) >= 5 and far(t.ar_coeffs_y, t.ar_coeffs_cr) >= 5 and far(t.ar_coeffs_cb, t.ar_coeffs_cr) >= 5
    assert t.ar_coeffs_cb[-1] > 0 > t.ar_coeffs_cr[-1], "luma enters Cb with a positive weight and Cr with a negative one"


@pytest.mark.parametrize("bd,xd,yd", [(8, 1, 1), (10, 0, 0)])
def test_table_changes_when_cb_and_cr_are_exchanged(bd, xd, yd):
    assert _oracle_table(["distinct"] * 3, 320, 192, bd, xd, yd) != _oracle_table(["distinct"] * 3, 320, 192, bd, xd, yd, transform=_swap_chroma)


@pytest.mark.parametrize("bd,xd,yd", [(8, 1, 1), (10, 0, 0)])
def test_table_changes_when_every_plane_is_mirrored(bd, xd, yd):
    a = parse_tbl(_oracle_table(["distinct"] * 3, 320, 192, bd, xd, yd))[0]
    b = parse_tbl(_oracle_table(["distinct"] * 3, 320, 192, bd, xd, yd, transform=_mirror))[0]
    for name in ("ar_coeffs_y", "ar_coeffs_cb", "ar_coeffs_cr"):  # not through the scaling points alone: every plane's coefficients
        assert sum(abs(x - y) >= 4 for x, y in zip(getattr(a, name), getattr(b, name))) >= 2, name


@pytest.mark.parametrize("bd,xd,yd", [(8, 1, 1), (10, 0, 0)])
def test_table_changes_when_every_plane_is_transposed(bd, xd, yd):
    a = parse_tbl(_oracle_table(["distinct"] * 3, 256, 256, bd, xd, yd))[0]
    b = parse_tbl(_oracle_table(["distinct"] * 3, 256, 256, bd, xd, yd, transform=_transpose))[0]
    for name in ("ar_coeffs_y", "ar_coeffs_cb", "ar_coeffs_cr"):
        assert sum(abs(x - y) >= 4 for x, y in zip(getattr(a, name), getattr(b, name))) >= 2, name


FOLD_CASES = [
    (["distinct"] * 3, 320, 192, 10, 1, 1, 3),
    (["distinct"] * 3, 326, 198, 8, 1, 1, 2),
    (["distinct"] * 2, 256, 160, 10, 0, 0, 3),
    (["distinct"] * 2, 320, 192, 8, 1, 0, 1),
    (["clamped"] * 3, 320, 192, 8, 1, 1, 3),
    (["clamped"] * 2, 256, 160, 10, 0, 0, 2),
    (["distinct", "distinct", "busy", "busy", "flat", "flat"], 320, 192, 8, 1, 1, 3),
    (["distinct", "busy", "flat", "damaged", "flat"], 320, 200, 10, 1, 0, 1),
]


@pytest.mark.parametrize("kinds,w,h,bd,xd,yd,lag", FOLD_CASES, ids=lambda v: "-".join(v) if isinstance(v, list) else str(v))
def test_host_fold_on_oracle_records_gives_the_oracles_table(kinds, w, h, bd, xd, yd, lag):
    """RecordFold over records holding the oracle's integers, frame by frame; the per-frame half (latest_from_records) and the
    ordered half (push_latest_many) over the same records: the oracle's table each way."""
    recs = []
    want = _oracle_table(kinds, w, h, bd, xd, yd, lag, records=recs)
    fold = RecordFold(FPS, lag)
    for r in recs:
        fold.push(r)
    assert format_tbl(fold.finish()) == want
    fold = RecordFold(FPS, lag)
    fold.push_latest_many(latest_from_records(np.stack(recs), lag))
    assert format_tbl(fold.finish()) == want


def _shard_worker(rank, world, port, nframes, out_path):
    """tests/test_dist_cpu.py's record shard (a contiguous chunk of frames a rank, one all-gather, rank 0 folds in frame order) on
    `distinct` frames, the kind changing to `busy` in the last third."""
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from grav1synth_amd.dist import fold_records, gather_records

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per = (nframes + world - 1) // world
    recs = []
    for k in range(rank * per, min(nframes, (rank + 1) * per)):
        o = OracleDiff(24, 1, 8, 8, 3, True)  # (records are per-frame: a fresh oracle a frame gives the same integers)
        s, d = make_frames(_shard_kind(k, nframes), 256, 160, 8, 1, 1, k)
        o.diff_frame(s, d, 1, 1)
        recs.append(record_from_oracle(o, (256, 160, 1, 1), 3, 3).buf)
    per_rank = gather_records(np.stack(recs) if recs else np.zeros((0, 0), np.uint8), dist)
    if rank == 0:
        with open(out_path, "wb") as f:
            f.write(format_tbl(fold_records(per_rank, FPS, 3)))
    dist.barrier()
    dist.destroy_process_group()


def _shard_kind(k, nframes):
    return "busy" if k >= nframes - nframes // 3 else "distinct"


@pytest.mark.parametrize("world,nframes", [(2, 5), (3, 7)])
def test_record_shards_over_gloo_give_the_oracles_table(tmp_path, world, nframes):
    out = str(tmp_path / "sharded.tbl")
    port = 33500 + (os.getpid() % 2000) + world
    mp.spawn(_shard_worker, args=(world, port, nframes, out), nprocs=world, join=True)
    want = _oracle_table([_shard_kind(k, nframes) for k in range(nframes)], 256, 160, 8, 1, 1)
    assert open(out, "rb").read() == want


def test_table_with_three_different_planes_round_trips_and_drives_the_lookup():
    """parse(format(x)) == x through both readers on a table whose Cb and Cr entries differ in every list, and
    g1s_tbl_segment_for hands back that segment's own Cb and Cr (a `damaged` job: the oracle cuts it into two segments)."""
    raw = _oracle_table(["distinct"] * 2 + ["damaged"] * 2, 320, 192, 8, 1, 1)
    segs = parse_tbl(raw)
    assert segs == parse_tbl_native(raw) and format_tbl(segs) == raw
    assert len(segs) >= 2
    for s in segs:
        assert s.scaling_points_cb != s.scaling_points_cr and s.ar_coeffs_cb != s.ar_coeffs_cr
        assert s.scaling_points_y != s.scaling_points_cb and s.ar_coeffs_y != s.ar_coeffs_cb[:-1]
    assert segs[0].ar_coeffs_cb != segs[1].ar_coeffs_cb
    table = GrainTable(segs)
    for i, s in enumerate(segs):
        hit = table.segment_for(s.start_time)
        assert hit is not None and hit.start_time == s.start_time
        assert (hit.scaling_points_y, hit.scaling_points_cb, hit.scaling_points_cr) == (s.scaling_points_y, s.scaling_points_cb, s.scaling_points_cr)
        assert (hit.ar_coeffs_y, hit.ar_coeffs_cb, hit.ar_coeffs_cr) == (s.ar_coeffs_y, s.ar_coeffs_cb, s.ar_coeffs_cr)
        assert (hit.cb_mult, hit.cb_luma_mult, hit.cb_offset, hit.cr_mult, hit.cr_luma_mult, hit.cr_offset) == \
            (s.cb_mult, s.cb_luma_mult, s.cb_offset, s.cr_mult, s.cr_luma_mult, s.cr_offset)
