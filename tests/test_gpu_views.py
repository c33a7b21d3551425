"""Device frames as an integrator hands them over -- a pitch larger than the row, a base off a 16-byte boundary, a hostile
margin around the samples (tests/views.py) -- through every entry point, against the references.

Every entry point takes device planes in place, and which kernel code runs is decided from those pointers and strides:

  g1s_diff::batch_geom   fast_rows (the source luma of every frame of the batch) and vec_mask (a bit a plane, ANDed over it)
  g1s_diff::wide_ok      all vec_mask bits: the wide chain (k3w_pass) or the stream chain (k3s_fused)
  k3s.hip.h              vec_all per plane class: the vector or the scalar loader of the stream chain
  estimate.hip           three load tiers by address, `fast` by base, stride and W & 7
  grain.hip              vec (in, out, both strides) and vec_luma (the co-located luma the chroma planes read)

`diff`: EVERY frame's record against the oracle's shadows and the table's bytes, as test_gpu_records.py does.  The chain a
case means is asserted on a short timed generator over the same views (_chains), outside the job under test, because a
timed batch runs on one stream: a case that silently runs the other chain fails."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Sequence, Union

import numpy as np
import pytest

from tests.test_gpu_records import CHAIN_KERNEL, FPS, JOB_KINDS, SLOTS, Geom, _generator, _job
from tests.helpers import record_mismatches
from tests.views import contiguous, device_view

pytestmark = pytest.mark.gpu
SIDES = ("source", "denoised")


# ---- placing a frame --------------------------------------------------------------------------------------------------------

class At(NamedTuple):
    """Where a plane lies: pitch rule ("+", n): row + n bytes; ("^", n): the next multiple of n above the row; ("=", n): n
    bytes -- and the base's offset from a 256-byte boundary."""
    rule: tuple = ("+", 16)
    off: int = 0
    fill: Union[str, int, tuple] = "random"

    def pitch(self, row: int) -> int:
        op, n = self.rule
        return row + n if op == "+" else (row // n + 1) * n if op == "^" else n


Place = Union[str, Sequence[At]]  # "host" (numpy), "pinned", "dev" (a fresh contiguous tensor), or an At for every plane


def _place(planes, place: Place, bit_depth: int, xd: int, yd: int, seed: int):
    """(Frame, guards) of one frame's planes placed as `place` says."""
    import torch

    from grav1synth_amd.diff import Frame

    if place == "host":
        return Frame(list(planes), xd, yd), []
    if place == "pinned":
        return Frame([torch.from_numpy(p).pin_memory() for p in planes], xd, yd, async_host=True), []
    if place == "dev":
        return Frame([contiguous(p) for p in planes], xd, yd), []
    views, guards = [], []
    for c, (p, at) in enumerate(zip(planes, place)):
        row = p.shape[1] * p.dtype.itemsize
        v, g = device_view(p, pitch_bytes=at.pitch(row), base_offset_bytes=at.off, fill=at.fill, max_code=(1 << bit_depth) - 1,
                           seed=seed * 8 + c)
        assert v.data_ptr() & 15 == at.off & 15 and v.stride(0) * p.dtype.itemsize == at.pitch(row)
        views.append(v)
        guards.append(g)
    return Frame(views, xd, yd), guards


class Placed(NamedTuple):
    pairs: list    # (source Frame, denoised Frame) of every frame of the job
    guards: list   # (what, Guard) of every plane that is a view


def _place_job(geom: Geom, frames, plan) -> Placed:
    """plan(i) -> (source Place, denoised Place) of frame i."""
    pairs, guards = [], []
    for i, (s, d) in enumerate(frames):
        ps, pd = plan(i)
        fs, gs = _place(s, ps, geom.src_bd, geom.xd, geom.yd, 2 * i)
        fd, gd = _place(d, pd, geom.den_bd, geom.xd, geom.yd, 2 * i + 1)
        pairs.append((fs, fd))
        guards += [(f"frame {i} {SIDES[side]} plane {c}", g) for side, gl in enumerate((gs, gd)) for c, g in enumerate(gl)]
    return Placed(pairs, guards)


def _feed(g, pairs) -> None:
    for s, d in pairs:
        g.diff_frame(s, d)


def _chains(geom: Geom, pairs) -> set:
    """The chains a timed generator runs on these frames as ONE batch (kernel_times: k3w_pass is the wide chain, k3s_fused
    the stream chain)."""
    g = _generator(geom, len(pairs), records_only=True)
    try:
        g.set_timing(True)
        _feed(g, pairs)
        g.sync()
        names = set(g.kernel_times())
    finally:
        g.close()
    return {c for c, k in CHAIN_KERNEL.items() if any(n.startswith(k) for n in names)}


def _check(geom: Geom, kinds, batch: int, plan, chain_of_batch, job=None) -> None:
    """The job of `kinds` placed by `plan` in batches of `batch`: the chain of every distinct kind of batch
    (chain_of_batch(j) -> "wide" / "stream", asserted once for each value's first batch), every frame's record, the table,
    and the input buffers afterwards."""
    from grav1synth_amd.diff import Record, format_tbl

    kinds = tuple(kinds)
    frames, shadows, want_tbl = job or _job(geom, kinds)
    placed = _place_job(geom, frames, plan)
    nb = (len(frames) + batch - 1) // batch
    seen = {}
    for j in range(nb):
        want = chain_of_batch(j)
        key = (want, min(batch, len(frames) - j * batch))
        if key not in seen:
            seen[key] = j
            ran = _chains(geom, placed.pairs[j * batch:(j + 1) * batch])
            assert ran == {want}, f"batch {j} was meant for the {want} chain and ran {sorted(ran)}"
    g = _generator(geom, batch, records_only=True)
    try:
        _feed(g, placed.pairs)
        recs, n = g.take_records(geom.w, geom.h, 3 if geom.chroma else 1, len(frames))
    finally:
        g.close()
    assert n == len(frames)
    bad = []
    for i in range(n):
        j = i // batch
        where = f"frame {i} ({kinds[i]}; batch {j} [{chain_of_batch(j)}], position {i % batch}, slot {j % SLOTS})"
        bad.extend(record_mismatches(shadows[i], Record(recs[i]), where))
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:40])
    g = _generator(geom, batch)
    try:
        _feed(g, placed.pairs)
        got_tbl = format_tbl(g.finish())
    finally:
        g.close()
    assert got_tbl == want_tbl
    for what, guard in placed.guards:
        guard.assert_unchanged(what)


def _all(at: At, n: int = 3):
    return [at] * n


# ---- 2a. the wide chain under a pitch -----------------------------------------------------------------------------------------

PITCH_GEOMS = {
    "8b420_320x192": Geom(320, 192, 8, 8, 1, 1, 3),
    "10b422_320x192": Geom(320, 192, 10, 10, 1, 0, 2),
    "10b444_256x160": Geom(256, 160, 10, 10, 0, 0, 3),
    "8b_luma_only_320x192": Geom(320, 192, 8, 8, 1, 1, 3, False),
    "8_10_420_320x192": Geom(320, 192, 8, 10, 1, 1, 3),   # the wide chain's general residual
}
VIEW_KINDS = ("distinct", "damaged", "clamped", "distinct")


def _pitch_plan(mode: str):
    if mode == "row+16":
        return lambda i: (_all(At(("+", 16))), _all(At(("+", 16))))
    if mode == "round256":
        return lambda i: (_all(At(("^", 256))), _all(At(("^", 256), 128)))
    if mode == "six_pitches":   # a pitch of its own for every one of the six planes; bases at different multiples of 16
        return lambda i: ([At(("+", 16 * (1 + c)), 16 * c) for c in range(3)], [At(("+", 16 * (5 + 2 * c)), 48 + 32 * c) for c in range(3)])
    if mode == "pitch_per_frame":
        return lambda i: (_all(At(("+", 16 * (1 + i)), 16 * i)), _all(At(("+", 32 * (3 - i % 3)))))
    raise KeyError(mode)


@pytest.mark.parametrize("mode", ["row+16", "round256", "six_pitches", "pitch_per_frame"])
@pytest.mark.parametrize("name", list(PITCH_GEOMS))
def test_wide_chain_reads_pitched_views_by_their_stride(name, mode):
    """Aligned bases, 16-aligned pitches larger than the row: the wide chain (k2w_select_units, k3w_pass, k3w_tail, k3m_*) and
    the fast rows of k1_moments, batches of three and one."""
    _check(PITCH_GEOMS[name], VIEW_KINDS, 3, _pitch_plan(mode), lambda j: "wide")


@pytest.mark.parametrize("fill", ["random", "max", 0])
def test_wide_chain_edge_blocks_replicate_the_plane_not_the_margin(fill):
    """336 x 200 8-bit 4:2:0, pitches 384 / 192: neither a multiple of 32, so the right and bottom edge blocks replicate the
    last column and row, whose neighbours in memory are the hostile margin; chroma 168 wide, still whole 8-sample words."""
    geom = Geom(336, 200, 8, 8, 1, 1, 3)
    place = [At(("=", 384), 0, fill), At(("=", 192), 64, fill), At(("=", 192), 128, fill)]
    _check(geom, VIEW_KINDS, 3, lambda i: (place, place), lambda j: "wide")


def test_wide_chain_at_4k_under_a_pitch_of_8192():
    """3840 x 2160 10-bit 4:2:0, three frames: luma rows of 7680 bytes 8192 apart, chroma rows of 3840 bytes 4096 apart."""
    geom = Geom(3840, 2160, 10, 10, 1, 1, 3)
    place = [At(("=", 8192)), At(("=", 4096)), At(("=", 4096))]
    _check(geom, ("distinct", "damaged", "distinct"), 2, lambda i: (place, place), lambda j: "wide")



QUIET_LEVELS = (120, 100, 150)  # 8-bit levels of Y, Cb, Cr


def _quiet_job(geom: Geom, nframes: int):
    """Frames without a picture: every denoised plane one level, the source that level plus the plane's own noise of the
    content family, a dozen code values either way.  (On the ramps of tests/content.py a row read from the wrong place leaves
    int8, the wide chain hands the unit to the exact kernel, which reads for itself, and the record comes out right: a wrong
    address in k3w_pass alone stays hidden.  Here every sample of the buffer is a plausible neighbour.)"""
    from tests.content import TAPS, _plane_noise
    from tests.helpers import oracle_shadow
    from tests.oracle_binding import OracleDiff, format_tbl as oracle_tbl

    assert geom.src_bd == geom.den_bd
    up, dt = geom.src_bd - 8, np.uint8 if geom.src_bd == 8 else np.uint16
    o = OracleDiff(FPS.numerator, FPS.denominator, geom.src_bd, geom.den_bd, geom.lag, geom.chroma)
    frames, shadows = [], []
    for k in range(nframes):
        s, d = [], []
        for c in range(3 if geom.chroma else 1):
            h, w = (geom.h >> geom.yd, geom.w >> geom.xd) if c else (geom.h, geom.w)
            n = _plane_noise(np.random.default_rng([7, k, c]), h, w, TAPS[c])
            den = np.full((h, w), QUIET_LEVELS[c] << up, np.int64)
            d.append(den.astype(dt))
            s.append((den + np.clip((n * (2 + c)) >> (10 - up), -(12 << up), 12 << up)).astype(dt))
        o.diff_frame(s, d, geom.xd, geom.yd)
        frames.append((s, d))
        shadows.append(oracle_shadow(o, len(s)))
    return frames, shadows, oracle_tbl(o.finish())


@pytest.mark.parametrize("rule", [("+", 16), ("^", 256)], ids=["row+16", "round256"])
@pytest.mark.parametrize("name", ["8b420_320x192", "10b444_256x160"])
def test_wide_chain_on_views_whose_margin_looks_like_the_picture(name, rule):
    """A crop of a larger surface: what lies beside and between the rows is more of the same picture.  Nothing a kernel reads
    from the wrong address trips a range guard; only the sums can tell."""
    geom = PITCH_GEOMS[name]
    up = geom.src_bd - 8

    def places(off):
        return [At(rule, off, ((QUIET_LEVELS[c] - 12) << up, (QUIET_LEVELS[c] + 12) << up)) for c in range(3)]

    _check(geom, ("quiet",) * 4, 3, lambda i: (places(0), places(64)), lambda j: "wide", job=_quiet_job(geom, 4))


# ---- 2b. one vec_mask bit at a time -------------------------------------------------------------------------------------------

BIT_GEOMS = {"8b420": Geom(320, 192, 8, 8, 1, 1, 3), "10b420": Geom(320, 192, 10, 10, 1, 1, 2)}
PLANES6 = ["src_Y", "src_Cb", "src_Cr", "den_Y", "den_Cb", "den_Cr"]
OFF_BITS = {"base+2": At(("+", 16), 2), "base+4": At(("+", 32), 4), "base+8": At(("^", 256), 8), "stride=8mod16": At(("+", 8), 0)}


@pytest.mark.parametrize("how", list(OFF_BITS))
@pytest.mark.parametrize("plane", PLANES6)
@pytest.mark.parametrize("name", list(BIT_GEOMS))
def test_one_misaligned_plane_of_one_frame_moves_the_batch_to_the_stream_chain(name, plane, how):
    """Eleven planes of a batch of two on 16-byte boundaries under a 16-aligned pitch, one plane of the second frame not: off by
    2, 4 or 8 bytes, or on a boundary with every second row off by 8.  "den_Y" leaves the source luma aligned (fast_rows
    stays, the chain changes), "src_Y" drops both.  The stream chain's loader of that plane class turns scalar."""
    k = PLANES6.index(plane)

    def plan(i):
        places = [At(("+", 16), 16 * c) for c in range(6)]
        if i == 1:
            places[k] = OFF_BITS[how]
        return places[:3], places[3:]

    _check(BIT_GEOMS[name], ("distinct", "damaged", "clamped"), 2, plan, lambda j: "stream" if j == 0 else "wide")


# ---- 2c. mixed batches ----------------------------------------------------------------------------------------------------------

WIDE_8 = Geom(320, 192, 8, 8, 1, 1, 3)
ALIGNED = (_all(At(("+", 16))), _all(At(("+", 48), 32)))


def _misaligned(k: int):
    """Both frames' planes aligned under a pitch but plane k of the six, which is off by 2 + 2 * k bytes."""
    places = list(ALIGNED[0]) + list(ALIGNED[1])
    places[k] = At(("+", 16), 2 + 2 * k)
    return places[:3], places[3:]


@pytest.mark.parametrize("position", [0, 2, 3])
def test_one_misaligned_frame_in_a_batch_of_four(position):
    """vec_mask and fast_rows are per batch, the pointers per frame: one frame with a misaligned source luma (first, in the
    middle, last of four) takes the whole batch to the stream chain; the second batch (two aligned frames) runs wide."""
    plan = lambda i: _misaligned(0 if position != 2 else 4) if i == position else ALIGNED
    _check(WIDE_8, ("distinct", "damaged", "clamped", "distinct", "busy", "flat"), 4, plan, lambda j: "stream" if j == 0 else "wide")


def _batch_is_misaligned(j: int) -> bool:
    # a slot is batch mod 6, so a plain alternation (and any period that divides six) gives a slot one chain only: the phase
    # flips after seven batches
    return bool(j & 1) if j < 7 else not j & 1


def _alternating_plan(i: int):
    j = i // 2
    if _batch_is_misaligned(j) and (i % 2 == j % 2 or i == len(JOB_KINDS) - 1):  # one frame of the batch, plane j mod 6
        return _misaligned(j % 6)
    return ALIGNED


def alternation_covers_every_slot() -> bool:
    """Every slot meets an aligned and a misaligned batch, and a batch is misaligned exactly when one of its frames is."""
    nb = (len(JOB_KINDS) + 1) // 2
    slots = all({_batch_is_misaligned(j) for j in range(slot, nb, SLOTS)} == {False, True} for slot in range(SLOTS))
    return slots and all(any(_alternating_plan(i) is not ALIGNED for i in range(2 * j, min(2 * j + 2, len(JOB_KINDS)))) == _batch_is_misaligned(j)
                         for j in range(nb))


def test_every_record_of_a_job_whose_batches_change_chain_because_of_alignment():
    """29 frames in batches of two, content kind changing as in test_gpu_records.py: every slot runs the wide and the stream
    chain, each through buffers the other used before."""
    assert alternation_covers_every_slot()
    _check(WIDE_8, JOB_KINDS, 2, _alternating_plan, lambda j: "stream" if _batch_is_misaligned(j) else "wide")


def test_alternating_job_device_half_gives_the_host_halfs_table(monkeypatch):
    from grav1synth_amd.diff import format_tbl

    frames, _, want = _job(WIDE_8, JOB_KINDS)
    placed = _place_job(WIDE_8, frames, _alternating_plan)
    tbl = {}
    for where in ("host", "device"):
        monkeypatch.setenv("G1S_LATEST", where)
        g = _generator(WIDE_8, 2)
        g.set_timing(True)
        try:
            _feed(g, placed.pairs)
            tbl[where] = format_tbl(g.finish())
            assert ("k4_latest" in g.kernel_times()) == (where == "device")
        finally:
            g.close()
    assert tbl["device"] == tbl["host"] == want


# ---- 2d. kinds of frame in one batch ------------------------------------------------------------------------------------------

KINDS4 = ["host", "pinned", "dev", "view"]


def _kind_place(kind: str, view) -> Place:
    return view if kind == "view" else kind


@pytest.mark.parametrize("view,chain", [(ALIGNED, "wide"), (_misaligned(5), "stream")], ids=["aligned_view", "misaligned_view"])
def test_host_pinned_contiguous_and_view_frames_in_one_batch(view, chain):
    """Batches of four that hold a numpy frame, a pinned one (async_host), a contiguous device tensor and a device view, in
    an order that turns from batch to batch; host frames are staged into 16-byte-aligned rows, so the view decides the chain."""
    def plan(i):
        k = KINDS4[(i + i // 4) % 4]
        return _kind_place(k, view[0]), _kind_place(k, view[1])

    _check(WIDE_8, VIEW_KINDS * 2 + ("busy", "flat"), 4, plan, lambda j: chain)


def test_source_of_one_kind_and_denoised_of_another():
    def plan(i):
        return _kind_place(KINDS4[i % 4], ALIGNED[0]), _kind_place(KINDS4[(i + 1 + i // 4) % 4], ALIGNED[1])

    _check(WIDE_8, VIEW_KINDS * 2 + ("busy",), 4, plan, lambda j: "wide")


# ---- 2e. the natural stride that is not 16-aligned ----------------------------------------------------------------------------

@pytest.mark.parametrize("where,chain", [("dev", "stream"), ("host", "wide")])
def test_contiguous_336_wide_runs_stream_from_the_device_and_wide_from_the_host(where, chain):
    """8-bit 4:2:0, 336 wide: the chroma rows of a contiguous tensor are 168 bytes apart, every second one off a 16-byte
    boundary, so the frame runs the stream chain in place; from the host it is staged into 176-byte rows and runs wide."""
    _check(Geom(336, 192, 8, 8, 1, 1, 3), VIEW_KINDS, 3, lambda i: (where, where), lambda j: chain)


# ---- 2f. refusals ---------------------------------------------------------------------------------------------------------------

REFUSALS = {
    "stride_below_row": lambda f, c, row: f.stride_bytes.__setitem__(c, row - 2),
    "odd_stride_16bit": lambda f, c, row: f.stride_bytes.__setitem__(c, row + 17),
    "stride_above_32_bits": lambda f, c, row: f.stride_bytes.__setitem__(c, (1 << 32) + 64),
    "null_plane": lambda f, c, row: f.data.__setitem__(c, None),
    # the smallest even stride that puts the end of the plane's last row (192 luma, 96 chroma rows) 2^32 bytes from its first sample
    "extent_of_4_gib": lambda f, c, row: f.stride_bytes.__setitem__(c, (-(-((1 << 32) - row) // ((96 if c else 192) - 1)) + 1) & ~1),
}
REFUSAL_TEXT = {"extent_of_4_gib": "the plane's extent (row stride x (rows - 1) + a row) is 4 GiB or more"}


@pytest.mark.parametrize("on_device", [1, 0], ids=["device", "host"])
@pytest.mark.parametrize("side,c", [(0, 0), (0, 2), (1, 0), (1, 1)], ids=["src_Y", "src_Cr", "den_Y", "den_Cb"])
@pytest.mark.parametrize("what", list(REFUSALS))
def test_diff_frame_refuses_a_bad_plane_pointer_or_stride(what, side, c, on_device):
    """g1s_diff_frame answers G1S_ERR_INVALID and names frame and plane, before anything is copied or queued (the refused
    frame never reaches a kernel); the error stays (a job that lost a frame has no table)."""
    from grav1synth_amd import _lib
    from grav1synth_amd.diff import Frame

    geom = Geom(320, 192, 10, 10, 1, 1, 3)
    frames, _, _ = _job(geom, ("flat", "flat"))
    s, d = frames[0]
    keep = []
    if on_device:
        s, d = [contiguous(p) for p in s], [contiguous(p) for p in d]
    fs, fd = Frame(s, 1, 1).to_c(keep), Frame(d, 1, 1).to_c(keep)
    row = (320 >> (1 if c else 0)) * 2
    REFUSALS[what]((fs, fd)[side], c, row)
    L = _lib.lib()
    g = _generator(geom, 2)
    try:
        assert L.g1s_diff_frame(g._h, C.byref(fs), C.byref(fd)) == -1  # G1S_ERR_INVALID
        msg = L.g1s_diff_last_error(g._h).decode()
        assert msg == f"{SIDES[side]} frame, plane {c}: " + REFUSAL_TEXT.get(what, "bad plane pointer or row stride")
        assert g.stats().frames == 0
        fs2, fd2 = Frame(s, 1, 1).to_c(keep), Frame(d, 1, 1).to_c(keep)
        assert L.g1s_diff_frame(g._h, C.byref(fs2), C.byref(fd2)) == -1, "the refusal is sticky"
    finally:
        g.close()



def test_luma_only_generator_does_not_judge_the_chroma_planes_it_never_reads():
    """A luma-only generator takes three-plane frames and reads plane 0: null chroma pointers are none of its business."""
    from grav1synth_amd import _lib
    from grav1synth_amd.diff import Frame, format_tbl

    geom = Geom(320, 192, 8, 8, 1, 1, 3, False)
    frames, _, want = _job(geom, ("distinct", "damaged", "clamped"))
    L = _lib.lib()
    g = _generator(geom, 2)
    keep = []
    try:
        for s, d in frames:
            vs, _ = device_view(s[0], pitch_bytes=336, base_offset_bytes=0, seed=1)
            vd, _ = device_view(d[0], pitch_bytes=352, base_offset_bytes=16, seed=2)
            fs, fd = Frame([vs] * 3, 1, 1).to_c(keep), Frame([vd] * 3, 1, 1).to_c(keep)
            for f in (fs, fd):
                f.data[1] = f.data[2] = None
                f.stride_bytes[1] = f.stride_bytes[2] = 0
            assert L.g1s_diff_frame(g._h, C.byref(fs), C.byref(fd)) == 0, L.g1s_diff_last_error(g._h).decode()
        assert format_tbl(g.finish()) == want
    finally:
        g.close()


# ---- 3. estimate ------------------------------------------------------------------------------------------------------------------

EST_OFFSETS = (0, 2, 4, 8, 12)          # the 16-, 4- and 8-byte tiers of the word loader, and the slowest one
EST_PITCHES = (("+", 0), ("+", 16), ("+", 6))


@pytest.mark.parametrize("mode", ["default", "wide"])
@pytest.mark.parametrize("bd", [8, 10, 16])
@pytest.mark.parametrize("w", [320, 322])
def test_estimator_reads_views_of_every_load_tier(monkeypatch, w, bd, mode):
    """Fifteen frames of different content in one estimator, one for every base offset and pitch: `fast` with a pitch above the
    row (offset 0, row + 16, W = 320), the three tiers of the word loader by address, a pitch that moves the tier from row to row
    (row + 6).  The margin is hostile (maximum code value in the first frame); the input buffers stay as they were."""
    from grav1synth_amd.estimate import NoiseEstimator
    from tests.content import make_frames
    from tests.oracle_binding import estimate_plane_noise

    if mode == "wide":
        monkeypatch.setenv("G1S_ESTIMATE", "wide")
    else:
        monkeypatch.delenv("G1S_ESTIMATE", raising=False)
    est = NoiseEstimator(bd, batch_frames=4)
    want, keep, what = [], [], []
    try:
        for k, (off, rule) in enumerate((o, r) for o in EST_OFFSETS for r in EST_PITCHES):
            p = make_frames(("distinct", "clamped", "busy")[k % 3], w, 72, bd, 1, 1, k)[0][0]
            row = w * p.dtype.itemsize
            v, guard = device_view(p, pitch_bytes=At(rule).pitch(row), base_offset_bytes=off, fill="max" if k == 0 else "random",
                                   max_code=(1 << bd) - 1, seed=k)
            want.append(estimate_plane_noise(p, bd))
            keep.append((v, guard))
            what.append(f"frame {k}: base + {off}, pitch {At(rule).pitch(row)} for a row of {row}")
            est.estimate_frame(v)
        got = est.finish()
    finally:
        est.close()
    assert any(x is not None and x > 0 for x in want)
    bad = [f"{what[k]}: {got[k]} vs {want[k]}" for k in range(len(want)) if got[k] != want[k]]
    assert len(got) == len(want) and not bad, "\n".join(bad)
    for k, (_, guard) in enumerate(keep):
        guard.assert_unchanged(what[k])


# ---- 3. render ----------------------------------------------------------------------------------------------------------------------

def _io_views(planes, bd, ins: Sequence[At], outs: Sequence[At], seed: int):
    """Input views of the planes and output views of the same shapes (fill 0xA5 bytes inside and outside)."""
    vin, vout, gin, gout = [], [], [], []
    for c, p in enumerate(planes):
        row = p.shape[1] * p.dtype.itemsize
        v, g = device_view(p, pitch_bytes=ins[c].pitch(row), base_offset_bytes=ins[c].off, fill=ins[c].fill, max_code=(1 << bd) - 1,
                           seed=seed + c)
        vin.append(v), gin.append(g)
        blank = np.full(p.shape, 0xA5 if p.dtype == np.uint8 else 0xA5A5, p.dtype)
        v, g = device_view(blank, pitch_bytes=outs[c].pitch(row), base_offset_bytes=outs[c].off, fill=int(blank[0, 0]), seed=seed + c)
        vout.append(v), gout.append(g)
    return vin, vout, gin, gout


def _render_layouts(bd: int):
    """name -> (luma in, chroma in, luma out, chroma out).  grain.hip: `vec` of a plane wants its in and out bases and strides
    on 8 * BPS bytes; `vec_luma` of a chroma plane wants the input luma on 16 bytes when chroma is subsampled across, on 8 * BPS
    otherwise.  `m`: a misaligned offset for this sample size."""
    m, a = (3, At(("^", 256))) if bd == 8 else (6, At(("^", 256), 64))
    out = {
        "all aligned, pitch 256-aligned and above the row (vec, vec_luma)": (a, a, a, a),
        "luma in off, chroma aligned (chroma vec, not vec_luma)": (At(("+", 16), m), a, a, a),
        "luma aligned, chroma in off (vec_luma, chroma not vec)": (a, At(("+", 32), m), a, At(("+", 16))),
        "everything off (neither)": (At(("+", 16), m), At(("+", 16), m + 2), At(("+", 32), m + 4), At(("+", 16), m + 6)),
        "in aligned, out off (vec_luma, not vec)": (a, a, At(("+", 16), m), At(("+", 48), m + 2)),
        "in off, out aligned (neither)": (At(("+", 16), m), At(("+", 16), m), a, a),
        "in and out of different aligned pitch (vec, vec_luma)": (At(("+", 16)), At(("+", 48)), At(("^", 256), 128), At(("+", 32), 16)),
    }
    if bd == 8:  # the 8-byte rule of the 8-bit instance: luma on 8 bytes is `vec` and, under 4:2:0, not `vec_luma`
        out["luma 8 bytes off, strides 8 mod 16 (vec; vec_luma only without subsampling)"] = (At(("+", 8), 8), At(("+", 8), 8), At(("+", 8), 8),
                                                                                          At(("+", 24), 8))
    return out


@pytest.mark.parametrize("w,h", [(322, 194), (320, 192)])
@pytest.mark.parametrize("ss", ["420", "444"])
@pytest.mark.parametrize("bd", [8, 10])
def test_render_on_views_of_every_vec_and_vec_luma_combination(bd, ss, w, h):
    from grav1synth_amd.grain import GrainSynthesizer
    from tests import grain_ref as R
    from tests.test_gpu_grain import assert_planes_equal, content, make_segment

    subx, suby = {"420": (1, 1), "444": (0, 0)}[ss]
    seg = make_segment(3, 21 + bd)
    planes = content(w, h, bd, subx, suby, seed=3)
    want = R.add_noise(planes, seg, bd, subx, suby)
    syn = GrainSynthesizer(bd)
    try:
        for n, (name, (li, ci, lo, co)) in enumerate(_render_layouts(bd).items()):
            fill = "max" if n == 0 else "random"
            vin, vout, gin, gout = _io_views(planes, bd, [li._replace(fill=fill)] + [ci._replace(fill=fill)] * 2, [lo, co, co], 10 * n)
            got = syn.apply(vin, seg, subx, suby, out=vout)
            assert_planes_equal(got, want, name)
            for c in range(3):
                gin[c].assert_unchanged(f"{name}: input plane {c}")
                gout[c].assert_margin_intact(f"{name}: output plane {c}")
    finally:
        syn.close()


# ---- 3. denoise ---------------------------------------------------------------------------------------------------------------------

DENOISE_LAYOUTS = {
    # bd, in (luma, chroma), out (luma, chroma)
    "8-bit, odd bases": (8, (At(("+", 13), 3), At(("+", 7), 5)), (At(("+", 9), 7), At(("+", 11), 1))),
    "16-bit samples, aligned pitch above the row": (10, (At(("^", 256)), At(("^", 256), 64)), (At(("^", 256), 128), At(("^", 256)))),
    "16-bit samples, in and out of different pitch": (10, (At(("+", 16)), At(("+", 6), 2)), (At(("+", 64), 32), At(("+", 22), 10))),
}


@pytest.mark.parametrize("w,h", [(131, 97), (208, 136)])
@pytest.mark.parametrize("name", list(DENOISE_LAYOUTS))
def test_denoise_on_views_with_tile_edges_under_a_pitch(name, w, h):
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise import gradient, reference
    from tests.test_gpu_grain import assert_planes_equal

    bd, (li, ci), (lo, co) = DENOISE_LAYOUTS[name]
    planes = gradient(w, h, bd, 1, 1, seed=7)
    want = reference(planes, bd)
    dn = Denoiser(bd)
    try:
        for fill in ("random", "max"):
            vin, vout, gin, gout = _io_views(planes, bd, [li._replace(fill=fill)] + [ci._replace(fill=fill)] * 2, [lo, co, co], 5)
            got = dn.apply(vin, 1, 1, out=vout)
            assert_planes_equal(got, want, f"{name}, margin {fill}")
            for c in range(3):
                gin[c].assert_unchanged(f"{name}: input plane {c}")
                gout[c].assert_margin_intact(f"{name}: output plane {c}")
    finally:
        dn.close()


# ---- 3. resize --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tw,th", [(480, 304), (200, 120)], ids=["up", "down"])
def test_resize_of_a_device_view(tw, th):
    """10-bit 4:2:0, 320 x 200 in views off a 16-byte boundary under a pitch: through FilterChain.apply, and through
    g1s_resize_frame_to_host with the views' own pointers and strides (the resize kernels read them in place)."""
    from grav1synth_amd import _lib
    from grav1synth_amd.diff import Frame
    from grav1synth_amd.filters import FilterChain
    from tests.content import make_frames
    from tests.oracle_binding import resize_planes

    bd, alg = 10, "lanczos"
    planes = make_frames("distinct", 320, 200, bd, 1, 1, 0)[0]
    want = resize_planes(planes, 1, 1, tw, th, bd, alg)
    vin, _, gin, _ = _io_views(planes, bd, [At(("+", 22), 6), At(("^", 256), 2), At(("+", 16), 0, "max")], [At()] * 3, 3)
    frame = Frame(vin, 1, 1)
    got = FilterChain(f"resize:width={tw},height={th},alg={alg}").apply(frame, bd).planes
    for c in range(3):
        assert np.array_equal(got[c], want[c]), f"FilterChain.apply: plane {c}"
    keep = []
    fr = frame.to_c(keep)
    assert fr.on_device == 1 and fr.stride_bytes[0] == 320 * 2 + 22
    outs = [np.zeros_like(p) for p in want]
    ptrs = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
    strides = (C.c_size_t * 3)(*[o.strides[0] for o in outs])
    err = C.create_string_buffer(256)
    rc = _lib.lib().g1s_resize_frame_to_host(alg.encode(), C.byref(fr), bd, tw, th, -1, ptrs, strides, err, len(err))
    assert rc == 0, err.value.decode()
    for c in range(3):
        assert np.array_equal(outs[c], want[c]), f"in place: plane {c}"
        gin[c].assert_unchanged(f"input plane {c}")
