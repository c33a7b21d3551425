"""Frames at the limits of what the kernels can address, against the references, bit for bit or refused -- whichever
include/g1s_diff.h documents for the size; no test accepts either.

A. Extreme aspect ratios: a frame at a stated limit in one direction and tiny in the other, for every operation.
   `diff`: 131 072 samples a side (4 096 blocks: the last value of the 12-bit fields the unit lists pack a block's column and
   row into) is right, 131 072 + 32 / + 33 is refused; 130 944 wide and 131 040 high are the largest frames the wide chain
   takes (g1s_diff::wide_ok) and run it.  The content puts flat blocks in the last two block columns and rows and textured
   ones next to them, and every case asserts that from the oracle's mask.
B. Plane extents past 2^31 and 2^32 bytes: a 256 x 160 plane as a device view with a pitch of 2^24 or 2^25 bytes
   (tests/views.py far_view).  `diff` runs the stream chain from 2^31 bytes and refuses from 2^32; the frame operations
   widen to 64 bits before row * stride and must be right at both.

`diff` under G1S_K3=stream runs in a child (`python -m tests.test_gpu_limits NAME ...`), as tests/sweep_worker.py does: the
library reads the switch once per process.  A case that needs more device memory than is free skips with both numbers;
nothing else skips."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import oracle_shadow, record_mismatches
from tests.views import contiguous, far_view

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = Fraction(24, 1)
MARK = "LIMITS-WORKER-RESULT "
CHAIN_KERNEL = {"wide": "k3w_pass", "stream": "k3s_fused"}
GIB = 1 << 30


def _need(nbytes: int) -> None:
    import torch

    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    if free < nbytes + GIB:
        pytest.skip(f"the case needs {nbytes + GIB} bytes of device memory, {free} are free")


# ---- A. diff ----------------------------------------------------------------------------------------------------------------

# name -> (width, height, 4:2:0 chroma planes?, the chain the default build runs)
DIFF_LIMITS = {
    "131072x64_luma": (131072, 64, False, "stream"),
    "131072x96_420": (131072, 96, True, "stream"),
    "64x131072_luma": (64, 131072, False, "stream"),
    "96x131072_420": (96, 131072, True, "stream"),
    "130944x64_luma_widest_of_the_wide_chain": (130944, 64, False, "wide"),
    "130944x64_420_widest_of_the_wide_chain": (130944, 64, True, "wide"),
    "64x131040_luma_tallest_of_the_wide_chain": (64, 131040, False, "wide"),
    "64x131040_420_tallest_of_the_wide_chain": (64, 131040, True, "wide"),
}
LAG = 1


def limit_frame(w: int, h: int, chroma: bool, frame: int = 0):
    """(source planes, denoised planes, textured[by, bx]): the flat synthetic pair with a checker laid over the luma of two blocks
    in five -- never over the last two block columns and rows, always over the third from last."""
    from grav1synth_amd.synth import SynthSpec, make_pair

    s, d = make_pair(SynthSpec(w, h, 8, textured=False, nplanes=3 if chroma else 1), frame)
    s, d = [p.numpy().copy() for p in s], [p.numpy().copy() for p in d]
    nbw, nbh = (w + 31) // 32, (h + 31) // 32
    by, bx = np.arange(nbh)[:, None], np.arange(nbw)[None, :]
    tex = (bx + 3 * by) % 5 >= 3
    if nbw > 4:
        tex[:, nbw - 3], tex[:, nbw - 2:] = True, False
    if nbh > 4:
        tex[nbh - 3, :nbw - 2 if nbw > 4 else nbw], tex[nbh - 2:, :] = True, False
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    checker = ((((xs >> 3) + (ys >> 3)) & 1) * 48 - 24) + ((xs & 1) * 8)
    on = np.repeat(np.repeat(tex, 32, 0), 32, 1)[:h, :w]
    for p in (s, d):
        p[0] = np.clip(p[0].astype(np.int64) + on * checker, 0, 255).astype(np.uint8)
    return s, d, tex


def limit_job(name: str):
    """The one-frame job of a DIFF_LIMITS case: planes, the oracle's shadow and table, and the assertion that the case cannot
    pass by having nothing to compute at the far edge."""
    from tests.oracle_binding import OracleDiff, format_tbl as oracle_tbl

    w, h, chroma, _chain = DIFF_LIMITS[name]
    s, d, tex = limit_frame(w, h, chroma)
    o = OracleDiff(FPS.numerator, FPS.denominator, 8, 8, LAG, chroma)
    o.diff_frame(s, d, 1, 1)
    shadow = oracle_shadow(o, len(s))
    tbl = oracle_tbl(o.finish())
    o.close()
    mask = shadow["mask"] != 0
    nbh, nbw = mask.shape
    assert (nbw, nbh) == ((w + 31) // 32, (h + 31) // 32)
    # Flat is the oracle's word, and its threshold moves with the frame's scores: of the blocks without the checker a few in a
    # hundred miss it (also in the last two columns / rows, so `all` cannot be asked there); a block with the checker never passes.
    assert not mask[tex].any() and mask[~tex].mean() > 0.9 and 0.3 < tex.mean() < 0.5
    last = {131072: 4095, 130944: 4091, 131040: 4094}[max(w, h)]  # the largest value the case puts into the packed field
    edge = mask[:, nbw - 2:] if w > h else mask[nbh - 2:, :]
    before = mask[:, nbw - 3] if w > h else mask[nbh - 3, :]
    assert (nbw if w > h else nbh) - 1 == last
    assert edge[:, 1].any() if w > h else edge[1, :].any(), f"{name}: a flat block in block column / row {last}"
    assert edge.mean() >= 0.5 and not before.any(), f"{name}: most blocks of the last two block columns / rows flat, none in the third from last"
    return s, d, shadow, tbl


def _generator(chroma: bool, batch: int, records_only=False, lag: int = LAG):
    from grav1synth_amd.diff import DiffGenerator

    return DiffGenerator(FPS, 8, 8, ar_coeff_lag=lag, luma_only=not chroma, batch_frames=batch, records_only=records_only)


def _chains(chroma: bool, pairs, lag: int = LAG) -> set:
    """The chains a timed generator runs on these frames as one batch (kernel_times)."""
    g = _generator(chroma, len(pairs), records_only=True, lag=lag)
    try:
        g.set_timing(True)
        for fs, fd in pairs:
            g.diff_frame(fs, fd)
        g.sync()
        names = set(g.kernel_times())
    finally:
        g.close()
    return {c for c, k in CHAIN_KERNEL.items() if any(n.startswith(k) for n in names)}


def diff_mismatches(w, h, chroma, pairs, shadows, want_tbl, chain, lag: int = LAG) -> list:
    """The chain that ran, every frame's record and the table's bytes for `pairs` of Frames in one batch: what differs."""
    from grav1synth_amd.diff import Record, format_tbl

    out = []
    ran = _chains(chroma, pairs, lag)
    if ran != {chain}:
        out.append(f"meant for the {chain} chain, ran {sorted(ran)}")
    g = _generator(chroma, len(pairs), records_only=True, lag=lag)
    try:
        for fs, fd in pairs:
            g.diff_frame(fs, fd)
        recs, n = g.take_records(w, h, 3 if chroma else 1, len(pairs))
    finally:
        g.close()
    if n != len(pairs):
        return out + [f"{n} records for {len(pairs)} frames"]
    for i in range(n):
        out.extend(record_mismatches(shadows[i], Record(recs[i]), f"frame {i} [{chain}]"))
    g = _generator(chroma, len(pairs), lag=lag)
    try:
        for fs, fd in pairs:
            g.diff_frame(fs, fd)
        got = format_tbl(g.finish())
    finally:
        g.close()
    if got != want_tbl:
        out.append(f".tbl differs ({len(got)} bytes for {len(want_tbl)})")
    return out


def run_diff_limit(name: str, chain: str) -> list:
    from grav1synth_amd.diff import Frame

    w, h, chroma, _c = DIFF_LIMITS[name]
    s, d, shadow, tbl = limit_job(name)
    pair = (Frame([contiguous(p) for p in s], 1, 1), Frame([contiguous(p) for p in d], 1, 1))
    return diff_mismatches(w, h, chroma, [pair], [shadow], tbl, chain)


def _stream_child(kind: str, names) -> dict:
    """name -> what differs, from a child that starts with G1S_K3=stream."""
    import ast

    env = dict(os.environ, G1S_K3="stream")
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_limits", kind] + list(names), capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    marks = [line[len(MARK):] for line in p.stdout.splitlines() if line.startswith(MARK)]
    assert p.returncode == 0 and len(marks) == 1, f"the G1S_K3=stream child ended with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    return ast.literal_eval(marks[0])


@pytest.mark.parametrize("name", list(DIFF_LIMITS))
def test_diff_at_the_size_limit_equals_the_oracle(name):
    bad = run_diff_limit(name, DIFF_LIMITS[name][3])
    assert not bad, f"{len(bad)} things differ:\n" + "\n".join(bad[:40])


def test_diff_at_the_size_limit_on_the_stream_chain_equals_the_oracle():
    """The same frames under G1S_K3=stream: the four at the limit again, and the four the wide chain would take."""
    got = _stream_child("size", list(DIFF_LIMITS))
    assert set(got) == set(DIFF_LIMITS)
    bad = [f"{name}: {line}" for name, lines in got.items() for line in lines]
    assert not bad, f"{len(bad)} things differ:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("name", ["131072x64_luma", "64x131072_luma"])
def test_device_half_of_the_fold_at_the_size_limit_gives_the_host_halfs_bytes(name, monkeypatch):
    """8 192 blocks a frame, a wide and a tall one: k4_latest's latest states against the host half's, byte for byte."""
    from tests.test_gpu_sweep import _latest_mismatches

    w, h, chroma, _c = DIFF_LIMITS[name]
    assert ((w + 31) // 32) * ((h + 31) // 32) >= 4096
    feed = []
    for k in range(2):
        s, d, _tex = limit_frame(w, h, chroma, k)
        feed.append(([contiguous(p) for p in s], [contiguous(p) for p in d]))
    try:
        bad = _latest_mismatches(dict(src_bd=8, den_bd=8), feed, 1, 1, dict(ar_coeff_lag=LAG, luma_only=True, batch_frames=2), monkeypatch)
    finally:
        monkeypatch.delenv("G1S_LATEST", raising=False)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("on_device", [1, 0], ids=["device", "host"])
@pytest.mark.parametrize("w,h", [(131072 + 32, 64), (131072 + 33, 64), (131073, 64), (64, 131072 + 32), (64, 131073), (131073, 131073)])
def test_diff_refuses_a_frame_beyond_131072_samples_a_side(w, h, on_device):
    """G1S_ERR_INVALID from the call that was handed the frame, the limit named, nothing copied or queued, sticky.  (The
    planes behind the pointers are one row long: a refused frame is never read.)"""
    from grav1synth_amd import _lib
    from grav1synth_amd.diff import Frame

    rowbuf = np.zeros((1, max(w, h)), np.uint8)
    t = contiguous(rowbuf) if on_device else rowbuf
    keep = []
    L = _lib.lib()
    g = _generator(False, 2)
    try:
        frames = []
        for _side in range(2):
            f = Frame([t], 1, 1).to_c(keep)
            f.width, f.height = w, h
            f.stride_bytes[0] = w
            frames.append(f)
        assert L.g1s_diff_frame(g._h, C.byref(frames[0]), C.byref(frames[1])) == -1  # G1S_ERR_INVALID
        assert L.g1s_diff_last_error(g._h).decode() == f"frame of {w} x {h} samples: diff takes at most 131072 x 131072"
        assert g.stats().frames == 0
        ok = [Frame([contiguous(np.zeros((64, 64), np.uint8))], 1, 1).to_c(keep) for _ in range(2)]
        assert L.g1s_diff_frame(g._h, C.byref(ok[0]), C.byref(ok[1])) == -1, "the refusal is sticky"
    finally:
        g.close()


# ---- B. diff on planes whose last row is gigabytes from the first ------------------------------------------------------------

FAR_W, FAR_H = 256, 160
# name -> (pitch, base offset, the boundary the plane's last row lies beyond, the outcome)
FAR_PITCHES = {
    "2^24": (1 << 24, 0, 1 << 31, "stream"),
    "2^24+16_base48": ((1 << 24) + 16, 48, 1 << 31, "stream"),
    "2^25": (1 << 25, 0, 1 << 32, "refused"),
    "2^25+48_base48": ((1 << 25) + 48, 48, 1 << 32, "refused"),
}
FAR_SIDES = {"source": (True, False), "denoised": (False, True), "both": (True, True)}


def _far_planes(planes, pitch, off, boundary, bd=8, seed=0, chroma_pitch=None):
    """Far views of `planes`, the luma plane asserted to have its last row beyond `boundary` bytes from its first sample.
    Chroma planes lie under chroma_pitch, by default half the luma pitch (with half the rows: a quarter of the extent)."""
    views, guards = [], []
    for c, p in enumerate(planes):
        pc = pitch if c == 0 else chroma_pitch or (pitch // 2 + 15) & ~15
        v, g = far_view(p, pitch_bytes=pc, base_offset_bytes=off, max_code=(1 << bd) - 1, seed=seed + c)
        last_row = v[p.shape[0] - 1:].data_ptr() - v.data_ptr()
        assert last_row == pc * (p.shape[0] - 1)
        if c == 0 or chroma_pitch:
            assert last_row + p.shape[1] * p.dtype.itemsize > boundary, f"plane {c}: the last row ends {last_row} bytes from the first sample"
        views.append(v), guards.append(g)
    return views, guards


def far_job(chroma: bool, h: int = FAR_H):
    from tests.test_gpu_records import Geom, _job

    geom = Geom(FAR_W, h, 8, 8, 1, 1, 2, chroma)
    return geom, _job(geom, ("distinct", "damaged"))


def run_diff_views(geom, job, plan, what: str) -> list:
    """Two frames in one batch, the first contiguous, the planes of the second placed by plan(side, c) -> None (contiguous) or
    (pitch, base offset, the boundary its last row lies beyond): the whole batch runs the stream chain; records and table
    against the oracle; the far buffers unchanged."""
    import torch

    from grav1synth_amd.diff import Frame

    frames, shadows, want_tbl = job
    pairs, guards = [], []
    for i, (s, d) in enumerate(frames):
        fr = []
        for side, planes in enumerate((s, d)):
            v = []
            for c, p in enumerate(planes):
                at = plan(side, c) if i == 1 else None
                if at is None:
                    v.append(contiguous(p))
                    continue
                pitch, off, boundary = at
                view, g = far_view(p, pitch_bytes=pitch, base_offset_bytes=off, max_code=255, seed=10 * side + c)
                end = view[p.shape[0] - 1:].data_ptr() - view.data_ptr() + p.shape[1]
                assert end == pitch * (p.shape[0] - 1) + p.shape[1] > boundary, f"side {side} plane {c}: the last row ends {end} bytes from the first sample"
                v.append(view), guards.append(g)
            fr.append(Frame(v, 1, 1))
        pairs.append(tuple(fr))
    out = [f"{what}: {line}" for line in diff_mismatches(geom.w, geom.h, geom.chroma, pairs, shadows, want_tbl, "stream", geom.lag)]
    for k, guard in enumerate(guards):
        guard.assert_unchanged(f"{what}: far plane {k}")
    del pairs, guards
    torch.cuda.empty_cache()
    return out


def run_diff_far(pitch_name: str, side_name: str, chroma: bool) -> list:
    """The second frame's planes of the side(s) named under the pitch named, chroma planes under half of it."""
    pitch, off, boundary, outcome = FAR_PITCHES[pitch_name]
    assert outcome == "stream"
    geom, job = far_job(chroma)

    def plan(side, c):
        if not FAR_SIDES[side_name][side]:
            return None
        return (pitch, off, boundary) if c == 0 else ((pitch // 2 + 15) & ~15, off, boundary // 4)

    return run_diff_views(geom, job, plan, f"{pitch_name}, {side_name}")


FAR_RIGHT = [(p, s, ch) for p in ("2^24", "2^24+16_base48") for s in FAR_SIDES for ch in (True, False) if ch or s == "both"]


@pytest.mark.parametrize("pitch_name,side_name,chroma", FAR_RIGHT, ids=[f"{p}-{s}-{'420' if c else 'luma'}" for p, s, c in FAR_RIGHT])
def test_diff_on_planes_of_2_gib_or_more_runs_the_stream_chain_and_equals_the_oracle(pitch_name, side_name, chroma):
    pitch = FAR_PITCHES[pitch_name][0]
    _need((2 if side_name == "both" else 1) * (2 if chroma else 1) * pitch * FAR_H)
    bad = run_diff_far(pitch_name, side_name, chroma)
    assert not bad, f"{len(bad)} things differ:\n" + "\n".join(bad[:40])


def test_diff_on_planes_of_2_gib_or_more_under_the_stream_switch_equals_the_oracle():
    _need(2 * 2 * FAR_H << 24)
    names = [f"{p}|{s}|{int(c)}" for p, s, c in FAR_RIGHT if s == "both" or p == "2^24"]
    got = _stream_child("far", names)
    assert set(got) == set(names)
    bad = [f"{name}: {line}" for name, lines in got.items() for line in lines]
    assert not bad, f"{len(bad)} things differ:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("side,c", [(0, 1), (1, 2)], ids=["source_Cb", "denoised_Cr"])
def test_diff_with_one_chroma_plane_of_2_gib_or_more(side, c):
    """4:2:0, every plane tight but one chroma plane of the second frame: 128 x 80 under a pitch of 2^25 + 16, its last row 2.5 GiB
    from its first.  The chroma plane alone takes the batch to the stream chain."""
    pitch = (1 << 25) + 16
    _need(pitch * FAR_H // 2)
    geom, job = far_job(True)
    bad = run_diff_views(geom, job, lambda sd, pc: (pitch, 16, 1 << 31) if (sd, pc) == (side, c) else None, f"plane {c} of side {side}")
    assert not bad, f"{len(bad)} things differ:\n" + "\n".join(bad[:40])


MAX_STRIDE = 0xffffffff // 36  # csrc/frame_op.h kDiffMaxStride: 36 tile rows of it fit 32 bits


@pytest.mark.parametrize("side_name", list(FAR_SIDES))
def test_diff_under_the_largest_stride_it_takes(side_name):
    """256 x 32 luma (one block row: every tile has rows below the plane) under a pitch of 119 304 640 bytes, the largest multiple
    of 16 that 36 tile rows of keep inside 32 bits: 3.4 GiB from the first row to the last, the stream chain, right."""
    pitch = MAX_STRIDE & ~15
    assert 36 * pitch < 1 << 32
    _need((2 if side_name == "both" else 1) * pitch * 32)
    geom, job = far_job(False, 32)
    bad = run_diff_views(geom, job, lambda sd, pc: (pitch, 0, 1 << 31) if FAR_SIDES[side_name][sd] else None, f"pitch {pitch}, {side_name}")
    assert not bad, f"{len(bad)} things differ:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("side", [0, 1], ids=["source", "denoised"])
def test_diff_refuses_a_stride_of_2_to_the_27(side):
    """256 x 32 under a pitch of 2^27: the extent is below 4 GiB (31 x 2^27 + 256), 36 tile rows of the pitch are not.  A real view
    of 4 GiB: refused by the call that was handed it, the plane and the bound named, sticky, the buffer untouched."""
    from grav1synth_amd import _lib
    from grav1synth_amd.diff import Frame

    pitch = 1 << 27
    assert pitch * 31 + 256 < 1 << 32 <= 36 * pitch
    _need(pitch * 32)
    _geom, (frames, _shadows, _tbl) = far_job(False, 32)
    s, d = frames[0]
    far, guards = _far_planes((d if side else s), pitch, 0, 1 << 31)
    near = [contiguous(p) for p in (s if side else d)]
    keep = []
    fs, fd = Frame(near if side else far, 1, 1).to_c(keep), Frame(far if side else near, 1, 1).to_c(keep)
    L = _lib.lib()
    g = _generator(False, 2, lag=2)
    try:
        assert L.g1s_diff_frame(g._h, C.byref(fs), C.byref(fd)) == -1
        want = f"{('source', 'denoised')[side]} frame, plane 0: a row stride above 119304647 bytes (36 rows of it leave 32 bits)"
        assert L.g1s_diff_last_error(g._h).decode() == want
        assert g.stats().frames == 0
        ok = [Frame([contiguous(p) for p in x], 1, 1).to_c(keep) for x in (s, d)]
        assert L.g1s_diff_frame(g._h, C.byref(ok[0]), C.byref(ok[1])) == -1, "the refusal is sticky"
    finally:
        g.close()
    guards[0].assert_unchanged("the refused plane")


def test_the_same_frames_contiguous_run_the_wide_chain():
    """The control of the routing: nothing but the extent moves the batch."""
    from grav1synth_amd.diff import Frame

    geom, (frames, _shadows, _tbl) = far_job(True)
    pairs = [(Frame([contiguous(p) for p in s], 1, 1), Frame([contiguous(p) for p in d], 1, 1)) for s, d in frames]
    assert _chains(True, pairs, geom.lag) == {"wide"}


@pytest.mark.parametrize("side", [0, 1], ids=["source", "denoised"])
@pytest.mark.parametrize("pitch_name", ["2^25", "2^25+48_base48"])
def test_diff_refuses_a_device_plane_of_4_gib_or_more(pitch_name, side):
    """A real view of 5 GiB (luma only): refused by the call that was handed it, plane and limit named, sticky, the buffer
    untouched."""
    from grav1synth_amd import _lib
    from grav1synth_amd.diff import Frame

    pitch, off, boundary, outcome = FAR_PITCHES[pitch_name]
    assert outcome == "refused"
    _need(pitch * FAR_H)
    geom, (frames, _shadows, _tbl) = far_job(False)
    s, d = frames[0]
    far, guards = _far_planes((d if side else s), pitch, off, boundary)
    near = [contiguous(p) for p in (s if side else d)]
    keep = []
    fs, fd = Frame(near if side else far, 1, 1).to_c(keep), Frame(far if side else near, 1, 1).to_c(keep)
    L = _lib.lib()
    g = _generator(False, 2)
    try:
        assert L.g1s_diff_frame(g._h, C.byref(fs), C.byref(fd)) == -1
        want = f"{('source', 'denoised')[side]} frame, plane 0: the plane's extent (row stride x (rows - 1) + a row) is 4 GiB or more"
        assert L.g1s_diff_last_error(g._h).decode() == want
        assert g.stats().frames == 0
        ok = [Frame([contiguous(p) for p in x], 1, 1).to_c(keep) for x in (s, d)]
        assert L.g1s_diff_frame(g._h, C.byref(ok[0]), C.byref(ok[1])) == -1, "the refusal is sticky"
    finally:
        g.close()
    guards[0].assert_unchanged("the refused plane")


# ---- A. the frame operations at their stated sizes ---------------------------------------------------------------------------

def edge_planes(w, h, bd, subx, suby, mono=False, seed=0):
    """Gradient with noise (tests/test_gpu_denoise.gradient) whose last 64 columns and 48 rows carry a pattern of their own."""
    from tests.test_gpu_denoise import gradient

    planes = gradient(w, h, bd, subx, suby, seed=seed, mono=mono)
    top = (1 << bd) - 1
    for c, p in enumerate(planes):
        ph, pw = p.shape
        ys, xs = np.arange(ph)[:, None], np.arange(pw)[None, :]
        far = (xs >= pw - min(64, pw // 2)) | (ys >= ph - min(48, ph // 2))
        mark = ((xs * 7 + ys * 13 + 31 * c) % 61) << max(bd - 8, 0)
        p[...] = np.where(far, np.clip(top // 2 + mark - (30 << max(bd - 8, 0)), 0, top), p).astype(p.dtype)
    return planes


FRAME_LIMIT_SHAPES = [(65536, 8), (8, 65536)]


@pytest.mark.parametrize("w,h", FRAME_LIMIT_SHAPES)
@pytest.mark.parametrize("bd,ss", [(8, "420"), (12, "mono")])
def test_denoise_at_65536_samples_a_side(w, h, bd, ss):
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise import reference
    from tests.test_gpu_grain import _to_dev, assert_planes_equal

    planes = edge_planes(w, h, bd, 1, 1, mono=ss == "mono", seed=3)
    dn = Denoiser(bd)
    try:
        got = dn.apply(_to_dev(planes, bd), 1, 1)
    finally:
        dn.close()
    assert_planes_equal(got, reference(planes, bd), f"{w}x{h} {bd} bit {ss}")


@pytest.mark.parametrize("w,h", FRAME_LIMIT_SHAPES)
@pytest.mark.parametrize("bd,ss", [(8, "420"), (12, "mono")])
def test_temporal_denoise_at_65536_samples_a_side(w, h, bd, ss):
    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise_temporal import assert_clips_equal, reference
    from tests.test_gpu_grain import _to_dev

    frames = [edge_planes(w, h, bd, 1, 1, mono=ss == "mono", seed=10 + t) for t in range(3)]
    dn = Denoiser(bd, temporal_radius=1)
    try:
        got = dn.denoise_clip([_to_dev(f, bd) for f in frames], 1, 1)
    finally:
        dn.close()
    assert_clips_equal(got, reference(frames, bd, 1), f"{w}x{h} {bd} bit {ss}, temporal radius 1")


@pytest.mark.parametrize("w,h", [(65537, 8), (8, 65537)])
@pytest.mark.parametrize("op", ["denoise", "measure"])
def test_denoise_and_measure_refuse_65537(op, w, h):
    from grav1synth_amd import _lib
    from grav1synth_amd.denoise import Denoiser
    from grav1synth_amd.measure import GrainMeter
    from tests.test_gpu_grain import _to_dev

    planes = _to_dev([np.zeros((h, w), np.uint16)], 10)
    obj = Denoiser(10) if op == "denoise" else GrainMeter(10)
    try:
        with pytest.raises(_lib.G1SError) as e:
            obj.apply(planes, 1, 1) if op == "denoise" else obj.measure(planes, planes, 1, 1)
        assert e.value.code == -1 and "unsupported frame geometry (1 or 3 planes, 4:2:0 / 4:2:2 / 4:4:4, up to 65536 x 65536)" in str(e.value)
    finally:
        obj.close()


@pytest.mark.parametrize("w,h", FRAME_LIMIT_SHAPES)
def test_measure_at_65536_samples_a_side_with_extreme_residuals_at_the_far_edge(w, h):
    """4:2:0 12-bit; the last column (row) of every plane holds residuals of +4095 and -4095 in turn."""
    from grav1synth_amd.measure import GrainMeter
    from tests import measure_ref as R
    from tests.test_gpu_grain import _to_dev

    bd = 12
    clean = edge_planes(w, h, bd, 1, 1, seed=5)
    noisy = [np.clip(p.astype(np.int64) + np.random.default_rng(c).integers(-40, 41, p.shape), 0, 4095).astype(np.uint16) for c, p in enumerate(clean)]
    for n, c in zip(noisy, clean):
        a, b = (n[:, -1], c[:, -1]) if w > h else (n[-1, :], c[-1, :])
        alt = np.arange(a.size) & 1
        a[...], b[...] = np.where(alt, 4095, 0), np.where(alt, 0, 4095)
    want = R.measure_frame(noisy, clean, bd, 1, 1)
    m = GrainMeter(bd)
    try:
        m.measure(_to_dev(noisy, bd), _to_dev(clean, bd), 1, 1)
        got = m.finish()
    finally:
        m.close()
    assert len(got) == 1
    bad = R.mismatches(got[0], want, f"{w}x{h}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("w,h", [(65536, 3), (3, 65536), (131072, 3)])
@pytest.mark.parametrize("bd", [8, 10])
def test_estimate_at_and_beyond_65536_samples_a_side(w, h, bd):
    """The estimator states no size limit of its own (an empty frame is all it refuses): 131 072 x 3 must be right as well."""
    from grav1synth_amd.estimate import NoiseEstimator
    from tests.oracle_binding import estimate_plane_noise

    p = edge_planes(w, h, bd, 1, 1, mono=True, seed=9)[0]
    est = NoiseEstimator(bd)
    try:
        est.estimate_frame(contiguous(p))
        got = est.finish()
    finally:
        est.close()
    assert got == [estimate_plane_noise(p, bd)]


@pytest.mark.parametrize("w,h,ss,bd", [(16384, 4, "420", 8), (16384, 4, "444", 10), (4, 65536, "420", 10), (4, 65536, "444", 8)])
def test_render_at_its_stated_sizes(w, h, ss, bd):
    from grav1synth_amd.grain import GrainSynthesizer
    from tests import grain_ref as R
    from tests.test_gpu_grain import SUBSAMPLINGS, _to_dev, assert_planes_equal, make_segment

    subx, suby = SUBSAMPLINGS[ss]
    seg = make_segment(3, 77 + bd, overlap=True)
    planes = edge_planes(w, h, bd, subx, suby, seed=11)
    syn = GrainSynthesizer(bd)
    try:
        got = syn.apply(_to_dev(planes, bd), seg, subx, suby)
    finally:
        syn.close()
    assert_planes_equal(got, R.add_noise(planes, seg, bd, subx, suby), f"{w}x{h} {ss} {bd} bit")


def test_render_refuses_16385_wide():
    from grav1synth_amd import _lib
    from grav1synth_amd.grain import GrainSynthesizer
    from tests.test_gpu_grain import _to_dev, make_segment

    syn = GrainSynthesizer(8)
    try:
        with pytest.raises(_lib.G1SError) as e:
            syn.apply(_to_dev([np.zeros((4, 16385), np.uint8)], 8), make_segment(), 1, 1)
        assert e.value.code == -1 and "width up to 16384" in str(e.value)
    finally:
        syn.close()


@pytest.mark.parametrize("w,h,tw,th", [(8, 65535, 16, 65535), (2, 65536, 4, 32768), (16, 65536, 8, 65534), (6, 32, 4, 65535), (32, 6, 65535, 4),
                                       (4, 65537, 4, 64), (2, 131072, 2, 65535), (70000, 4, 64, 4)])
def test_resize_at_heights_and_widths_of_65535_and_65536(w, h, tw, th):
    """4:4:4 10-bit; a source of 65 535 and 65 536 rows (one launch row a source row), targets of 65 535 either way; and sources
    of 65 537 and 131 072 rows and of 70 000 columns: the header states no limit for a source and any size is taken."""
    from grav1synth_amd.diff import Frame
    from grav1synth_amd.filters import FilterChain
    from tests.oracle_binding import resize_planes

    bd, alg = 10, "catmullrom"
    planes = edge_planes(w, h, bd, 0, 0, seed=13)
    want = resize_planes(planes, 0, 0, tw, th, bd, alg)
    got = FilterChain(f"resize:width={tw},height={th},alg={alg}").apply(Frame([contiguous(p) for p in planes], 0, 0), bd).planes
    for c in range(3):
        assert np.array_equal(got[c], want[c]), f"plane {c}"


@pytest.mark.parametrize("tw,th", [(65536, 4), (4, 65536)])
def test_resize_to_65536_is_refused_on_the_device_path_as_by_the_parser(tw, th):
    from grav1synth_amd import _lib
    from grav1synth_amd.diff import Frame

    planes = [contiguous(np.zeros((8, 8), np.uint16)) for _ in range(3)]
    keep = []
    fr = Frame(planes, 0, 0).to_c(keep)
    outs = [np.zeros((th, tw), np.uint16) for _ in range(3)]  # (whole planes: a call that is not refused has somewhere to write)
    ptrs = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
    strides = (C.c_size_t * 3)(*[tw * 2] * 3)
    err = C.create_string_buffer(256)
    rc = _lib.lib().g1s_resize_frame_to_host(b"lanczos", C.byref(fr), 10, tw, th, -1, ptrs, strides, err, len(err))
    assert rc == -1 and err.value.decode() == "resize: target larger than 65535 x 65535"


# ---- B. the frame operations on far views ------------------------------------------------------------------------------------

def _blank_far(p, pitch, off, seed):
    blank = np.full(p.shape, 0xA5 if p.dtype == np.uint8 else 0xA5A5, p.dtype)
    return far_view(blank, pitch_bytes=pitch, base_offset_bytes=off, seed=seed)


FAR_IO = [(p, io) for p in FAR_PITCHES for io in ("in", "out", "both")]


def _io(planes, pitch_name, io, bd):
    """(input planes, output planes, input guards, output guards): far views where `io` says so, contiguous tensors elsewhere;
    chroma planes of a far frame lie under half the pitch."""
    import torch

    pitch, off, boundary, _outcome = FAR_PITCHES[pitch_name]
    total = sum((pitch if c == 0 else pitch // 2) * p.shape[0] for c, p in enumerate(planes)) * (2 if io == "both" else 1)
    _need(total)
    gin, gout = [], []
    if io in ("in", "both"):
        vin, gin = _far_planes(planes, pitch, off, boundary, bd)
    else:
        vin = [contiguous(p) for p in planes]
    if io in ("out", "both"):
        vout = []
        for c, p in enumerate(planes):
            v, g = _blank_far(p, pitch if c == 0 else (pitch // 2 + 15) & ~15, off, 50 + c)
            if c == 0:
                assert v[p.shape[0] - 1:].data_ptr() - v.data_ptr() + p.shape[1] * p.dtype.itemsize > boundary
            vout.append(v), gout.append(g)
    else:
        vout = [torch.zeros(p.shape, dtype=v.dtype, device="cuda") for p, v in zip(planes, vin)]
    return vin, vout, gin, gout


def _guards_hold(gin, gout, what):
    for c, g in enumerate(gin):
        g.assert_unchanged(f"{what}: input plane {c}")
    for c, g in enumerate(gout):
        g.assert_margin_intact(f"{what}: output plane {c}")


def _far_frame_planes(bd, pitch_name, seed=0):
    """256 x 160: 4:2:0 under the 2^24 pitches, one plane under the 2^25 ones (two planes of 5 GiB and what goes with them)."""
    mono = FAR_PITCHES[pitch_name][0] >= 1 << 25
    return edge_planes(FAR_W, FAR_H, bd, 1, 1, mono=mono, seed=seed), mono


@pytest.mark.parametrize("pitch_name,io", FAR_IO, ids=[f"{p}-{io}" for p, io in FAR_IO])
def test_denoise_on_far_views(pitch_name, io):
    import torch

    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise import reference
    from tests.test_gpu_grain import assert_planes_equal

    bd = 10
    planes, _mono = _far_frame_planes(bd, pitch_name, seed=21)
    vin, vout, gin, gout = _io(planes, pitch_name, io, bd)
    dn = Denoiser(bd)
    try:
        got = dn.apply(vin, 1, 1, out=vout)
    finally:
        dn.close()
    assert_planes_equal(got, reference(planes, bd), f"{pitch_name} {io}")
    _guards_hold(gin, gout, f"{pitch_name} {io}")
    del vin, vout, gin, gout, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pitch_name", list(FAR_PITCHES))
def test_temporal_denoise_on_far_views_with_far_neighbours(pitch_name):
    """Mono frames, temporal radius 1, every input a far view.  Under the 2^24 pitches (2.5 GiB a plane): three frames, so the
    middle one has a far neighbour on either side, and its output is a far view too (10 GiB).  Under the 2^25 pitches (5 GiB a
    plane): two frames, each the other's neighbour, outputs in ordinary tensors (10 GiB) -- a third input or a far output
    would take the case past 12 GiB, and nothing is freed while the clip is queued; denoise's far outputs under 2^25 are
    test_denoise_on_far_views' business."""
    import torch

    from grav1synth_amd.denoise import Denoiser
    from tests.test_gpu_denoise_temporal import assert_clips_equal, reference

    bd = 8
    pitch, off, boundary, _o = FAR_PITCHES[pitch_name]
    small = pitch < 1 << 25
    nframes = 3 if small else 2
    _need(pitch * FAR_H * (4 if small else 2))
    frames = [edge_planes(FAR_W, FAR_H, bd, 1, 1, mono=True, seed=30 + t) for t in range(nframes)]
    dn = Denoiser(bd, temporal_radius=1)
    gin, gout, outs, keep = [], [], [], []
    try:
        for t, f in enumerate(frames):
            v, g = _far_planes(f, pitch, off, boundary, bd, seed=t)
            gin += g
            keep.append(v)
            if small and t == 1:
                vo, go = _blank_far(f[0], pitch, off, 60 + t)
                gout.append(go)
                outs.append(dn.apply(v, 1, 1, sync=False, out=[vo]))
            else:
                outs.append(dn.apply(v, 1, 1, sync=False))
        dn.sync()
    finally:
        dn.close()
    assert_clips_equal(outs, reference(frames, bd, 1), pitch_name)
    _guards_hold(gin, gout, pitch_name)
    del keep, outs, gin, gout
    torch.cuda.empty_cache()


def test_render_of_420_with_every_input_plane_past_2_gib():
    """4:2:0 8-bit, luma under a pitch of 2^25 (5 GiB) and both chroma planes under the same pitch (80 rows: 2.5 GiB each): the
    co-located luma row of a chroma sample lies up to 5 GiB from the plane's origin.  Outputs in ordinary tensors (10 GiB)."""
    import torch

    from grav1synth_amd.grain import GrainSynthesizer
    from tests import grain_ref as R
    from tests.test_gpu_grain import assert_planes_equal, make_segment

    bd, pitch = 8, 1 << 25
    _need(2 * pitch * FAR_H)
    planes = edge_planes(FAR_W, FAR_H, bd, 1, 1, seed=43)
    seg = make_segment(3, 101)
    vin, gin = _far_planes(planes, pitch, 0, 1 << 31, bd, chroma_pitch=pitch)
    assert vin[0][FAR_H - 1:].data_ptr() - vin[0].data_ptr() > 1 << 32
    syn = GrainSynthesizer(bd)
    try:
        got = syn.apply(vin, seg, 1, 1)
    finally:
        syn.close()
    assert_planes_equal(got, R.add_noise(planes, seg, bd, 1, 1), "4:2:0 under 2^25")
    _guards_hold(gin, [], "4:2:0 under 2^25")
    del vin, gin, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pitch_name,io", FAR_IO, ids=[f"{p}-{io}" for p, io in FAR_IO])
def test_render_on_far_views(pitch_name, io):
    import torch

    from grav1synth_amd.grain import GrainSynthesizer
    from tests import grain_ref as R
    from tests.test_gpu_grain import assert_planes_equal, make_segment

    bd = 8
    planes, _mono = _far_frame_planes(bd, pitch_name, seed=41)
    seg = make_segment(2, 99)
    want = R.add_noise(planes, seg, bd, 1, 1)
    vin, vout, gin, gout = _io(planes, pitch_name, io, bd)
    syn = GrainSynthesizer(bd)
    try:
        got = syn.apply(vin, seg, 1, 1, out=vout)
    finally:
        syn.close()
    assert_planes_equal(got, want, f"{pitch_name} {io}")
    _guards_hold(gin, gout, f"{pitch_name} {io}")
    del vin, vout, gin, gout, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ["noisy", "clean", "both"])
@pytest.mark.parametrize("pitch_name", list(FAR_PITCHES))
def test_measure_on_far_views(pitch_name, which):
    import torch

    from grav1synth_amd.measure import GrainMeter
    from tests import measure_ref as R

    bd = 12
    clean, mono = _far_frame_planes(bd, pitch_name, seed=51)
    noisy = [np.clip(p.astype(np.int64) + np.random.default_rng(c).integers(-300, 301, p.shape), 0, 4095).astype(np.uint16) for c, p in enumerate(clean)]
    want = R.measure_frame(noisy, clean, bd, 1, 1)
    pitch, off, boundary, _o = FAR_PITCHES[pitch_name]
    _need(pitch * FAR_H * (2 if which == "both" else 1) * (1 if mono else 2))
    guards, devs = [], []
    for name, planes in (("noisy", noisy), ("clean", clean)):
        if which in (name, "both"):
            v, g = _far_planes(planes, pitch, off, boundary, bd, seed=len(devs))
            guards += g
        else:
            v = [contiguous(p) for p in planes]
        devs.append(v)
    m = GrainMeter(bd)
    try:
        m.measure(devs[0], devs[1], 1, 1)
        got = m.finish()
    finally:
        m.close()
    bad = R.mismatches(got[0], want, f"{pitch_name} {which}")
    assert len(got) == 1 and not bad, "\n".join(bad)
    _guards_hold(guards, [], f"{pitch_name} {which}")
    del devs, guards
    torch.cuda.empty_cache()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("pitch_name", list(FAR_PITCHES))
def test_estimate_on_a_far_view(pitch_name, bd):
    import torch

    from grav1synth_amd.estimate import NoiseEstimator
    from tests.oracle_binding import estimate_plane_noise

    pitch, off, boundary, _o = FAR_PITCHES[pitch_name]
    _need(pitch * FAR_H)
    p = edge_planes(FAR_W, FAR_H, bd, 1, 1, mono=True, seed=61)[0]
    v, g = _far_planes([p], pitch, off, boundary, bd)
    est = NoiseEstimator(bd)
    try:
        est.estimate_frame(v[0])
        got = est.finish()
    finally:
        est.close()
    assert got == [estimate_plane_noise(p, bd)]
    _guards_hold(g, [], pitch_name)
    del v, g
    torch.cuda.empty_cache()


@pytest.mark.parametrize("tw,th", [(384, 240), (128, 80)], ids=["up", "down"])
@pytest.mark.parametrize("pitch_name", list(FAR_PITCHES))
def test_resize_of_a_far_view(pitch_name, tw, th):
    """The resize entry points write new host planes: the input is the view.  4:2:0 under the 2^24 pitches; under 2^25 the
    chroma planes are contiguous (a frame of three far planes would be 10 GiB)."""
    import torch

    from grav1synth_amd.diff import Frame
    from grav1synth_amd.filters import FilterChain
    from tests.oracle_binding import resize_planes

    bd, alg = 10, "lanczos"
    pitch, off, boundary, _o = FAR_PITCHES[pitch_name]
    planes = edge_planes(FAR_W, FAR_H, bd, 1, 1, seed=71)
    want = resize_planes(planes, 1, 1, tw, th, bd, alg)
    if pitch >= 1 << 25:
        _need(pitch * FAR_H)
        v, g = _far_planes(planes[:1], pitch, off, boundary, bd)
        v += [contiguous(p) for p in planes[1:]]
    else:
        _need(2 * pitch * FAR_H)
        v, g = _far_planes(planes, pitch, off, boundary, bd)
    got = FilterChain(f"resize:width={tw},height={th},alg={alg}").apply(Frame(v, 1, 1), bd).planes
    for c in range(3):
        assert np.array_equal(got[c], want[c]), f"plane {c}"
    _guards_hold(g, [], pitch_name)
    del v, g
    torch.cuda.empty_cache()


# ---- the G1S_K3=stream child -------------------------------------------------------------------------------------------------

def main(argv) -> int:
    kind, names = argv[0], argv[1:]
    out = {}
    for name in names:
        if kind == "size":
            out[name] = run_diff_limit(name, "stream")
        else:
            p, s, c = name.split("|")
            out[name] = run_diff_far(p, s, bool(int(c)))
    print(MARK + repr(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
