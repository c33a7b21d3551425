"""`grav1synth estimate` on an MI355X: av1_grain::estimate_plane_noise per frame (N4; /root/reference/src/main.rs:534-608).

>>> est = NoiseEstimator(10)
>>> est.estimate_frame(y_plane)                 # numpy / torch (host or cuda), u8 or u16; only the luma plane is read
>>> estimates = est.finish()                    # List[Optional[float]]: None where the reference has None
>>> open(out, "wb").write(format_estimates(estimates))     # "filmgrn1" + one "{:.3}" line per frame (-1 for None)

Noise levels (include/g1s_diff.h, rules N1 - N8): the same stencil summed per intensity bin and per plane, and what a
clip's record says about the clip -- the curve of a grain prior and the strength, for `Denoiser`.

>>> meter = NoiseLevelMeter(10)
>>> meter.frame([y, u, v], xdec=1, ydec=1)      # numpy arrays or torch tensors, as GrainMeter.measure takes them
>>> total = noise_levels_sum(meter.finish())    # numpy structured array, one entry a frame: n, a, q (3 x 32)
>>> fwd, inv = noise_prior(total, 10)           # rules N5 - N6 and the curve of rules 12 - 13
>>> h_luma, h_chroma = auto_strength(total, 10) # rule N7
>>> Denoiser(10, curve=(fwd, inv), strength=h_luma, chroma_strength=h_chroma or 0.0)

Temporal noise levels (rules T1 - T8): the same from the difference of consecutive frames where the picture stands still,
which holds on spatially correlated grain; motion reads as noise.

>>> meter = NoiseLevelMeter(10, temporal=True)
>>> for f in frames: meter.frame(f)             # meter.cut() where a scene ends
>>> ttotal = noise_levels_sum_temporal(meter.finish_temporal())   # one record a frame with a predecessor: n, s, q
>>> fwd, inv = noise_prior(ttotal, 10, temporal=True)
>>> h_luma, h_chroma = auto_strength(ttotal, 10, temporal=True)
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._frame_op import FrameOp
from ._lib import G1SError, G1SNlfLRecord, G1SNlfOpts, G1SNlfRecord, G1SNlfTRecord
from .diff import Frame

# g1s_nlf_record_t
NLF_RECORD = np.dtype([("n", "<u8", (3, 32)), ("a", "<u8", (3, 32)), ("q", "<u8", (3, 32))])
assert NLF_RECORD.itemsize == C.sizeof(G1SNlfRecord)
# g1s_nlf_trecord_t
NLF_TRECORD = np.dtype([("n", "<u8", (3, 32)), ("s", "<i8", (3, 32)), ("q", "<u8", (3, 32))])
assert NLF_TRECORD.itemsize == C.sizeof(G1SNlfTRecord)
# g1s_nlf_lrecord_t
NLF_LRECORD = np.dtype([("n", "<u8", (3, 46)), ("r", "<i8", (3, 46)), ("s", "<i8", (3,)), ("xn", "<u8", (2, 25)), ("xr", "<i8", (2, 25)), ("ln", "<u8"),
                        ("ls", "<i8"), ("l2", "<u8")])
assert NLF_LRECORD.itemsize == C.sizeof(G1SNlfLRecord)

log = logging.getLogger("grav1synth")


class NoiseEstimator:
    def __init__(self, bit_depth: int, *, device: int = -1, batch_frames: int = 0):
        self._L = _lib.lib()
        self._h = self._L.g1s_estimate_new(bit_depth, device, batch_frames)
        if not self._h:
            raise G1SError(-5, "g1s_estimate_new failed: no HIP device (the estimator has no CPU fallback) or bit depth outside 8..16")
        self._keep: list = []

    def _check(self, rc: int) -> None:
        if rc:
            raise G1SError(rc, self._L.g1s_estimate_last_error(self._h).decode())

    def estimate_frame(self, y_plane) -> None:
        keep: list = []
        f = Frame([y_plane], 1, 1).to_c(keep)
        if f.on_device == 1:
            import torch
            torch.cuda.current_stream().synchronize()
            self._keep.extend(keep)
        elif f.on_device == 2:
            f.on_device = 0  # (pinned or not: this entry point copies before it returns)
        self._check(self._L.g1s_estimate_frame(self._h, C.byref(f)))

    def finish(self) -> List[Optional[float]]:
        n = C.c_size_t()
        cap = 4096
        buf = (C.c_double * cap)()
        rc = self._L.g1s_estimate_finish(self._h, buf, cap, C.byref(n))
        if rc == _lib.G1S_ERR_CAPACITY:
            cap = n.value
            buf = (C.c_double * cap)()
            rc = self._L.g1s_estimate_finish(self._h, buf, cap, C.byref(n))
        self._check(rc)
        self._keep.clear()
        return [None if buf[i] == -1.0 else float(buf[i]) for i in range(n.value)]

    def kernel_time(self, enable: bool = True):
        """(milliseconds, frames) of the kernel launches so far (HIP events); enables / disables the timing."""
        ms, fr = C.c_double(), C.c_uint64()
        self._L.g1s_estimate_set_timing(self._h, int(enable), C.byref(ms), C.byref(fr))
        return ms.value, fr.value

    def last_launch(self) -> dict:
        """g1s_estimate_last_launch (a test and measurement aid): strip_rows, row_strips, packed, launched, cus and wgs_per_cu
        of the last batch's launch, and `sums`: (accum, count) of every frame finish() has an estimate for, in its order."""
        info, n = _lib.G1SEstimateLaunch(), C.c_size_t()
        self._check(self._L.g1s_estimate_last_launch(self._h, C.byref(info), None, 0, C.byref(n)))
        buf = (C.c_uint64 * max(2 * n.value, 1))()
        self._check(self._L.g1s_estimate_last_launch(self._h, None, buf, n.value, C.byref(n)))
        out = {name: int(getattr(info, name)) for name, _ in info._fields_}
        out["packed"], out["launched"] = bool(info.packed), bool(info.launched)
        out["sums"] = [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n.value)]
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.g1s_estimate_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_estimates(estimates) -> bytes:
    """The command's output file (src/main.rs:596-603)."""
    L = _lib.lib()
    n = len(estimates)
    arr = (C.c_double * max(n, 1))(*[-1.0 if e is None else float(e) for e in estimates])
    buf = C.create_string_buffer(16 + 32 * n)
    w = L.g1s_format_estimates(arr, n, buf, len(buf))
    if w < 0:
        raise G1SError(int(w), "g1s_format_estimates failed")
    return buf.raw[:w]


TABLE_NEEDS_TWO_FRAMES = "a table needs two frames"


def estimate_y4m_file(source: str, output: str, *, device: int = -1, levels: Optional[str] = None, levels_temporal: Optional[str] = None,
                      table: Optional[str] = None, table_lag: int = 3, max_frames: int = 0, min_count: int = 0, lags: Optional[str] = None) -> int:
    """`grav1synth estimate SOURCE -o OUTPUT [--levels PATH] [--levels-temporal PATH]` for a .y4m input: with `levels` the
    noise-level report of the clip is written there, with `levels_temporal` its temporal report (the file one run), from the
    same read of the clip.  With `table` the clip's own grain table (rules L1 - L10: the file one run, made from its first
    max_frames frames, 0 = all) is written there as a .tbl and with `lags` the lag report of those frames; the two level
    reports stay those of the whole clip.  A refusal of the table (G1SError; fewer than two frames: TABLE_NEEDS_TWO_FRAMES) is
    raised before anything is written.  Returns the number of frames."""
    from .ingest import Y4MReader

    rd = Y4MReader(source)
    d = rd.details
    est = NoiseEstimator(d.bit_depth, device=device)
    temporal = levels_temporal is not None or table is not None
    lag_kw = dict(lags=True) if table is not None else {}  # (a job without --table makes the calls it made)
    meter = NoiseLevelMeter(d.bit_depth, device=device, temporal=temporal, **lag_kw) if levels is not None or temporal else None
    total, ttotal, ltotal = np.zeros((), NLF_RECORD), np.zeros((), NLF_TRECORD), np.zeros((), NLF_LRECORD)
    first = None  # the first frame's record: the one frame without a predecessor
    pairs = 0
    reports = levels is not None or levels_temporal is not None  # (they are of the whole clip, whatever the table is made from)
    table_sums = None  # (ttotal, ltotal, pairs) of the table's frames: the first max_frames, or all

    def take():
        nonlocal total, ttotal, ltotal, first, pairs
        recs = meter.finish()
        if first is None and len(recs):
            first = recs[0].copy()
        total = noise_levels_sum(np.concatenate([total.reshape(1), recs]))
        if temporal:
            trecs = meter.finish_temporal()
            pairs += len(trecs)
            ttotal = noise_levels_sum_temporal(np.concatenate([ttotal.reshape(1), trecs]))
        if table is not None:
            lrecs = meter.finish_lags()
            if table_sums is None:  # (behind the table's frames the lag records are not wanted)
                ltotal = noise_lags_sum(np.concatenate([ltotal.reshape(1), lrecs]))

    n = metered = 0
    try:
        while True:
            planes = rd.get_frame()
            if planes is None:
                break
            est.estimate_frame(planes[0])
            if meter is not None and (table_sums is None or reports):
                meter.frame(planes, d.xdec, d.ydec)
                metered += 1
                if table is not None and max_frames and metered == max_frames:  # the table's frames are in: its sums as they stand
                    take()
                    table_sums = (ttotal.copy(), ltotal.copy(), pairs)
                elif (n + 1) % 32 == 0:
                    take()
            n += 1
        segment = None
        if table is not None:  # (before anything is written: a refusal writes nothing)
            if table_sums is None:
                take()
                table_sums = (ttotal.copy(), ltotal.copy(), pairs)
            if min(metered, max_frames or metered) < 2:
                raise G1SError(-1, TABLE_NEEDS_TWO_FRAMES)  # G1S_ERR_INVALID
            segment = noise_table(table_sums[0], table_sums[1], d.bit_depth, d.xdec, d.ydec, d.nplanes, table_lag, min_count)
            lag_report = None if lags is None else format_noise_lags(table_sums[1], table_sums[2], d.bit_depth, d.nplanes, table_lag, min_count)
        with open(output, "wb") as f:
            f.write(format_estimates(est.finish()))
        if meter is not None:
            take()
            if levels is not None:
                with open(levels, "wb") as f:
                    f.write(format_noise_levels(total, n, d.bit_depth, d.nplanes))
            if segment is not None:
                from .diff import write_tbl

                write_tbl(table, [segment])
                if lags is not None:
                    with open(lags, "wb") as f:
                        f.write(lag_report)
            if levels_temporal is not None:
                later = total.copy()
                if first is not None:
                    for name in ("n", "a", "q"):
                        later[name] -= first[name]
                with open(levels_temporal, "wb") as f:
                    f.write(format_noise_levels_temporal(ttotal, pairs, d.bit_depth, d.nplanes, ordinary=later))
    finally:
        if meter is not None:
            meter.close()
        est.close()
        rd.close()
    return n


def format_noise_lags(lags_total: np.ndarray, pairs: int, bit_depth: int, nplanes: int = 3, lag: int = 3, min_count: int = 0) -> bytes:
    """Rule L10: the report of a clip's lag record (g1s_format_noise_lags; host only; the grammar is in include/g1s_diff.h)."""
    L = _lib.lib()
    record = np.ascontiguousarray(lags_total, NLF_LRECORD)
    buf = C.create_string_buffer(1 << 14)
    w = L.g1s_format_noise_lags(record.ctypes.data, pairs, bit_depth, nplanes, lag, min_count, buf, len(buf))
    if w < 0:
        raise G1SError(int(w), "g1s_format_noise_lags failed")
    return buf.raw[:w]


def noise_table_y4m_file(source: str, table: Optional[str] = None, *, levels: Optional[str] = None, levels_temporal: Optional[str] = None,
                         lags: Optional[str] = None, device: int = -1, batch_frames: int = 0, max_frames: int = 0, lag: int = 3, min_count: int = 0):
    """The clip's own grain table from the first max_frames frames (0 = all) of a .y4m file, the file one run
    (g1s_nlf_y4m_file_table): the .tbl into `table`, and where they are given the noise levels, the temporal noise levels and
    the lag report of those frames.  A refusal raises and writes nothing.  Returns (frames, the GrainTableSegment)."""
    from ._lib import G1SSegment
    from .diff import GrainTableSegment

    enc = lambda p: None if p is None else str(p).encode()  # noqa: E731
    opts = G1SNlfOpts(C.sizeof(G1SNlfOpts), device, batch_frames)
    err = C.create_string_buffer(512)
    seg = G1SSegment()
    n = _lib.lib().g1s_nlf_y4m_file_table(enc(source), enc(table), enc(levels), enc(levels_temporal), enc(lags), C.byref(opts), max_frames, lag, min_count,
                                          C.byref(seg), err, len(err))
    if n < 0:
        raise G1SError(int(n), err.value.decode())
    return int(n), GrainTableSegment.from_c(seg)


class NoiseLevelMeter(FrameOp):
    """g1s_nlf_*: the noise level function of frames on the device (rules N1 - N4); no CPU fallback.  temporal = True: a
    temporal meter (rules T1 - T5): the same records from finish(), and from finish_temporal() one record per frame with a
    predecessor in its run; cut() ends a run.  lags = True: a lag meter (rules L1 - L5): a temporal meter that also keeps a
    lag record a pair, from finish_lags()."""
    _name = "nlf"

    def __init__(self, bit_depth: int, *, device: int = -1, batch_frames: int = 0, temporal: bool = False, lags: bool = False):
        self._L = _lib.lib()
        self.bit_depth = bit_depth
        self.temporal = temporal or lags
        self.lags = lags
        opts = G1SNlfOpts(C.sizeof(G1SNlfOpts), device, batch_frames)
        new = self._L.g1s_nlf_new_lags if lags else self._L.g1s_nlf_new_temporal if temporal else self._L.g1s_nlf_new
        self._h = new(bit_depth, C.byref(opts))
        if not self._h:
            raise G1SError(-5, self._L.g1s_last_global_error().decode())
        self._keep: list = []  # planes the queued kernels still read

    def frame(self, planes: Sequence, xdec: int = 1, ydec: int = 1, *, async_host: bool = False) -> None:
        """Queues one frame ([y] or [y, u, v]); its record comes with finish().  Host planes are copied before the call
        returns; async_host = True queues the copies of pinned torch tensors instead: they must stay as they are until
        finish()."""
        planes = list(planes)
        if not hasattr(planes[0], "is_cuda"):
            planes = [np.asarray(p) for p in planes]
        keep: list = [planes]
        pinned = async_host and hasattr(planes[0], "is_pinned") and not planes[0].is_cuda and planes[0].is_pinned()
        f = Frame(planes, xdec, ydec, async_host=pinned).to_c(keep)
        if f.on_device == 1:
            import torch

            torch.cuda.current_stream().synchronize()  # (the planes were produced on torch's stream)
        self._keep.append(keep)
        self._check(self._L.g1s_nlf_frame(self._h, C.byref(f)))

    def _finish(self, call, dtype, cap: Optional[int]) -> np.ndarray:
        n = C.c_size_t()
        if cap is None:
            rc = call(self._h, None, 0, C.byref(n))
            if rc not in (0, _lib.G1S_ERR_CAPACITY):
                self._check(rc)
            cap = n.value
        out = np.zeros(max(cap, 1), dtype)
        rc = call(self._h, out.ctypes.data, cap, C.byref(n))
        if rc == _lib.G1S_ERR_CAPACITY:
            raise G1SError(rc, f"{n.value} records do not fit {cap}")
        self._check(rc)
        self._keep.clear()
        return out[:n.value]

    def finish(self, cap: Optional[int] = None) -> np.ndarray:
        """Launches what is queued, waits, and returns the records since the last finish(), one a frame, in order.  cap:
        the size of the buffer handed to the library (a test aid; too small raises G1S_ERR_CAPACITY and loses nothing)."""
        return self._finish(self._L.g1s_nlf_finish, NLF_RECORD, cap)

    def cut(self) -> None:
        """Ends the run of a temporal meter: the next frame has no predecessor.  Waits for nothing."""
        self._check(self._L.g1s_nlf_cut(self._h))

    def finish_temporal(self, cap: Optional[int] = None) -> np.ndarray:
        """finish() for the temporal records: one per frame with a predecessor since the last finish_temporal(), in order.  A
        meter made without temporal = True refuses."""
        return self._finish(self._L.g1s_nlf_finish_temporal, NLF_TRECORD, cap)

    def finish_lags(self, cap: Optional[int] = None) -> np.ndarray:
        """finish() for the lag records (NLF_LRECORD): one per frame with a predecessor since the last finish_lags(), in
        order.  A meter made without lags = True refuses."""
        return self._finish(self._L.g1s_nlf_finish_lags, NLF_LRECORD, cap)

    def kernel_times_lags(self) -> Tuple[float, float, int]:
        """(ms in the luma lag launches, ms in the chroma lag launches, pairs) of the batches kernel_times() had timed."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint64()
        self._L.g1s_nlf_lag_times(self._h, C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value

    def kernel_times_temporal(self) -> Tuple[float, float, int]:
        """(ms in the temporal luma launches, ms in the temporal chroma launches, pairs) of the batches kernel_times() had
        timed (HIP events)."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint64()
        self._L.g1s_nlf_temporal_times(self._h, C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value

    def kernel_times(self, enable: bool = True) -> Tuple[float, float, int]:
        """(ms in the luma launches, ms in the chroma launches, frames) of the timed batches so far (HIP events)."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint64()
        self._L.g1s_nlf_set_timing(self._h, int(enable), C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value


def _sum_records(call, dtype, records: np.ndarray) -> np.ndarray:
    records = np.ascontiguousarray(records, dtype).reshape(-1)
    total = np.zeros((), dtype)
    rc = call(records.ctypes.data if records.size else None, records.size, total.ctypes.data)
    if rc:
        raise G1SError(rc, "the clip's sums leave 64 bits")
    return total


def noise_levels_sum(records: np.ndarray) -> np.ndarray:
    """Rule N4: a clip's record from its frames' (g1s_nlf_sum; host only).  An overflow raises."""
    return _sum_records(_lib.lib().g1s_nlf_sum, NLF_RECORD, records)


def noise_levels_sum_temporal(records: np.ndarray) -> np.ndarray:
    """Rule T5: a clip's temporal record from its pairs' (g1s_nlf_sum_temporal; host only).  An overflow raises."""
    return _sum_records(_lib.lib().g1s_nlf_sum_temporal, NLF_TRECORD, records)


def noise_lags_sum(records: np.ndarray) -> np.ndarray:
    """Rule L5: a clip's lag record from its pairs' (g1s_nlf_sum_lags; host only).  An overflow raises."""
    return _sum_records(_lib.lib().g1s_nlf_sum_lags, NLF_LRECORD, records)


def noise_ar(lags_total: np.ndarray, plane: int, bit_depth: int, xdec: int = 1, ydec: int = 1, lag: int = 3, min_count: int = 0) -> Tuple[np.ndarray, float]:
    """Rules L6 - L7: (the AR coefficients of a plane before quantisation -- 2 lag (lag + 1) of them, on a chroma plane the luma
    coefficient behind them --, the fold's gain) from a clip's lag record (g1s_nlf_ar; host only).  A refusal raises."""
    L = _lib.lib()
    record = np.ascontiguousarray(lags_total, NLF_LRECORD)
    x, gain = (C.c_double * 25)(), C.c_double()
    rc = L.g1s_nlf_ar(record.ctypes.data, plane, bit_depth, xdec, ydec, lag, min_count, x, C.byref(gain))
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    n = 2 * lag * (lag + 1) + (1 if plane else 0)
    return np.array(x[:n], np.float64), gain.value


def noise_table(ttotal: np.ndarray, lags_total: np.ndarray, bit_depth: int, xdec: int = 1, ydec: int = 1, nplanes: int = 3, lag: int = 3, min_count: int = 0):
    """Rules L6 - L9: a GrainTableSegment from a clip's temporal record and its lag record (g1s_nlf_table; host only): the
    clip's own grain table, no denoiser involved.  A refusal raises."""
    from ._lib import G1SSegment
    from .diff import GrainTableSegment

    L = _lib.lib()
    t, l = np.ascontiguousarray(ttotal, NLF_TRECORD), np.ascontiguousarray(lags_total, NLF_LRECORD)
    out = G1SSegment()
    rc = L.g1s_nlf_table(t.ctypes.data, l.ctypes.data, bit_depth, xdec, ydec, nplanes, lag, min_count, C.byref(out))
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    return GrainTableSegment.from_c(out)


def noise_sigma(record: np.ndarray, bit_depth: int, min_count: int = 0, *, temporal: bool = False) -> np.ndarray:
    """Rules N5 - N6: the scaling function s[1 << bit_depth] of a clip's record (g1s_nlf_sigma; host only).  temporal: of a
    clip's temporal record (rules T6 - T7), here and in the four below."""
    L = _lib.lib()
    record = np.ascontiguousarray(record, NLF_TRECORD if temporal else NLF_RECORD)
    s = np.zeros(1 << min(max(bit_depth, 0), 16), np.uint8)
    rc = (L.g1s_nlf_sigma_temporal if temporal else L.g1s_nlf_sigma)(record.ctypes.data, bit_depth, min_count, s.ctypes.data)
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    return s


def noise_prior(record: np.ndarray, bit_depth: int, range: int = 0, min_count: int = 0, *, temporal: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(fwd, inv): the variance-stabilising curve of a clip's record, rules N5 - N6 then rules 12 - 13 of `denoise`, as
    Denoiser(curve=...) takes it (host only)."""
    L = _lib.lib()
    s = noise_sigma(record, bit_depth, min_count, temporal=temporal)
    fwd, inv = np.zeros(1 << bit_depth, np.uint16), np.zeros(4096, np.uint16)
    rc = L.g1s_denoise_curve_sigma(s.ctypes.data, bit_depth, range, fwd.ctypes.data, inv.ctypes.data)
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    return fwd, inv


def noise_chroma_sigma(record: np.ndarray, min_count: int = 0, *, temporal: bool = False) -> np.ndarray:
    """Rule N9: the chroma scaling function s[256] over the luma under it, from the two chroma planes of a clip's record
    pooled (g1s_nlf_chroma_sigma; host only).  The same for every bit depth."""
    L = _lib.lib()
    record = np.ascontiguousarray(record, NLF_TRECORD if temporal else NLF_RECORD)
    s = np.zeros(256, np.uint8)
    rc = (L.g1s_nlf_chroma_sigma_temporal if temporal else L.g1s_nlf_chroma_sigma)(record.ctypes.data, min_count, s.ctypes.data)
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    return s


def noise_chroma_prior(record: np.ndarray, range: int = 0, min_count: int = 0, *, temporal: bool = False) -> np.ndarray:
    """m[256]: the chroma gain of a clip's record, rule N9 then rule 21 of `denoise`, as Denoiser(chroma_gain=...) takes it
    (host only)."""
    L = _lib.lib()
    s = noise_chroma_sigma(record, min_count, temporal=temporal)
    gain = np.zeros(256, np.uint16)
    rc = L.g1s_denoise_chroma_gain_sigma(s.ctypes.data, range & 0xFFFFFFFF, gain.ctypes.data)
    if rc:
        raise G1SError(rc, L.g1s_last_global_error().decode())
    return gain


def auto_strength(record: np.ndarray, bit_depth: int, min_count: int = 0, *, temporal: bool = False) -> Tuple[float, Optional[float]]:
    """Rule N7: (h_luma, h_chroma) in 8-bit code values; h_chroma is None where the rule refuses (a luma-only clip); a
    refusal for luma raises (host only)."""
    L = _lib.lib()
    record = np.ascontiguousarray(record, NLF_TRECORD if temporal else NLF_RECORD)
    strength = L.g1s_nlf_strength_temporal if temporal else L.g1s_nlf_strength
    h = C.c_double()
    if strength(record.ctypes.data, bit_depth, min_count, 0, C.byref(h)):
        raise G1SError(-1, L.g1s_last_global_error().decode())
    h_luma = h.value
    h_chroma = None if strength(record.ctypes.data, bit_depth, min_count, 1, C.byref(h)) else h.value
    return h_luma, h_chroma


def format_noise_levels(total: np.ndarray, frames: int, bit_depth: int, nplanes: int = 3, min_count: int = 0, cap: int = 1 << 16) -> bytes:
    """The report of a clip's record (g1s_format_noise_levels; host only).  cap: the size of the buffer handed to the
    library (a test aid)."""
    total = np.ascontiguousarray(total, NLF_RECORD)
    buf = C.create_string_buffer(max(cap, 1))
    w = _lib.lib().g1s_format_noise_levels(total.ctypes.data, frames, bit_depth, nplanes, min_count, buf, cap)
    if w < 0:
        raise G1SError(int(w), "g1s_format_noise_levels failed")
    return buf.raw[:w]


def format_noise_levels_temporal(total: np.ndarray, pairs: int, bit_depth: int, nplanes: int = 3, min_count: int = 0, *,
                                 ordinary: Optional[np.ndarray] = None, cap: int = 1 << 16) -> bytes:
    """The report of a clip's temporal record (g1s_format_noise_levels_temporal; host only).  ordinary: the ordinary record
    of the frames with a predecessor, for the ratio lines ("-" without it).  cap: a test aid."""
    total = np.ascontiguousarray(total, NLF_TRECORD)
    if ordinary is not None:
        ordinary = np.ascontiguousarray(ordinary, NLF_RECORD)
    buf = C.create_string_buffer(max(cap, 1))
    w = _lib.lib().g1s_format_noise_levels_temporal(total.ctypes.data, None if ordinary is None else ordinary.ctypes.data, pairs, bit_depth, nplanes,
                                                    min_count, buf, cap)
    if w < 0:
        raise G1SError(int(w), "g1s_format_noise_levels_temporal failed")
    return buf.raw[:w]


def noise_levels_y4m_file(source: str, output: Optional[str] = None, *, device: int = -1, batch_frames: int = 0,
                          max_frames: int = 0, temporal_report=None):
    """The noise levels of the first max_frames frames (0 = all) of a .y4m file (g1s_nlf_y4m_file): the report into
    `output` when it is given.  Returns (frames, the clip's record).  temporal_report: a path, or True for no file: the
    meter is a temporal one (g1s_nlf_y4m_file_temporal), the temporal report goes there, and the clip's temporal record is
    returned as a third value."""
    opts = G1SNlfOpts(C.sizeof(G1SNlfOpts), device, batch_frames)
    err = C.create_string_buffer(512)
    total = np.zeros((), NLF_RECORD)
    if temporal_report is not None:
        ttotal = np.zeros((), NLF_TRECORD)
        n = _lib.lib().g1s_nlf_y4m_file_temporal(str(source).encode(), None if output is None else str(output).encode(),
                                                 None if temporal_report is True else str(temporal_report).encode(), C.byref(opts), max_frames,
                                                 total.ctypes.data, ttotal.ctypes.data, err, len(err))
        if n < 0:
            raise G1SError(int(n), err.value.decode())
        return int(n), total, ttotal
    n = _lib.lib().g1s_nlf_y4m_file(str(source).encode(), None if output is None else str(output).encode(), C.byref(opts), max_frames,
                                    total.ctypes.data, err, len(err))
    if n < 0:
        raise G1SError(int(n), err.value.decode())
    return int(n), total
