"""`measure` and `check`: exact grain statistics of a frame pair on an MI355X -- how well a grain table fits.

HIP kernels behind g1s_measure_* (include/g1s_diff.h, where the statistics are defined: rules 1 - 6); no CPU fallback.
A record holds, per plane, the residual noisy - clean binned by the clean frame's intensity (count, sum, sum of squares
in 32 bins) and its lagged products over the table's causal lag-3 neighbourhood: the two things a grain table describes.

>>> meter = GrainMeter(10)
>>> meter.measure([y, u, v], [cy, cu, cv])      # numpy arrays or torch device tensors, as Denoiser.apply takes them
>>> records = meter.finish()                    # numpy structured array, one entry a pair: n, s1, s2 (3 x 32), r (3 x 25)
>>> text = format_profile(sum_records(records), len(records), 10, width, height)
>>> measure_y4m_files("grainy.y4m", "clean.y4m", "profile.txt")
>>> check_y4m_files("source.y4m", "denoised.y4m", "table.tbl", "fit.txt")   # source - denoised beside rendered - denoised

A temporal meter also says whether the residual is independent from frame to frame (rules 7 - 11): from the second pair of
a run on, every pair has a temporal record against the pair before it.

>>> meter = GrainMeter(10, temporal=True)
>>> for noisy, clean in pairs: meter.measure(noisy, clean)
>>> trecords = meter.finish_temporal()          # one entry a pair but the run's first: n, x, u, v (3 x 32), c (3 x 25)
>>> text = format_temporal_profile(sum_temporal_records(trecords), len(trecords), 10, width, height)
>>> measure_y4m_files("grainy.y4m", "clean.y4m", "profile.txt", temporal_output="temporal.txt")

A cross meter also looks across the planes (rules 12 - 17): the chroma residuals against the luma residual under them, and
against each other.  Every pair has a cross record; the two modes combine.

>>> meter = GrainMeter(10, cross=True)
>>> for noisy, clean in pairs: meter.measure(noisy, clean)
>>> xrecords = meter.finish_cross()             # one entry a pair: n, x, u, v (3 pairings x 32), c (3 pairings x 25)
>>> text = format_cross_profile(sum_cross_records(xrecords), len(xrecords), 10, width, height)
>>> check_y4m_files("source.y4m", "denoised.y4m", "table.tbl", "fit.txt", cross_output="cross.txt")

A scales meter also looks further than 3 samples (rules 18 - 23): the residual summed over aligned 2^k x 2^k boxes, k = 1 .. 5,
binned by the box.  Every pair has a scale record; it combines with the other modes.

>>> meter = GrainMeter(10, scales=True)
>>> for noisy, clean in pairs: meter.measure(noisy, clean)
>>> srecords, records = meter.finish_scales(), meter.finish()   # n, s1, s2 (3 planes x 5 scales x 32 bins)
>>> text = format_scale_profile(sum_records(records), sum_scale_records(srecords), len(records), 10)
>>> check_y4m_files("source.y4m", "denoised.y4m", "table.tbl", "fit.txt", scales_output="scales.txt")
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import G1SError, G1SGrainOpts, G1SMeasureOpts, G1SMeasureRecord, G1SMeasureSRecord, G1SMeasureTRecord, G1SMeasureXRecord
from ._frame_op import FrameOp
from .diff import Frame
from .ingest import UNEQUAL_WARNING

log = logging.getLogger("grav1synth")

# g1s_measure_record_t
RECORD = np.dtype([("n", "<u8", (3, 32)), ("s1", "<i8", (3, 32)), ("s2", "<u8", (3, 32)), ("r", "<i8", (3, 25))])
assert RECORD.itemsize == C.sizeof(G1SMeasureRecord)
# g1s_measure_trecord_t
TRECORD = np.dtype([("n", "<u8", (3, 32)), ("x", "<i8", (3, 32)), ("u", "<u8", (3, 32)), ("v", "<u8", (3, 32)), ("c", "<i8", (3, 25))])
assert TRECORD.itemsize == C.sizeof(G1SMeasureTRecord)
# g1s_measure_xrecord_t: the same fields, the first index the pairing (cb_luma, cr_luma, cb_cr)
XRECORD = np.dtype(TRECORD.descr)
assert XRECORD.itemsize == C.sizeof(G1SMeasureXRecord)
# g1s_measure_srecord_t: [plane][k - 1][bin]
SRECORD = np.dtype([("n", "<u8", (3, 5, 32)), ("s1", "<i8", (3, 5, 32)), ("s2", "<u8", (3, 5, 32))])
assert SRECORD.itemsize == C.sizeof(G1SMeasureSRecord) == 11520


def _opts(device: int, batch_frames: int) -> G1SMeasureOpts:
    return G1SMeasureOpts(C.sizeof(G1SMeasureOpts), device, batch_frames)


class GrainMeter(FrameOp):
    _name = "measure"

    def __init__(self, bit_depth: int, *, device: int = -1, batch_frames: int = 0, temporal: bool = False, cross: bool = False,
                 scales: bool = False):
        self._L = _lib.lib()
        self.bit_depth = bit_depth
        self.temporal = temporal
        self.cross = cross
        self.scales = scales
        opts = _opts(device, batch_frames)
        if scales:
            modes = (_lib.G1S_MEASURE_TEMPORAL if temporal else 0) | (_lib.G1S_MEASURE_CROSS if cross else 0)
            self._h = self._L.g1s_measure_new_scales(bit_depth, C.byref(opts), modes)
        elif cross:
            modes = (_lib.G1S_MEASURE_TEMPORAL if temporal else 0) | _lib.G1S_MEASURE_CROSS
            self._h = self._L.g1s_measure_new_modes(bit_depth, C.byref(opts), modes)
        else:
            self._h = (self._L.g1s_measure_new_temporal if temporal else self._L.g1s_measure_new)(bit_depth, C.byref(opts))
        if not self._h:
            raise G1SError(-5, self._L.g1s_last_global_error().decode())
        self._keep: list = []  # planes the queued kernels still read

    def measure(self, noisy_planes: Sequence, clean_planes: Sequence, xdec: int = 1, ydec: int = 1, *, async_host: bool = False) -> None:
        """Queues one pair (a batch goes out as one launch per plane class); its record comes with finish().  Host planes
        are copied before the call returns; async_host = True queues the copies of pinned torch tensors instead: they
        must stay as they are until finish()."""
        keep: list = []
        pair = []
        for planes in (noisy_planes, clean_planes):
            planes = list(planes)
            if not hasattr(planes[0], "is_cuda"):
                planes = [np.asarray(p) for p in planes]
            keep.append(planes)
            pinned = async_host and hasattr(planes[0], "is_pinned") and not planes[0].is_cuda and planes[0].is_pinned()
            pair.append(Frame(planes, xdec, ydec, async_host=pinned).to_c(keep))
        if pair[0].on_device == 1 or pair[1].on_device == 1:
            import torch

            torch.cuda.current_stream().synchronize()  # (the planes were produced on torch's stream)
        self._keep.append(keep)
        self._check(self._L.g1s_measure_frame(self._h, C.byref(pair[0]), C.byref(pair[1])))

    def finish(self, cap: Optional[int] = None) -> np.ndarray:
        """Launches what is queued, waits, and returns the records since the last finish(), one a pair, in order.  The
        meter can be used again.  cap: the size of the buffer handed to the library (a test aid; too small raises
        G1S_ERR_CAPACITY and loses nothing)."""
        return self._finish(self._L.g1s_measure_finish, RECORD, cap)

    def _finish(self, fn, dtype: np.dtype, cap: Optional[int]) -> np.ndarray:
        """A g1s_measure_finish* call: the size asked for first unless `cap` gives it, then the records."""
        n = C.c_size_t()
        if cap is None:
            rc = fn(self._h, None, 0, C.byref(n))
            if rc not in (0, _lib.G1S_ERR_CAPACITY):
                self._check(rc)
            cap = n.value
        out = np.zeros(max(cap, 1), dtype)
        rc = fn(self._h, out.ctypes.data, cap, C.byref(n))
        if rc == _lib.G1S_ERR_CAPACITY:
            raise G1SError(rc, f"{n.value} records do not fit {cap}")
        self._check(rc)
        self._keep.clear()
        return out[:n.value]

    def cut(self) -> None:
        """Ends the run of a temporal meter: what is queued goes out, and the next pair has no temporal record."""
        self._check(self._L.g1s_measure_cut(self._h))
        self._keep.clear()

    def finish_temporal(self, cap: Optional[int] = None) -> np.ndarray:
        """As finish(), for the temporal records of a temporal meter: one for every pair that has a predecessor in its run,
        in order, since the last finish_temporal().  The ordinary records stay until finish() fetches them."""
        return self._finish(self._L.g1s_measure_finish_temporal, TRECORD, cap)

    def finish_cross(self, cap: Optional[int] = None) -> np.ndarray:
        """As finish(), for the cross records of a cross meter: one for every pair, in order, since the last finish_cross()
        (zeros for a pair with one plane).  The ordinary and the temporal records stay until their own calls fetch them."""
        return self._finish(self._L.g1s_measure_finish_cross, XRECORD, cap)

    def finish_scales(self, cap: Optional[int] = None) -> np.ndarray:
        """As finish(), for the scale records of a scales meter: one for every pair, in order, since the last finish_scales().
        The other records stay until their own calls fetch them."""
        return self._finish(self._L.g1s_measure_finish_scales, SRECORD, cap)

    def scales_kernel_times(self) -> Tuple[float, int]:
        """(ms in km_measure_s and its summing launch, scale records) of the batches kernel_times() had timed."""
        return self._times(self._L.g1s_measure_scales_timing)

    def cross_kernel_times(self) -> Tuple[float, int]:
        """(ms in km_measure_x and its summing launch, cross records) of the batches kernel_times() had timed."""
        return self._times(self._L.g1s_measure_cross_timing)

    def chroma_kernel_times(self) -> Tuple[float, float]:
        """(ms in km_measure's chroma launches, ms in km_measure_t's chroma launches) of the batches kernel_times() had timed."""
        a, b = C.c_double(), C.c_double()
        self._L.g1s_measure_chroma_timing(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def temporal_kernel_times(self) -> Tuple[float, int]:
        """(ms in km_measure_t and km_tail_t, temporal records) of the batches kernel_times() had timed."""
        return self._times(self._L.g1s_measure_temporal_timing)

    def kernel_times(self, enable: bool = True) -> Tuple[float, int]:
        """(ms in km_measure and km_tail, frames) of the timed batches so far (HIP events); enables / disables the timing."""
        return self._times(self._L.g1s_measure_set_timing, int(enable))

    def _times(self, fn, *args) -> Tuple[float, int]:
        """A g1s_measure_*_timing call: (ms, records)."""
        a, n = C.c_double(), C.c_uint64()
        fn(self._h, *args, C.byref(a), C.byref(n))
        return a.value, n.value


def _sum(fn, dtype: np.dtype, records: np.ndarray, what: str) -> np.ndarray:
    """A g1s_measure_sum* call over records of `dtype`; `what`: "", "temporal " ... in the text of an overflow."""
    records = np.ascontiguousarray(records, dtype).reshape(-1)
    total = np.zeros((), dtype)
    rc = fn(records.ctypes.data if records.size else None, records.size, total.ctypes.data)
    if rc:
        raise G1SError(rc, f"the clip's {what}sums leave 64 bits")
    return total


def sum_records(records: np.ndarray) -> np.ndarray:
    """Rule 6: a clip's record from its frames' (g1s_measure_sum; host only).  An overflow raises."""
    return _sum(_lib.lib().g1s_measure_sum, RECORD, records, "")


def format_profile(total: np.ndarray, frames: int, bit_depth: int, width: int, height: int, xdec: int = 1, ydec: int = 1, nplanes: int = 3,
                   synth: Optional[np.ndarray] = None) -> bytes:
    """The report of a clip's record (g1s_format_measure; host only): one value column, or two with `synth`."""
    total = np.ascontiguousarray(total, RECORD)
    synth = None if synth is None else np.ascontiguousarray(synth, RECORD)
    buf = C.create_string_buffer(1 << 16)
    w = _lib.lib().g1s_format_measure(total.ctypes.data, None if synth is None else synth.ctypes.data, frames, bit_depth, width, height, xdec,
                                      ydec, nplanes, buf, len(buf))
    if w < 0:
        raise G1SError(int(w), "g1s_format_measure failed")
    return buf.raw[:w]


def sum_temporal_records(records: np.ndarray) -> np.ndarray:
    """Rule 10: a clip's temporal record from its pairs' (g1s_measure_sum_temporal; host only).  An overflow raises."""
    return _sum(_lib.lib().g1s_measure_sum_temporal, TRECORD, records, "temporal ")


def format_temporal_profile(total: np.ndarray, pairs: int, bit_depth: int, width: int, height: int, xdec: int = 1, ydec: int = 1, nplanes: int = 3,
                            synth: Optional[np.ndarray] = None, cap: int = 1 << 16) -> bytes:
    """The temporal report of a clip's temporal record (g1s_format_measure_temporal; host only): one value column, or two
    with `synth`.  cap: the size of the buffer handed to the library (a test aid)."""
    total = np.ascontiguousarray(total, TRECORD)
    synth = None if synth is None else np.ascontiguousarray(synth, TRECORD)
    buf = C.create_string_buffer(max(cap, 1))
    w = _lib.lib().g1s_format_measure_temporal(total.ctypes.data, None if synth is None else synth.ctypes.data, pairs, bit_depth, width, height,
                                               xdec, ydec, nplanes, buf, cap)
    if w < 0:
        raise G1SError(int(w), "g1s_format_measure_temporal failed")
    return buf.raw[:w]


def sum_cross_records(records: np.ndarray) -> np.ndarray:
    """Rule 16: a clip's cross record from its pairs' (g1s_measure_sum_cross; host only).  An overflow raises."""
    return _sum(_lib.lib().g1s_measure_sum_cross, XRECORD, records, "cross ")


def format_cross_profile(total: np.ndarray, frames: int, bit_depth: int, width: int, height: int, xdec: int = 1, ydec: int = 1,
                         synth: Optional[np.ndarray] = None, cap: int = 1 << 16) -> bytes:
    """The cross report of a clip's cross record (g1s_format_measure_cross; host only): one value column, or two with
    `synth`.  cap: the size of the buffer handed to the library (a test aid)."""
    total = np.ascontiguousarray(total, XRECORD)
    synth = None if synth is None else np.ascontiguousarray(synth, XRECORD)
    buf = C.create_string_buffer(max(cap, 1))
    w = _lib.lib().g1s_format_measure_cross(total.ctypes.data, None if synth is None else synth.ctypes.data, frames, bit_depth, width, height,
                                            xdec, ydec, buf, cap)
    if w < 0:
        raise G1SError(int(w), "g1s_format_measure_cross failed")
    return buf.raw[:w]


def sum_scale_records(records: np.ndarray) -> np.ndarray:
    """Rule 22: a clip's scale record from its pairs' (g1s_measure_sum_scales; host only).  An overflow raises."""
    return _sum(_lib.lib().g1s_measure_sum_scales, SRECORD, records, "scale ")


def format_scale_profile(total: np.ndarray, stotal: np.ndarray, frames: int, bit_depth: int, nplanes: int = 3,
                         synth: Optional[np.ndarray] = None, ssynth: Optional[np.ndarray] = None, cap: int = 1 << 16) -> bytes:
    """The scale report of a clip's plain record and its scale record (g1s_format_measure_scales; host only): one value
    column, or two with `synth` and `ssynth`.  cap: the size of the buffer handed to the library (a test aid)."""
    total, stotal = np.ascontiguousarray(total, RECORD), np.ascontiguousarray(stotal, SRECORD)
    synth = None if synth is None else np.ascontiguousarray(synth, RECORD)
    ssynth = None if ssynth is None else np.ascontiguousarray(ssynth, SRECORD)
    buf = C.create_string_buffer(max(cap, 1))
    w = _lib.lib().g1s_format_measure_scales(total.ctypes.data, stotal.ctypes.data, None if synth is None else synth.ctypes.data,
                                             None if ssynth is None else ssynth.ctypes.data, frames, bit_depth, nplanes, buf, cap)
    if w < 0:
        raise G1SError(int(w), "g1s_format_measure_scales failed")
    return buf.raw[:w]


def _path(p) -> Optional[bytes]:
    return None if p is None else str(p).encode()


def measure_y4m_files(noisy: str, clean: str, output: str, *, device: int = -1, batch_frames: int = 0,
                      temporal_output: Optional[str] = None, cross_output: Optional[str] = None,
                      scales_output: Optional[str] = None) -> Tuple[int, bool]:
    """`measure NOISY CLEAN -o REPORT [--temporal PATH] [--cross PATH] [--scales PATH]` for two .y4m files.  Returns
    (frames, unequal)."""
    opts = _opts(device, batch_frames)
    err = C.create_string_buffer(512)
    unequal = C.c_int(0)
    n = _lib.lib().g1s_measure_y4m_files_scales(str(noisy).encode(), str(clean).encode(), str(output).encode(), _path(temporal_output),
                                                _path(cross_output), _path(scales_output), C.byref(opts), C.byref(unequal), err, len(err))
    if n < 0:
        raise G1SError(int(n), err.value.decode())
    if unequal.value:
        log.warning(UNEQUAL_WARNING)
    log.info("Measured %d frames", n)
    return int(n), bool(unequal.value)


def check_y4m_files(source: str, denoised: str, table: str, output: str, *, device: int = -1, batch_frames: int = 0,
                    clip_to_restricted_range: bool = False, temporal_output: Optional[str] = None,
                    cross_output: Optional[str] = None, scales_output: Optional[str] = None) -> Tuple[int, bool]:
    """`check SOURCE DENOISED -g TABLE -o REPORT [--temporal PATH] [--cross PATH] [--scales PATH]`: source - denoised beside
    render(denoised, table) - denoised.  Returns (frames, unequal)."""
    opts = _opts(device, batch_frames)
    gopts = G1SGrainOpts(C.sizeof(G1SGrainOpts), device, batch_frames, int(clip_to_restricted_range), 0)
    err = C.create_string_buffer(512)
    unequal = C.c_int(0)
    n = _lib.lib().g1s_check_y4m_files_scales(str(source).encode(), str(denoised).encode(), str(table).encode(), str(output).encode(),
                                              _path(temporal_output), _path(cross_output), _path(scales_output), C.byref(opts), C.byref(gopts),
                                              C.byref(unequal), err, len(err))
    if n < 0:
        raise G1SError(int(n), err.value.decode())
    if unequal.value:
        log.warning(UNEQUAL_WARNING)
    log.info("Checked %d frames", n)
    return int(n), bool(unequal.value)
