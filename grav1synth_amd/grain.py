"""`render`: AV1 film grain synthesis on an MI355X -- what a grain table does to a frame (the inverse of `diff`).

The film grain synthesis process of the AV1 specification (clause 7.18.3) as HIP kernels behind g1s_grain_*
(include/g1s_diff.h): integer-exact, no CPU fallback.

>>> syn = GrainSynthesizer(10)
>>> grainy = syn.apply([y, u, v], segment)      # torch device tensors stay on the device; numpy in, numpy out
>>> render_y4m_file("clean.y4m", "table.tbl", "grainy.y4m")
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import G1SError, G1SGrainOpts
from ._frame_op import FrameOp
from .diff import GrainTableSegment

log = logging.getLogger("grav1synth")


def gaussian_sequence() -> np.ndarray:
    """Gaussian_Sequence[2048] of the specification's "Additional tables" (int16)."""
    return np.ctypeslib.as_array(_lib.lib().g1s_grain_gaussian_sequence(), shape=(2048,)).copy()


def _opts(device: int, batch_frames: int, clip_to_restricted_range: bool, mc_identity: bool) -> G1SGrainOpts:
    o = G1SGrainOpts()
    o.struct_size = C.sizeof(G1SGrainOpts)
    o.device = device
    o.batch_frames = batch_frames
    o.clip_to_restricted_range = int(clip_to_restricted_range)
    o.mc_identity = int(mc_identity)
    return o


class GrainSynthesizer(FrameOp):
    _name = "grain"

    def __init__(self, bit_depth: int, *, device: int = -1, batch_frames: int = 0, clip_to_restricted_range: bool = False,
                 mc_identity: bool = False):
        self._L = _lib.lib()
        self.bit_depth = bit_depth
        opts = _opts(device, batch_frames, clip_to_restricted_range, mc_identity)
        self._h = self._L.g1s_grain_new(bit_depth, C.byref(opts))
        if not self._h:
            raise G1SError(-5, self._L.g1s_last_global_error().decode())
        self._keep: list = []  # planes the queued kernels still read or write

    def apply(self, frame_planes: Sequence, segment: Optional[GrainTableSegment], xdec: int = 1, ydec: int = 1, *, sync: bool = True,
              out: Optional[Sequence] = None) -> List:
        """The grain of `segment` (its random_seed is the frame's grain_seed) on one frame: new planes of the same kind -- torch
        device tensors stay on the device, host planes go through host frames.  segment = None: a copy (apply_grain = 0).
        sync = False queues the frame (a batch goes out as one launch): the returned planes are complete after sync()."""
        planes, out, keep, fin, fout = self._frame_pair(frame_planes, xdec, ydec, out)
        seg = segment.to_c() if segment is not None else None
        self._keep.append(keep)
        self._check(self._L.g1s_grain_frame(self._h, C.byref(seg) if seg is not None else None, C.byref(fin), C.byref(fout)))
        if sync:
            self.sync()
        return out

    def sync(self) -> None:
        self._check(self._L.g1s_grain_sync(self._h))
        self._keep.clear()

    def templates(self, segment: GrainTableSegment, xdec: int = 1, ydec: int = 1):
        """(LumaGrain 73 x 82, CbGrain, CrGrain, ScalingLut 3 x 256) of the generate grain process and the scaling lookup
        initialisation for these parameters, as the device computes them."""
        cw, ch = (44 if xdec else 82), (38 if ydec else 73)
        luma, cb, cr = np.zeros((73, 82), np.int16), np.zeros((ch, cw), np.int16), np.zeros((ch, cw), np.int16)
        lut = np.zeros((3, 256), np.uint8)
        seg = segment.to_c()
        self._check(self._L.g1s_grain_templates(self._h, C.byref(seg), xdec, ydec, luma.ctypes.data, cb.ctypes.data, cr.ctypes.data,
                                                lut.ctypes.data))
        return luma, cb, cr, lut

    def kernel_times(self, enable: bool = True):
        """(ms in kg_template, ms in kg_apply, frames) of the timed batches so far (HIP events); enables / disables the timing."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint64()
        self._L.g1s_grain_set_timing(self._h, int(enable), C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value


def render_y4m_file(input: str, table: str, output: str, *, device: int = -1, batch_frames: int = 0,
                    clip_to_restricted_range: bool = False, mc_identity: bool = False) -> int:
    """`render INPUT -g TABLE -o OUTPUT` for a .y4m input: every frame through the table's lookup at its presentation time.
    Returns the number of frames."""
    L = _lib.lib()
    opts = _opts(device, batch_frames, clip_to_restricted_range, mc_identity)
    err = C.create_string_buffer(512)
    n = L.g1s_grain_y4m_file(input.encode(), table.encode(), output.encode(), C.byref(opts), err, len(err))
    if n < 0:
        raise G1SError(int(n), err.value.decode())
    log.info("Rendered grain onto %d frames", n)
    return int(n)
