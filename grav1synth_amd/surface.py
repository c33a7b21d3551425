"""Decoder surfaces on an MI355X: NV12, P010 / P012 / P016 and MSB-aligned planes to planar frames and back.

A hardware decoder hands out semi-planar surfaces (a luma plane and a plane of interleaved Cb, Cr pairs, above 8 bits with
the sample in the high bits of its 16-bit word); every operation of this package takes planar frames with the sample in the
low bits.  HIP kernels behind g1s_surface_* (include/g1s_diff.h, where the layouts and the six rules are); no CPU fallback.

>>> conv = SurfaceConverter(10)
>>> y, u, v = conv.unpack(Surface([luma, cbcr], 10))        # P010: torch device tensors stay on the device
>>> p010 = conv.pack([y, u, v])                             # and back: p010.planes == [luma, cbcr]
>>> nv12 = SurfaceConverter(8).pack([y8, u8, v8])           # NV12

The converter runs on a stream of its own: with sync = False a frame is complete, and may go to another operation, after
sync().  There is no command for this: .y4m has no tag for these layouts."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import G1SError, G1SSurface, G1SSurfaceOpts
from ._frame_op import FrameOp
from .diff import Frame

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _chroma_shape(h: int, w: int, xdec: int, ydec: int) -> Tuple[int, int]:
    return (h + ydec) >> ydec, (w + xdec) >> xdec


class Surface:
    """A decoder surface: len(planes) is 1 (luma only), 2 (luma and a plane of interleaved Cb, Cr pairs, 2 cw samples a row)
    or 3 (planar).  msb_aligned: the sample sits in the high bit_depth bits of its 16-bit word; by default what P010 / P012 /
    P016 do (two planes above 8 bits)."""

    def __init__(self, planes: Sequence, bit_depth: int, xdec: int = 1, ydec: int = 1, msb_aligned: Optional[bool] = None):
        self.planes = list(planes)
        self.bit_depth, self.xdec, self.ydec = bit_depth, xdec, ydec
        self.msb_aligned = (bit_depth > 8 and len(self.planes) == 2) if msb_aligned is None else bool(msb_aligned)

    def to_c(self, keep: list) -> G1SSurface:
        f = Frame(self.planes, self.xdec, self.ydec).to_c(keep)  # (pointers, strides, sample size and memory kind as a frame's)
        s = G1SSurface()
        s.width, s.height, s.bytes_per_sample, s.xdec, s.ydec, s.nplanes = f.width, f.height, f.bytes_per_sample, f.xdec, f.ydec, f.nplanes
        s.bit_depth, s.msb_aligned = self.bit_depth, int(self.msb_aligned)
        for c in range(len(self.planes)):
            s.data[c], s.stride_bytes[c] = f.data[c], f.stride_bytes[c]
        s.on_device = f.on_device
        return s


def _like(p, shape):
    if torch is not None and isinstance(p, torch.Tensor):
        return torch.empty(shape, dtype=p.dtype, device=p.device)
    return np.empty(shape, np.asarray(p).dtype)


class SurfaceConverter(FrameOp):
    _name = "surface"

    def __init__(self, bit_depth: int, device: int = -1, batch_frames: int = 0):
        self._L = _lib.lib()
        self.bit_depth = bit_depth
        opts = G1SSurfaceOpts(C.sizeof(G1SSurfaceOpts), device, batch_frames)
        self._h = self._L.g1s_surface_new(bit_depth, C.byref(opts))
        if not self._h:
            raise G1SError(-5, self._L.g1s_last_global_error().decode())
        self._keep: list = []  # planes the queued kernels still read or write

    def _run(self, call, cin, cout, keep, sync: bool) -> None:
        if cin.on_device == 1:
            torch.cuda.current_stream().synchronize()  # (the planes were produced on torch's stream)
        self._keep.append(keep)
        self._check(call(self._h, C.byref(cin), C.byref(cout)))
        if sync:
            self.sync()

    def unpack(self, surface: Surface, out: Optional[Sequence] = None, *, sync: bool = True) -> List:
        """The planar frame of a surface (frame = word >> sh): 1 or 3 new planes of the same kind as the surface's, or `out`.
        sync = False queues the frame (a batch goes out as one launch): the planes are complete after sync()."""
        p0 = surface.planes[0]
        h, w = int(p0.shape[0]), int(p0.shape[1])
        if out is None:
            out = [_like(p0, (h, w))]
            if len(surface.planes) > 1:
                out += [_like(p0, _chroma_shape(h, w, surface.xdec, surface.ydec)) for _ in range(2)]
        out = list(out)
        keep: list = []
        self._run(self._L.g1s_surface_unpack, surface.to_c(keep), Frame(out, surface.xdec, surface.ydec).to_c(keep), keep, sync)
        return out

    def pack(self, planes: Sequence, xdec: int = 1, ydec: int = 1, interleaved: bool = True, msb_aligned: Optional[bool] = None, out=None, *,
             sync: bool = True) -> Surface:
        """The surface of a planar frame (word = (sample << sh) & 0xffff): interleaved chroma (NV12, P010, ...) or three
        planes; msb_aligned by default as Surface has it.  `out`: a Surface or its planes to write into."""
        planes = list(planes)
        if not (torch is not None and isinstance(planes[0], torch.Tensor)):
            planes = [np.asarray(p) for p in planes]
        p0 = planes[0]
        h, w = int(p0.shape[0]), int(p0.shape[1])
        if isinstance(out, Surface):
            surface = out
        else:
            if out is None:
                ch, cw = _chroma_shape(h, w, xdec, ydec)
                out = [_like(p0, (h, w))]
                if len(planes) > 1:
                    out += [_like(p0, (ch, 2 * cw))] if interleaved else [_like(p0, (ch, cw)) for _ in range(2)]
            surface = Surface(list(out), self.bit_depth, xdec, ydec, msb_aligned)
        keep: list = []
        self._run(self._L.g1s_surface_pack, Frame(planes, xdec, ydec).to_c(keep), surface.to_c(keep), keep, sync)
        return surface

    def sync(self) -> None:
        self._check(self._L.g1s_surface_sync(self._h))
        self._keep.clear()

    def kernel_time(self, enable: bool = True) -> Tuple[float, int]:
        """(ms in ks_unpack / ks_pack, frames) of the timed batches so far (HIP events); enables / disables the timing."""
        a, n = C.c_double(), C.c_uint64()
        self._L.g1s_surface_set_timing(self._h, int(enable), C.byref(a), C.byref(n))
        return a.value, n.value
