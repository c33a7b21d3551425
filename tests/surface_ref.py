"""Rules 1 - 4 of include/g1s_diff.h ("decoder surfaces") in numpy: the reference of tests/test_surface_cpu.py,
tests/test_gpu_surface.py and tests/test_gpu_surface_sweep.py (test infrastructure).  A surface is a list of 1, 2 or 3 planes;
with 2, plane 1 holds rows of Cb[0], Cr[0], Cb[1], Cr[1], ...  Planes are uint8, or uint16 with sh = 16 - bit_depth when
msb_aligned."""
import numpy as np


def shift(bit_depth: int, msb_aligned: bool) -> int:
    return 16 - bit_depth if msb_aligned else 0


def chroma_shape(h: int, w: int, xdec: int, ydec: int):
    return (h + ydec) >> ydec, (w + xdec) >> xdec


def unpack(surface, bit_depth: int, msb_aligned: bool):
    """frame = word >> sh; the interleaved plane's even samples are Cb, its odd ones Cr."""
    sh = shift(bit_depth, msb_aligned)
    planes = [surface[0]] + ([surface[1][:, 0::2], surface[1][:, 1::2]] if len(surface) == 2 else list(surface[1:]))
    return [np.ascontiguousarray(p >> sh) for p in planes]


def pack(frame, bit_depth: int, msb_aligned: bool, interleaved: bool = True):
    """word = (sample << sh) & 0xffff (a byte for one-byte samples, which have sh = 0)."""
    sh = shift(bit_depth, msb_aligned)
    planes = [((p.astype(np.uint32) << sh) & 0xffff).astype(p.dtype) for p in frame]
    if len(planes) == 3 and interleaved:
        pairs = np.empty((planes[1].shape[0], 2 * planes[1].shape[1]), planes[1].dtype)
        pairs[:, 0::2], pairs[:, 1::2] = planes[1], planes[2]
        planes = [planes[0], pairs]
    return planes
