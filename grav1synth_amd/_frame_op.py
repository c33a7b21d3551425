"""What GrainSynthesizer and Denoiser share: a handle behind g1s_<name>_*, its error text, and a frame pair for the C call."""
from __future__ import annotations

import numpy as np

from ._lib import G1SError
from .diff import Frame

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class FrameOp:
    _name = ""  # the operation's symbols are g1s_<_name>_frame, _sync, _last_error, _free

    def _check(self, rc: int) -> None:
        if rc:
            raise G1SError(rc, getattr(self._L, f"g1s_{self._name}_last_error")(self._h).decode())

    @staticmethod
    def _frame_pair(frame_planes, xdec: int, ydec: int, out):
        """(planes, out, keep, fin, fout): `out` made like the input planes when None, both as g1s_frame_t; `keep` holds
        what the two structs point into."""
        planes = list(frame_planes)
        if out is None:
            if torch is not None and isinstance(planes[0], torch.Tensor):
                out = [torch.empty(p.shape, dtype=p.dtype, device=p.device) for p in planes]
            else:
                planes = [np.asarray(p) for p in planes]
                out = [np.empty(p.shape, p.dtype) for p in planes]
        out = list(out)
        keep: list = []
        fin = Frame(planes, xdec, ydec).to_c(keep)
        fout = Frame(out, xdec, ydec).to_c(keep)
        if fin.on_device == 1:
            torch.cuda.current_stream().synchronize()  # (the planes were produced on torch's stream)
        return planes, out, keep, fin, fout

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._L, f"g1s_{self._name}_free")(self._h)
            self._h = None
            self._keep.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
