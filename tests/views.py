"""A plane as a view into a larger device buffer, the way a decoder or a filter hands one out: a pitch that is not the
row, a base that is not what the allocator returns, and memory around the samples that is somebody else's (test
infrastructure; no fixtures).

The margin is hostile: the bytes left and right of every row and the guard rows above and below hold random samples over
the whole code range (or the maximum code value), so a kernel that replicates an edge from one sample past the row, or
sums over the pitch, computes something else.  The buffer is built on the host, samples and margin, and uploaded once; its
host copy is what the guard compares with afterwards."""
from __future__ import annotations

from typing import Tuple, Union

import numpy as np

PAD = 32      # bytes in front of the first guard row and behind the last row
ALIGN = 256   # the view's base is placed relative to a boundary of this many bytes


class Guard:
    """What device_view built around a plane.  `buffer`: the uint8 tensor that holds margin and samples; `inside`: which of
    its bytes are the view's."""

    def __init__(self, buffer, host: np.ndarray, inside: np.ndarray):
        self.buffer, self._host, self.inside = buffer, host, inside

    def _now(self) -> np.ndarray:
        return self.buffer.cpu().numpy()

    def changed_bytes(self) -> np.ndarray:
        """Offsets of the bytes of the whole buffer that differ from what was uploaded (an input: none may)."""
        return np.flatnonzero(self._now() != self._host)

    def changed_margin_bytes(self) -> np.ndarray:
        """Offsets of the bytes outside the view that no longer hold the fill (an output: none may)."""
        return np.flatnonzero((self._now() != self._host) & ~self.inside)

    def assert_unchanged(self, what: str) -> None:
        bad = self.changed_bytes()
        assert bad.size == 0, f"{what}: {bad.size} bytes of an input buffer were written, first at offset {int(bad[0])}"

    def assert_margin_intact(self, what: str) -> None:
        bad = self.changed_margin_bytes()
        assert bad.size == 0, f"{what}: {bad.size} bytes outside the view were written, first at offset {int(bad[0])}"


def device_view(plane: np.ndarray, *, pitch_bytes: int, base_offset_bytes: int, rows_above: int = 2, rows_below: int = 2,
                fill: Union[str, int, tuple] = "random", max_code: int = 0, seed: int = 0, device: str = "cuda") -> Tuple[object, Guard]:
    """(view, guard): `view` is a torch tensor of the plane's shape and dtype with stride(1) == 1, stride(0) * itemsize ==
    pitch_bytes and data_ptr() % 256 == base_offset_bytes, inside a uint8 buffer on `device` whose other bytes hold the fill:
    "random" (samples 0 .. max_code, seeded), (lo, hi) (random samples of that range: a margin that looks like the picture), "max"
    (max_code) or a sample value.  max_code: the depth's largest code value
    (default: the dtype's).  The alignment comes from the buffer's data_ptr(), which is looked at, not assumed."""
    import torch

    plane = np.ascontiguousarray(plane)
    h, w = plane.shape
    isz = plane.dtype.itemsize
    row = w * isz
    if isz not in (1, 2) or pitch_bytes < row or pitch_bytes % isz or base_offset_bytes % isz or not 0 <= base_offset_bytes < ALIGN:
        raise ValueError(f"no view of a {w}-sample row of {isz}-byte samples with pitch {pitch_bytes} at offset {base_offset_bytes}")
    top = max_code or (1 << (8 * isz)) - 1
    lead = PAD + rows_above * pitch_bytes                      # from the region's first byte to the view's first sample
    total = lead + (h + rows_below) * pitch_bytes + PAD
    nsamp = total // isz
    if fill == "random" or isinstance(fill, tuple):
        lo, hi = (0, top) if fill == "random" else fill
        host = np.random.default_rng([seed, h, w, pitch_bytes]).integers(lo, hi + 1, nsamp).astype(plane.dtype)
    else:
        host = np.full(nsamp, top if fill == "max" else int(fill), plane.dtype)
    host = host.view(np.uint8).copy()
    inside = np.zeros(total, bool)
    for r in range(h):
        o = lead + r * pitch_bytes
        host[o:o + row] = plane[r].view(np.uint8)
        inside[o:o + row] = True
    raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
    skip = (base_offset_bytes - raw.data_ptr() - lead) % ALIGN
    buffer = raw[skip:skip + total]
    buffer.copy_(torch.from_numpy(host))
    body = buffer[lead:lead + (h - 1) * pitch_bytes + row]
    if isz == 2:
        body = body.view(torch.uint16)
    view = body.as_strided((h, w), (pitch_bytes // isz, 1))
    assert view.data_ptr() % ALIGN == base_offset_bytes and view.data_ptr() & 15 == base_offset_bytes & 15, hex(view.data_ptr())
    assert view.stride(1) == 1 and view.stride(0) * view.element_size() == pitch_bytes
    assert view.data_ptr() - buffer.data_ptr() == lead
    return view, Guard(buffer, host, inside)


def contiguous(plane: np.ndarray, device: str = "cuda"):
    """The plane as a fresh contiguous tensor on the device: what the rest of the suite feeds."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(plane)).to(device)


# ---- views with a pitch of megabytes: gigabytes from the first row to the last ---------------------------------------------

GAP = 4096  # bytes behind every row and in front of the next one that hold hostile samples and are looked at afterwards


class FarGuard:
    """What far_view built around a plane: the rows, and of the gap between two rows the first and the last GAP bytes (random
    samples; the rest of the gap is one byte value and is not looked at: it is gigabytes)."""

    def __init__(self, buffer, spans):
        self.buffer, self._spans = buffer, spans  # spans: (offset, host bytes, inside the view?)

    def _changed(self, inside_too: bool):
        out = []
        for o, host, inside in self._spans:
            if inside and not inside_too:
                continue
            now = self.buffer[o:o + host.size].cpu().numpy()
            out += [o + int(k) for k in np.flatnonzero(now != host)]
        return out

    def assert_unchanged(self, what: str) -> None:
        bad = self._changed(True)
        assert not bad, f"{what}: {len(bad)} bytes of an input buffer were written, first at offset {bad[0]}"

    def assert_margin_intact(self, what: str) -> None:
        bad = self._changed(False)
        assert not bad, f"{what}: {len(bad)} bytes outside the view were written, first at offset {bad[0]}"


def far_view(plane: np.ndarray, *, pitch_bytes: int, base_offset_bytes: int, max_code: int = 0, seed: int = 0, device: str = "cuda"):
    """(view, guard) as device_view gives them, for a pitch so large that the buffer cannot be built on the host: one device
    allocation of (rows + 1) * pitch_bytes, filled with the byte 0xA5 on the device; the rows, and GAP bytes of random samples
    (0 .. max_code) on either side of every row, written one by one at offsets computed here in python integers, so that
    nothing of the placement depends on anybody's 32-bit arithmetic."""
    import torch

    plane = np.ascontiguousarray(plane)
    h, w = plane.shape
    isz = plane.dtype.itemsize
    row = w * isz
    if isz not in (1, 2) or pitch_bytes < row + 2 * GAP or pitch_bytes % isz or base_offset_bytes % isz or not 0 <= base_offset_bytes < ALIGN:
        raise ValueError(f"no far view of a {w}-sample row of {isz}-byte samples with pitch {pitch_bytes} at offset {base_offset_bytes}")
    top = max_code or (1 << (8 * isz)) - 1
    lead = GAP + ALIGN
    total = lead + (h - 1) * pitch_bytes + row + GAP
    raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
    skip = (base_offset_bytes - raw.data_ptr() - lead) % ALIGN
    buffer = raw[skip:skip + total]
    buffer.fill_(0xA5)
    rng = np.random.default_rng([seed, h, w, pitch_bytes])
    spans = []
    for r in range(h):
        o = lead + r * pitch_bytes
        piece = np.concatenate([rng.integers(0, top + 1, GAP // isz).astype(plane.dtype), plane[r], rng.integers(0, top + 1, GAP // isz).astype(plane.dtype)])
        buffer[o - GAP:o + row + GAP].copy_(torch.from_numpy(piece.view(np.uint8)))
        b = piece.view(np.uint8)
        spans += [(o - GAP, b[:GAP].copy(), False), (o, b[GAP:GAP + row].copy(), True), (o + row, b[GAP + row:].copy(), False)]
    body = buffer[lead:lead + (h - 1) * pitch_bytes + row]
    if isz == 2:
        body = body.view(torch.uint16)
    view = body.as_strided((h, w), (pitch_bytes // isz, 1))
    assert view.data_ptr() % ALIGN == base_offset_bytes and view.data_ptr() - buffer.data_ptr() == lead
    assert view.stride(1) == 1 and view.stride(0) * view.element_size() == pitch_bytes
    return view, FarGuard(buffer, spans)
