"""A second family of synthetic frame pairs, asymmetric where grav1synth_amd/synth.py is symmetric (test infrastructure).

synth.py's noise filter is invariant under mirroring and transposition and its Cb and Cr planes follow one law, so a
table made from it cannot tell Cb from Cr, nor a coefficient at (dx, dy) from the ones at (-dx, dy) and (dy, dx).  Here
every plane has its own causal, one-sided tap set (Y and Cr with a negative tap), its own intensity -> gain
law (Y rising, Cb rising more slowly, Cr falling) over base ramps wide enough for several scaling points, and the luma
residual enters Cb with weight + 1/2 and Cr with weight - 1/4.

Integer arithmetic on numpy int64 only; deterministic from the arguments.  The planes come in the layout
tests.helpers.np_pair returns: lists of C-contiguous 2-D arrays, uint8 for 8-bit and uint16 above.

Kinds, all variations of one frame so that a job can change kind from batch to batch at one geometry:
  distinct  the ramps, and a checker texture the flat-block finder must reject over the lower right part of the frame; its
            border lies 12 / 20 luma samples off the block grid (6 / 10 chroma samples at 4:2:0)
  flat      no texture: every block is accepted
  busy      texture everywhere but a corner of a few dozen blocks
  damaged   `distinct` with |source - denoised| > 127 (denoised side only: the finder reads the source) at many samples
            of all three planes, half of them in the last / first three samples of a 64-sample run
  clamped   base 1 in the left third and 254 in the right third (all planes): the clamp cuts the residuals, block means
            sit in the first and in the last intensity bin
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

KINDS = ("distinct", "flat", "busy", "damaged", "clamped")

# (dy, dx) -> weight; dy <= 0 and, on the row itself, dx <= 0: causal.
# The flat-block finder reads the luma source and refuses a block whose gradient covariance (central differences) has
# eigenvalues further apart than 1.25 : 1, which is what a left-heavy or up-heavy filter gives it.  Luma's taps are knight's
# moves: its autocorrelation is zero at (2, 0), (0, 2), (1, 1) and (-1, 1), the only lags that covariance sees, and
# 18 at (2, 1) against 0 at (-2, 1) and (1, 2).  The chroma planes are not the finder's business and take axial taps.
TAPS = (
    {(0, 0): 6, (-1, -2): 3, (-2, 1): -2},              # Y: one row up two left, two rows up one right (negative)
    {(0, 0): 6, (-1, 0): 3, (0, -1): 1, (-1, -1): 2},   # Cb: up-heavy, an up-left tap
    {(0, 0): 6, (0, -1): -3, (-1, 0): 2, (0, -2): 1},   # Cr: alternating along the row
)


def _plane_noise(rng, h: int, w: int, taps) -> np.ndarray:
    n0 = rng.integers(-255, 256, (h + 4, w + 4)).astype(np.int64) + rng.integers(-255, 256, (h + 4, w + 4))
    out = np.zeros((h, w), np.int64)
    for (dy, dx), k in taps.items():
        out += k * n0[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
    return out


def _thirds(base8: np.ndarray, xs: np.ndarray, w: int) -> np.ndarray:
    return np.where(xs < w // 3, 1, np.where(xs >= w - w // 3, 254, base8))


def _damage(rng, src: np.ndarray, den: np.ndarray, up: int) -> None:
    h, w = den.shape
    n = max(24, (h * w) // 2048)  # about one sample for every second 32 x 32 block of the plane
    for i in range(n):
        y = int(rng.integers(0, h))
        if i & 1 and w > 192:  # the last / first words of a 64-sample run
            u = int(rng.integers(1, w // 64))
            x = 64 * u - 1 - int(rng.integers(0, 3)) if i & 2 else 64 * u + int(rng.integers(0, 3))
        else:
            x = int(rng.integers(0, w))
        den[y, x] = 0 if (int(src[y, x]) >> up) > 140 else (255 << up)


def make_frames(kind: str, width: int, height: int, bit_depth: int, xdec: int, ydec: int, frame: int,
                seed: int = 1) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """(source_planes, denoised_planes) of frame `frame`: three planes each, chroma decimated by (xdec, ydec)."""
    if kind not in KINDS:
        raise ValueError(f"unknown content kind {kind!r}")
    w, h = width, height
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    tex = np.zeros((h, w), bool)
    if kind in ("distinct", "damaged", "clamped"):
        tex = (xs >= ((5 * w // 8) & ~31) + 12) & (ys >= ((h // 3) & ~31) + 20)
    elif kind == "busy":
        tex = ~((xs < min(6 * 32, (w // 2) & ~31) + 12) & (ys < min(4 * 32, (h // 2) & ~31) + 20))
    src, den = textured_frames(tex, width, height, bit_depth, xdec, ydec, frame, seed, thirds=kind == "clamped")
    if kind == "damaged":
        for c in range(3):
            _damage(np.random.default_rng([seed, frame, 8 + c]), src[c], den[c], bit_depth - 8)
    return src, den


def textured_frames(tex: np.ndarray, width: int, height: int, bit_depth: int, xdec: int, ydec: int, frame: int, seed: int = 1,
                    thirds: bool = False) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """The frame pair every kind is made of: the ramps, gain laws, taps and luma-into-chroma weights above, and the checker texture
    on the luma samples where `tex` (bool, height x width) is set.  tests/mask_content.py places the texture block by block."""
    w, h, up, maxv = width, height, bit_depth - 8, (1 << bit_depth) - 1
    dt = np.uint8 if bit_depth == 8 else np.uint16
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    base8 = 24 + (xs * 200) // w + (ys * 20) // h
    if thirds:
        base8 = _thirds(base8, xs, w)
    gain = 3 + (base8 >> 6)  # Y: rising, 3 .. 6
    checker = ((((xs >> 3) + (ys >> 3)) & 1) * 48 - 24) + (xs & 1) * 8
    den8 = np.clip(base8 + tex * checker, 0, 255)
    d = den8 << up
    n = _plane_noise(np.random.default_rng([seed, frame, 0]), h, w, TAPS[0])
    s = np.clip(d + ((n * gain) >> (12 - up)), 0, maxv)
    src, den = [s], [d]
    cw, ch = w >> xdec, h >> ydec
    lco = (s - d)[::1 << ydec, ::1 << xdec][:ch, :cw]  # the luma residual as it is after the clamp
    cys, cxs = np.arange(ch, dtype=np.int64)[:, None], np.arange(cw, dtype=np.int64)[None, :]
    for c in (1, 2):
        cb8 = (64 + (cxs * 128) // cw + 0 * cys) if c == 1 else (200 - (cys * 128) // ch + 0 * cxs)
        if thirds:
            cb8 = _thirds(cb8, cxs, cw)
        g = (2 + (cb8 >> 6)) if c == 1 else 2 * (6 - (cb8 >> 6))  # Cb: rising slowly; Cr: falling
        lw = (lco >> 1) if c == 1 else -(lco >> 2)
        cn = _plane_noise(np.random.default_rng([seed, frame, c]), ch, cw, TAPS[c])
        dc = cb8 << up
        src.append(np.clip(dc + ((cn * g) >> (12 - up)) + lw, 0, maxv))
        den.append(dc)
    src = [np.ascontiguousarray(p.astype(dt)) for p in src]
    den = [np.ascontiguousarray(p.astype(dt)) for p in den]
    return src, den
