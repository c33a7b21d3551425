"""Layouts, content and the seeded case list of the surface converter's tests (test infrastructure; numpy only).  The list is
drawn in the manner of tests/sweep.py, which is not edited: plain, pasteable records from numpy.random.default_rng, weighted to
the edges of the kernels' 16-byte lane and 32-byte interleaved load."""
from __future__ import annotations

import hashlib

import numpy as np

from tests import surface_ref as R

# name -> (bit depth, planes of the surface, msb_aligned, xdec, ydec)
LAYOUTS = {
    "nv12": (8, 2, False, 1, 1), "nv16": (8, 2, False, 1, 0), "nv24": (8, 2, False, 0, 0),
    "p010": (10, 2, True, 1, 1), "p012": (12, 2, True, 1, 1), "p016": (16, 2, True, 1, 1), "p210": (10, 2, True, 1, 0), "p410": (10, 2, True, 0, 0),
    "planar444_msb10": (10, 3, True, 0, 0), "planar420_lsb10": (10, 3, False, 1, 1), "mono12_msb": (12, 1, True, 0, 0), "mono12_lsb": (12, 1, False, 0, 0),
    "mono8": (8, 1, False, 0, 0),
}


def surface_shapes(name: str, w: int, h: int):
    _bd, nplanes, _msb, xdec, ydec = LAYOUTS[name]
    ch, cw = R.chroma_shape(h, w, xdec, ydec)
    return [(h, w)] + {1: [], 2: [(ch, 2 * cw)], 3: [(ch, cw)] * 2}[nplanes]


def frame_shapes(name: str, w: int, h: int):
    _bd, nplanes, _msb, xdec, ydec = LAYOUTS[name]
    return [(h, w)] + ([] if nplanes == 1 else [R.chroma_shape(h, w, xdec, ydec)] * 2)


def random_surface(name: str, w: int, h: int, seed=0):
    """Full-range words: the low sh bits of an MSB-aligned surface are random too.  Cb differs from Cr in the bits that count."""
    bd, nplanes, msb, _xdec, _ydec = LAYOUTS[name]
    rng = np.random.default_rng([seed, w, h, bd])
    dt, top = (np.uint8, 255) if bd == 8 else (np.uint16, 65535)
    planes = [rng.integers(0, top + 1, s).astype(dt) for s in surface_shapes(name, w, h)]
    if nplanes > 1:
        cb, cr = (planes[1][:, 0::2], planes[1][:, 1::2]) if nplanes == 2 else (planes[1], planes[2])
        if np.array_equal(cb >> R.shift(bd, msb), cr >> R.shift(bd, msb)):
            cr[0, 0] ^= dt(top ^ (top >> 1))  # the word's highest bit
    return planes


def random_frame(name: str, w: int, h: int, seed=0):
    """Samples over 0 .. 2^bit_depth - 1, both ends present in every plane that has two samples; Cb differs from Cr."""
    bd, _nplanes, _msb, _xdec, _ydec = LAYOUTS[name]
    rng = np.random.default_rng([seed, w, h, bd, 1])
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [rng.integers(0, 1 << bd, s).astype(dt) for s in frame_shapes(name, w, h)]
    for c, p in enumerate(planes):
        flat = p.reshape(-1)
        flat[0] = (1 << bd) - 1 if c < 2 else 0  # (a plane of one sample: Cb the top, Cr the bottom)
        if flat.size > 1:
            flat[-1] = (1 << bd) - 1 - int(flat[0])
    return planes


# ---- the seeded sweep ----------------------------------------------------------------------------------------------------------

SEED, N, CHUNKS = 12, 96, 3
PITCHES = ("row", "row+1", "row256")  # the row itself, one sample more, the row rounded up to 256 bytes
FORCED = [
    dict(layout="nv12", w=1, h=1, base=0, pitch="row"), dict(layout="p010", w=1, h=1, base=2, pitch="row+1"),
    dict(layout="nv12", w=32, h=2, base=0, pitch="row256"), dict(layout="nv12", w=33, h=3, base=15, pitch="row+1"),
    dict(layout="p016", w=16, h=49, base=0, pitch="row"), dict(layout="p010", w=17, h=47, base=14, pitch="row256"),
    dict(layout="planar444_msb10", w=8, h=5, base=0, pitch="row+1"), dict(layout="mono12_msb", w=9, h=48, base=8, pitch="row"),
    dict(layout="nv24", w=31, h=4, base=1, pitch="row256"), dict(layout="p410", w=15, h=1, base=0, pitch="row"),
]


def _pick(rng, menu):
    w = np.array([m[1] for m in menu], float)
    return menu[int(rng.choice(len(menu), p=w / w.sum()))][0]


def cases():
    """96 records: layout, luma width and height, the base offset of every plane in bytes (0 .. 15, a multiple of the sample
    size) and the pitch rule, for the surface and the frame side alike."""
    rng = np.random.default_rng([SEED] + list(b"surface"))
    out = []
    for i in range(N):
        if i < len(FORCED):
            c = dict(FORCED[i])
        else:
            layout = list(LAYOUTS)[int(rng.integers(0, len(LAYOUTS)))] if i % 2 else list(LAYOUTS)[(i // 2) % len(LAYOUTS)]
            bd, _np, _msb, xdec, _ydec = LAYOUTS[layout]
            bps = 1 if bd == 8 else 2
            # widths whose rows are one sample below, on and above 16 and 32 bytes -- in the luma plane or, doubled, in a chroma plane
            unit = int(_pick(rng, [(16, 2), (32, 2), (64, 1)])) // bps * int(_pick(rng, [(1, 2), (1 << xdec, 1)]))
            w = unit * int(rng.integers(1, 4)) + int(_pick(rng, [(-1, 2), (0, 2), (1, 2), (int(rng.integers(2, 9)), 1)]))
            h = int(_pick(rng, [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (47, 1), (48, 1), (49, 1)]))
            base = int(_pick(rng, [(0, 3), (int(rng.integers(0, 16)), 5), (15, 1), (8, 1)])) // bps * bps
            c = dict(layout=layout, w=max(w, 1), h=h, base=base, pitch=_pick(rng, [(p, 1) for p in PITCHES]))
        out.append({"op": "surface", "i": i, **c, "forced": i < len(FORCED)})
    return out


def digest(case_list) -> str:
    return hashlib.sha256(repr(case_list).encode()).hexdigest()


def pitch_of(rule: str, row_bytes: int, bps: int) -> int:
    return {"row": row_bytes, "row+1": row_bytes + bps, "row256": (row_bytes + 255) // 256 * 256}[rule]
