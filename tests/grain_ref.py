"""A numpy restatement of the AV1 film grain synthesis process (AV1 Bitstream & Decoding Process Specification, clause
7.18.3 and its sub-clauses), structured as the standard is: the random number process (7.18.3.2), the generate grain
process (7.18.3.3), the scaling lookup initialisation (7.18.3.4) and the add noise synthesis process (7.18.3.5) with
its noise stripes, its noise image and its final blend.  TEST INFRASTRUCTURE: the device kernels are compared with this
byte for byte.  It shares one thing with the library, the standard's constant Gaussian_Sequence, read through the
library's accessor; its LFSR, its lookup tables and its arithmetic are its own.

A segment is any object with the fields of grav1synth_amd.diff.GrainTableSegment; `random_seed` is the grain_seed of the
frame.  The table's fields carry the syntax elements as libaom's tables do: AR coefficients already minus 128,
ar_coeff_shift and scaling_shift as the shifts themselves, cb_mult / cb_luma_mult / cb_offset as coded (minus 128, 128, 256
where they are used).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

_GAUSS = None


def gaussian_sequence() -> np.ndarray:
    global _GAUSS
    if _GAUSS is None:
        from grav1synth_amd import _lib

        L = C.CDLL(_lib.LIB_PATH)
        L.g1s_grain_gaussian_sequence.restype = C.POINTER(C.c_int16)
        _GAUSS = np.ctypeslib.as_array(L.g1s_grain_gaussian_sequence(), shape=(2048,)).astype(np.int64)
    return _GAUSS


def round2(x, n):
    """Round2( x, n ) of the standard's conventions: ( x + ( 1 << ( n - 1 ) ) ) >> n, an arithmetic shift."""
    if n == 0:
        return x
    return (x + (1 << (n - 1))) >> n


class RandomRegister:
    """7.18.3.2: a 16-bit LFSR with taps 0, 1, 3, 12; a draw of `bits` bits is the top of the register after one step."""

    def __init__(self, seed: int):
        self.r = seed & 0xFFFF

    def get(self, bits: int) -> int:
        r = self.r
        bit = ((r >> 0) ^ (r >> 1) ^ (r >> 3) ^ (r >> 12)) & 1
        r = (r >> 1) | (bit << 15)
        self.r = r
        return (r >> (16 - bits)) & ((1 << bits) - 1)


def grain_range(bit_depth: int):
    center = 128 << (bit_depth - 8)
    return -center, (256 << (bit_depth - 8)) - 1 - center


def generate_grain(seg, bit_depth: int, subx: int, suby: int, mono: bool = False):
    """7.18.3.3: LumaGrain (73 x 82), CbGrain and CrGrain (chromaH x chromaW), int64 arrays."""
    gauss = gaussian_sequence()
    gmin, gmax = grain_range(bit_depth)
    lag = seg.ar_coeff_lag
    num_y = len(seg.scaling_points_y)
    shift = 12 - bit_depth + seg.grain_scale_shift
    rng = RandomRegister(seg.random_seed)
    luma = np.zeros((73, 82), np.int64)
    for y in range(73):
        for x in range(82):
            g = int(gauss[rng.get(11)]) if num_y > 0 else 0
            luma[y, x] = round2(g, shift)
    ar_shift = seg.ar_coeff_shift
    if lag > 0:  # (with no taps the filter adds Round2(0, shift) = 0)
        cy = np.array(list(seg.ar_coeffs_y)[: 2 * lag * (lag + 1)], np.int64)
        # the taps in scan order: rows -lag .. -1 whole, row 0 up to the sample itself
        taps = [(dr, dc) for dr in range(-lag, 1) for dc in range(-lag, lag + 1) if dr < 0 or dc < 0]
        for y in range(3, 73):
            for x in range(3, 82 - 3):
                s = 0
                for c, (dr, dc) in zip(cy, taps):
                    s += int(luma[y + dr, x + dc]) * int(c)
                luma[y, x] = min(gmax, max(gmin, int(luma[y, x]) + round2(s, ar_shift)))
    if mono:
        return luma, None, None
    cw, ch = (44 if subx else 82), (38 if suby else 73)
    csfl = bool(seg.chroma_scaling_from_luma)
    planes = []
    for seed_xor, npts in ((0xB524, len(seg.scaling_points_cb)), (0x49D8, len(seg.scaling_points_cr))):
        rng = RandomRegister(seg.random_seed ^ seed_xor)
        p = np.zeros((ch, cw), np.int64)
        for y in range(ch):
            for x in range(cw):
                g = int(gauss[rng.get(11)]) if (npts > 0 or csfl) else 0
                p[y, x] = round2(g, shift)
        planes.append(p)
    cb, cr = planes
    ncoef = 2 * lag * (lag + 1) + 1
    c0 = [int(v) for v in list(seg.ar_coeffs_cb)[:ncoef]]
    c1 = [int(v) for v in list(seg.ar_coeffs_cr)[:ncoef]]
    taps = [(dr, dc) for dr in range(-lag, 1) for dc in range(-lag, lag + 1) if dr < 0 or dc < 0]
    for y in range(3, ch):
        for x in range(3, cw - 3):
            s0 = s1 = 0
            for pos, (dr, dc) in enumerate(taps):
                s0 += int(cb[y + dr, x + dc]) * c0[pos]
                s1 += int(cr[y + dr, x + dc]) * c1[pos]
            if num_y > 0:
                lx, ly = ((x - 3) << subx) + 3, ((y - 3) << suby) + 3
                lu = 0
                for i in range(suby + 1):
                    for j in range(subx + 1):
                        lu += int(luma[ly + i, lx + j])
                lu = round2(lu, subx + suby)
                s0 += lu * c0[len(taps)]
                s1 += lu * c1[len(taps)]
            cb[y, x] = min(gmax, max(gmin, int(cb[y, x]) + round2(s0, ar_shift)))
            cr[y, x] = min(gmax, max(gmin, int(cr[y, x]) + round2(s1, ar_shift)))
    return luma, cb, cr


def scaling_lut(points) -> np.ndarray:
    """7.18.3.4 for one plane: 256 entries through the (value, scaling) points, flat outside them, zero without points."""
    lut = np.zeros(256, np.int64)
    n = len(points)
    if n == 0:
        return lut
    for x in range(points[0][0]):
        lut[x] = points[0][1]
    for i in range(n - 1):
        dy = points[i + 1][1] - points[i][1]
        dx = points[i + 1][0] - points[i][0]
        delta = dy * ((65536 + (dx >> 1)) // dx)
        for x in range(dx):
            lut[points[i][0] + x] = points[i][1] + ((x * delta + 32768) >> 16)
    for x in range(points[n - 1][0], 256):
        lut[x] = points[n - 1][1]
    return lut


def scaling_luts(seg) -> np.ndarray:
    """ScalingLut[ plane ][ 256 ]: chroma planes take the luma points under chroma_scaling_from_luma."""
    csfl = bool(seg.chroma_scaling_from_luma)
    return np.stack([scaling_lut(list(seg.scaling_points_y)),
                     scaling_lut(list(seg.scaling_points_y if csfl else seg.scaling_points_cb)),
                     scaling_lut(list(seg.scaling_points_y if csfl else seg.scaling_points_cr))])


def scale_lut(lut: np.ndarray, index: np.ndarray, bit_depth: int) -> np.ndarray:
    """scale_lut( plane, index ) on an array of indices."""
    shift = bit_depth - 8
    x = index >> shift
    if bit_depth == 8:
        return lut[x]
    rem = index - (x << shift)
    start = lut[x]
    end = lut[np.minimum(x + 1, 255)]
    return np.where(x == 255, start, start + round2((end - start) * rem, shift))


def block_offsets(seed: int, w: int, h: int):
    """The (offsetX, offsetY) draw of every 32 x 32 luma block, stripe by stripe: the LFSR is re-seeded per stripe."""
    out = []
    luma_num = 0
    for _y in range(0, (h + 1) // 2, 16):
        r = seed & 0xFFFF
        r ^= ((luma_num * 37 + 178) & 255) << 8
        r ^= (luma_num * 173 + 105) & 255
        rng = RandomRegister(r)
        row = []
        for _x in range(0, (w + 1) // 2, 16):
            rand = rng.get(8)
            row.append((rand >> 4, rand & 15))
        out.append(row)
        luma_num += 1
    return out


def noise_stripes(grain, seed, w, h, bit_depth, subx, suby, overlap):
    """noiseStripe[ lumaNum ][ plane ]: (34 >> planeSubY) rows, wide enough for the last block's 34 columns."""
    gmin, gmax = grain_range(bit_depth)
    offs = block_offsets(seed, w, h)
    stripes = []
    for luma_num, row in enumerate(offs):
        per_plane = []
        for plane, tmpl in enumerate(grain):
            if tmpl is None:
                continue
            psx, psy = (subx, suby) if plane > 0 else (0, 0)
            rows, cols = 34 >> psy, 34 >> psx
            stripe = np.zeros((rows, (len(row) * 32 + 34) >> psx), np.int64)
            for bx, (ox, oy) in enumerate(row):
                x = bx * 16  # the standard's x: half luma columns
                pox = 6 + ox if psx else 9 + ox * 2
                poy = 6 + oy if psy else 9 + oy * 2
                g = tmpl[poy:poy + rows, pox:pox + cols].copy()
                x0 = x if psx else x * 2
                if overlap and x > 0:
                    old = stripe[:, x0:x0 + 2].copy()
                    if psx == 0:
                        g[:, 0] = np.clip(round2(old[:, 0] * 27 + g[:, 0] * 17, 5), gmin, gmax)
                        g[:, 1] = np.clip(round2(old[:, 1] * 17 + g[:, 1] * 27, 5), gmin, gmax)
                    else:
                        g[:, 0] = np.clip(round2(old[:, 0] * 23 + g[:, 0] * 22, 5), gmin, gmax)
                stripe[:, x0:x0 + cols] = g
            per_plane.append(stripe)
        stripes.append(per_plane)
    return stripes


def noise_image(stripes, nplanes, w, h, bit_depth, subx, suby, overlap):
    """noiseImage[ plane ][ y ][ x ]: the stripes stacked, the first rows of a stripe blended with the rows the stripe
    above it left below its 32."""
    gmin, gmax = grain_range(bit_depth)
    out = []
    for plane in range(nplanes):
        psx, psy = (subx, suby) if plane > 0 else (0, 0)
        ph, pw = (h + psy) >> psy, (w + psx) >> psx
        img = np.zeros((ph, pw), np.int64)
        for y in range(ph):
            luma_num = y >> (5 - psy)
            i = y - (luma_num << (5 - psy))
            g = stripes[luma_num][plane][i, :pw].copy()
            if luma_num > 0 and overlap:
                if psy == 0 and i < 2:
                    old = stripes[luma_num - 1][plane][i + 32, :pw]
                    g = old * 27 + g * 17 if i == 0 else old * 17 + g * 27
                    g = np.clip(round2(g, 5), gmin, gmax)
                elif psy and i < 1:
                    old = stripes[luma_num - 1][plane][i + 16, :pw]
                    g = np.clip(round2(old * 23 + g * 22, 5), gmin, gmax)
            img[y] = g
        out.append(img)
    return out


def add_noise(planes, seg, bit_depth, subx=1, suby=1, clip_to_restricted_range=False, mc_identity=False, grain=None):
    """7.18.3.5 on one frame: planes = [Y] or [Y, U, V] (2-D unsigned arrays); returns new arrays of the same dtype."""
    mono = len(planes) == 1
    h, w = planes[0].shape
    if grain is None:
        grain = generate_grain(seg, bit_depth, subx, suby, mono)
    grain = [grain[0]] if mono else list(grain)
    luts = scaling_luts(seg)
    overlap = bool(seg.overlap_flag)
    stripes = noise_stripes(grain, seg.random_seed, w, h, bit_depth, subx, suby, overlap)
    noise = noise_image(stripes, len(planes), w, h, bit_depth, subx, suby, overlap)
    if clip_to_restricted_range:
        min_value = 16 << (bit_depth - 8)
        max_luma = 235 << (bit_depth - 8)
        max_chroma = max_luma if mc_identity else 240 << (bit_depth - 8)
    else:
        min_value = 0
        max_luma = (256 << (bit_depth - 8)) - 1
        max_chroma = max_luma
    shift = seg.scaling_shift
    out = [np.array(p, copy=True) for p in planes]
    in_y = planes[0].astype(np.int64)
    csfl = bool(seg.chroma_scaling_from_luma)
    if not mono:
        ph, pw = (h + suby) >> suby, (w + subx) >> subx
        ys = (np.arange(ph) << suby)[:, None]
        xs = (np.arange(pw) << subx)[None, :]
        if subx:
            average_luma = round2(in_y[ys, xs] + in_y[ys, np.minimum(xs + 1, w - 1)], 1)
        else:
            average_luma = in_y[ys, xs]
        for plane, npts, mult, luma_mult, offset in (
                (1, len(seg.scaling_points_cb), seg.cb_mult, seg.cb_luma_mult, seg.cb_offset),
                (2, len(seg.scaling_points_cr), seg.cr_mult, seg.cr_luma_mult, seg.cr_offset)):
            if not (npts > 0 or csfl):
                continue
            orig = planes[plane].astype(np.int64)
            if csfl:
                merged = average_luma
            else:
                combined = average_luma * (luma_mult - 128) + orig * (mult - 128)
                merged = np.clip((combined >> 6) + ((offset - 256) << (bit_depth - 8)), 0, (1 << bit_depth) - 1)
            n = round2(scale_lut(luts[plane], merged, bit_depth) * noise[plane], shift)
            out[plane] = np.clip(orig + n, min_value, max_chroma).astype(planes[plane].dtype)
    if len(seg.scaling_points_y) > 0:
        n = round2(scale_lut(luts[0], in_y, bit_depth) * noise[0], shift)
        out[0] = np.clip(in_y + n, min_value, max_luma).astype(planes[0].dtype)
    return out
