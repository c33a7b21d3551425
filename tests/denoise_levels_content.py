"""Content for the coarse-level tests of `denoise` (rules 25 - 29): what tests/test_gpu_denoise_levels.py feeds the device, and
what tests/test_denoise_levels_cpu.py shows the wrong restatements of tests/denoise_levels_ref.py on (test infrastructure).

grainy(): a textured world that moves a little from frame to frame, with correlated grain -- white noise through a 3 x 3 box
-- on every plane, so that a coarse level has something to remove.  checker(): cells of 0 and the largest code value with
scattered samples near both ends, where a coarse correction pushes the sum below 0 and above 2^B - 1.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from tests import motion_content as MC

SUB = {"mono": (1, 1), "420": (1, 1), "422": (1, 0), "444": (0, 0)}
SLOW = [(2, 1), (-1, 2), (1, -2), (2, 2), (-2, -1), (1, 1)]  # within the search radius: the temporal forms without motion


def shapes(w: int, h: int, ss: str) -> List[Tuple[int, int]]:
    if ss == "mono":
        return [(w, h)]
    sx, sy = SUB[ss]
    return [(w, h)] + [((w + sx) >> sx, (h + sy) >> sy)] * 2


def correlated(rng, w: int, h: int, sigma: float) -> np.ndarray:
    """Grain of standard deviation sigma: a 3 x 3 box filter of white noise."""
    n = rng.standard_normal((h + 2, w + 2))
    s = sum(n[j:j + h, i:i + w] for j in range(3) for i in range(3)) / 3.0
    return sigma * s


def grainy(n: int, w: int, h: int, bd: int, ss: str, seed: int = 0, sigma: float = 5.0, shifts: Sequence[Tuple[int, int]] = SLOW) -> List[List[np.ndarray]]:
    top, scale = (1 << bd) - 1, 1 << (bd - 8)
    per_plane = []
    for c, (pw, ph) in enumerate(shapes(w, h, ss)):
        use = [shifts[t % len(shifts)] for t in range(n - 1)]
        clean = MC.pan([seed, c, w, h], pw, ph, bd, use, 0.0, "texture")[0]
        rng = np.random.default_rng([seed, c, 91])
        per_plane.append([np.clip(np.rint(p.astype(np.float64) + correlated(rng, pw, ph, sigma * scale)), 0, top).astype(MC.dtype_of(bd)) for p in clean])
    return MC.clip(per_plane)


def checker(w: int, h: int, bd: int, seed: int = 0, cell: int = 3) -> List[List[np.ndarray]]:
    """One luma-only frame."""
    top = (1 << bd) - 1
    rng = np.random.default_rng([seed, w, h])
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.where(((xx // cell) + (yy // cell)) & 1, top, 0).astype(np.int64)
    near = rng.integers(0, 40 << (bd - 8), (h, w))
    p = np.where(rng.random((h, w)) < 0.3, np.where(p == 0, near, top - near), p)
    return [[p.astype(MC.dtype_of(bd))]]


# the cases both files name: (frames, bit depth, subsampling, the denoiser's / the reference's arguments)
def basic():
    return grainy(1, 65, 49, 8, "mono", seed=1), 8, "mono", dict(K=1)


def clipping():
    return checker(66, 50, 8, seed=2), 8, "mono", dict(K=1, h=10.0, rho=4.0)


def with_curve():
    from tests.test_gpu_denoise_curve import curve

    return grainy(1, 65, 49, 10, "mono", seed=3), 10, "mono", dict(K=1, curve=curve("example", 10))


def panned(mr: int):
    from tests.test_gpu_denoise_motion import panned as pan

    # (pans of mr + 4 samples: 5 or 6 on the coarse plane, beyond Mr' = 4 and within Mr, so a range that is not halved finds them)
    return pan(3, 129, 97, 8, "mono", seed=4 + mr, shifts=[(mr + 4, -2), (-4, mr + 4)], sigma=3.0, kind="texture"), 8, "mono", dict(K=1, D=1, mr=mr)


def ratio(rho: float, K: int = 1):
    return grainy(1, 65, 49, 10, "420", seed=5), 10, "420", dict(K=K, rho=rho)


def joint(gain: bool = False):
    kw = dict(K=1, joint=True)
    if gain:
        from tests.test_gpu_denoise_gain import steep_gain

        kw["gain"] = steep_gain()
    # (4:2:2: at 4:2:0 rule 8's box is rule 16's, and the guide of the coarse luma is the box of the fine guide, sample for sample)
    return grainy(1, 65, 49, 10, "422", seed=6), 10, "422", kw
