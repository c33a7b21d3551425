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


# ---- the grid of the three level kernels: what tests/test_gpu_denoise_levels_grid.py runs on the device and what
# tests/test_denoise_levels_grid_cpu.py shows, on the reference alone, to occupy the grid it claims --------------------------------
TILE_COARSE = (256, 8)  # coarse samples a workgroup of kd_down / kd_lowres / kd_add covers (kTileW x kTileRows of levels_row.hip.h)
TILE_FINE = (2 * TILE_COARSE[0], 2 * TILE_COARSE[1])


def tiles(w: int, h: int, level: int = 0) -> Tuple[int, int]:
    """(tile columns, tile rows) of the three kernels of level `level` on a plane of w x h samples at level 0."""
    for _ in range(level):
        w, h = (w + 1) >> 1, (h + 1) >> 1
    return -(-w // TILE_FINE[0]), -(-h // TILE_FINE[1])


def _grid_case(name, w, h, bd, ss, seed, level0, level1, *, n=1, sigma=12.0, h8=12.0, Ks=(1, 2), batch=0, fewer=False, **form):
    return dict(name=name, w=w, h=h, bd=bd, ss=ss, seed=seed, n=n, sigma=sigma, h8=h8, Ks=Ks, batch=batch, level0=level0, level1=level1, fewer=fewer, form=form)


def grid_cases() -> List[dict]:
    """The fixed cases.  level0 / level1: (tile columns, tile rows) of the luma and of a chroma plane that the case is there for;
    fewer: workgroups counted on the luma plane find no chroma plane under them.  form: D, joint, gain, curve (flags; grid_kw()
    makes the arguments).  sigma, h8 (the strength at 8 bits) and seed are chosen so that every tile of every plane has something
    to do at K = 1 and at K = 2 (tests/test_denoise_levels_grid_cpu.py asserts it): at grainy()'s and the filter's defaults
    the corner tiles of one and of six samples come out of a level unchanged for most seeds."""
    return [
        _grid_case("420 3 x 3", 1040, 36, 10, "420", 70, [(3, 3), (2, 2)], [(2, 2), (1, 1)], fewer=True),
        _grid_case("422 thin column", 1026, 35, 8, "422", 70, [(3, 3), (2, 3)], [(2, 2), (1, 2)], fewer=True),
        _grid_case("444 corner sample", 1025, 33, 10, "444", 70, [(3, 3), (3, 3)], [(2, 2), (2, 2)]),
        _grid_case("mono 2 x 2", 1024, 32, 12, "mono", 70, [(2, 2)], [(1, 1)]),
        _grid_case("mono one short", 1023, 31, 8, "mono", 70, [(2, 2)], [(1, 1)]),
        _grid_case("420 clip", 1040, 36, 8, "420", 70, [(3, 3), (2, 2)], [(2, 2), (1, 1)], n=3, batch=2, fewer=True, D=1),
        _grid_case("420 joint", 1026, 34, 10, "420", 70, [(3, 3), (2, 2)], [(2, 2), (1, 1)], fewer=True, joint=True),
        _grid_case("420 joint gain", 1026, 34, 10, "420", 70, [(3, 3), (2, 2)], [(2, 2), (1, 1)], fewer=True, joint=True, gain=True),
        _grid_case("mono curve", 1025, 33, 10, "mono", 70, [(3, 3)], [(2, 2)], curve=True),
        _grid_case("420 views 8", 1040, 36, 8, "420", 70, [(3, 3), (2, 2)], [(2, 2), (1, 1)], fewer=True),
        _grid_case("420 views 10", 1040, 36, 10, "420", 70, [(3, 3), (2, 2)], [(2, 2), (1, 1)], fewer=True),
        _grid_case("420 wide", 2050, 20, 8, "420", 70, [(5, 2), (3, 1)], [(3, 1), (2, 1)], Ks=(2,), fewer=True),
    ]


def grid_case(name: str) -> dict:
    return next(c for c in grid_cases() if c["name"] == name)


def grid_frames(case: dict) -> List[List[np.ndarray]]:
    return grainy(case["n"], case["w"], case["h"], case["bd"], case["ss"], seed=case["seed"], sigma=case["sigma"])


def grid_kw(case: dict, K: int) -> dict:
    """The denoiser's / the reference's arguments of a case at K levels: A = 1, S = 1."""
    form = case["form"]
    kw = dict(K=K, h=case["h8"], A=1, S=1)
    if form.get("D"):
        kw["D"] = form["D"]
    if form.get("joint"):
        kw["joint"] = True
    if form.get("gain"):
        from tests.test_gpu_denoise_gain import steep_gain

        kw["gain"] = steep_gain()
    if form.get("curve"):
        from tests.test_gpu_denoise_curve import curve

        kw["curve"] = curve("example", case["bd"])
    return kw
