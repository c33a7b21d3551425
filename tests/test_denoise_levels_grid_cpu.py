"""The grid cases of tests/test_gpu_denoise_levels_grid.py bite, shown without a device on tests/denoise_levels_ref.py alone: the
tile the cases are sized by is the tile of levels_row.hip.h, every case puts on the grid of kd_down, kd_lowres and kd_add what
tests/denoise_levels_content.py's grid_cases() says it does, and on the very frames the device file uses no tile of any plane is
idle: a level changes at least one sample of every tile, so a tile that a kernel skipped or put elsewhere cannot pass there."""
from __future__ import annotations

import functools
import os
import re

import numpy as np
import pytest

from tests import denoise_levels_content as LC
from tests import denoise_levels_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = LC.grid_cases()
NAMES = [c["name"] for c in CASES]


def test_the_tile_is_the_kernels():
    text = open(os.path.join(ROOT, "grav1synth_amd", "csrc", "levels_row.hip.h")).read()

    def constant(name):
        found = re.findall(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, text)
        assert len(found) == 1, (name, found)
        return int(found[0])

    lane, lanes, rows = constant("kLaneCoarse"), constant("kTileLanes"), constant("kTileRows")
    assert re.search(r"\bkTileW\s*=\s*kTileLanes\s*\*\s*kLaneCoarse\s*;", text) and re.search(r"\bkThreads\s*=\s*kTileLanes\s*\*\s*kTileRows\s*;", text)
    assert (lane * lanes, rows) == (256, 8) == LC.TILE_COARSE and LC.TILE_FINE == (512, 16)
    assert LC.tiles(512, 16) == (1, 1) and LC.tiles(513, 17) == (2, 2) and LC.tiles(1025, 33, 1) == (2, 2) and LC.tiles(1024, 32, 1) == (1, 1)


def test_the_case_list_is_the_issue_s():
    assert len(set(NAMES)) == len(NAMES) == 12
    sizes = {(c["w"], c["h"], c["bd"], c["ss"]) for c in CASES}
    assert sizes == {(1040, 36, 10, "420"), (1026, 35, 8, "422"), (1025, 33, 10, "444"), (1024, 32, 12, "mono"), (1023, 31, 8, "mono"), (1040, 36, 8, "420"),
                     (1026, 34, 10, "420"), (1025, 33, 10, "mono"), (2050, 20, 8, "420")}
    assert all(c["Ks"] == ((2,) if c["w"] == 2050 else (1, 2)) for c in CASES)
    clip = LC.grid_case("420 clip")
    assert (clip["n"], clip["batch"], clip["form"]) == (3, 2, dict(D=1)) and all(c["n"] == 1 and c["batch"] == 0 for c in CASES if c["name"] != "420 clip")
    assert [c["name"] for c in CASES if c["form"].get("joint")] == ["420 joint", "420 joint gain"] and LC.grid_case("420 joint gain")["form"]["gain"]
    assert [c["name"] for c in CASES if c["form"].get("curve")] == ["mono curve"]
    for c in CASES:
        kw = LC.grid_kw(c, 2)
        assert (kw["K"], kw["A"], kw["S"]) == (2, 1, 1)


@pytest.mark.parametrize("name", NAMES)
def test_a_case_has_the_grid_it_claims(name):
    c = LC.grid_case(name)
    planes = LC.shapes(c["w"], c["h"], c["ss"])
    assert [p.shape[::-1] for p in LC.grid_frames(c)[0]] == planes, "the frames are of these shapes"
    for level, claimed in ((0, c["level0"]), (1, c["level1"])):
        got = [LC.tiles(pw, ph, level) for pw, ph in planes[:2]]
        assert got == claimed, (level, got, claimed)
    lx, ly = c["level0"][0]
    assert lx >= 2 and ly >= 2, "more than one tile column and more than one tile row at once at level 0"
    if c["fewer"]:
        cx, cy = c["level0"][1]
        assert (cx < lx or cy < ly) and cx <= lx and cy <= ly, "workgroups counted on the luma plane leave a chroma plane"
    # what each row of the table is there for
    l1x, l1y = c["level1"][0]
    if name in ("420 3 x 3", "420 clip", "420 views 8", "420 views 10"):
        assert c["level0"] == [(3, 3), (2, 2)] and (l1x, l1y) == (2, 2), "chroma is left sideways and downwards; level 1 has 2 x 2"
        assert c["w"] % 512 and c["h"] % 16, "the last tiles are partial both ways"
    elif name == "422 thin column":
        assert c["w"] - 1024 == 2 and c["level0"][1] == (2, 3) and c["h"] & 1, "a last tile column of one coarse sample; chroma 2 x 3; odd H"
    elif name in ("444 corner sample", "mono curve"):
        assert (c["w"] - 1024, c["h"] - 32) == (1, 1), "the corner tile is one fine sample"
    elif name == "mono 2 x 2":
        assert (c["w"], c["h"]) == (1024, 32) and (l1x, l1y) == (1, 1), "exactly 2 x 2 tiles; level 1 exactly one"
    elif name == "mono one short":
        assert (c["w"], c["h"]) == (1023, 31) and (l1x, l1y) == (1, 1)
    elif name == "420 wide":
        assert lx == 5 and l1x == 3 and ((c["w"] + 1) >> 1) - 1024 == 1, "level 1 three tiles wide with a last column of one sample"


@functools.lru_cache(maxsize=None)
def references(name):
    """K -> the reference's clip for K = 0, 1, 2, on the frames the device file uses"""
    c = LC.grid_case(name)
    frames = LC.grid_frames(c)
    return {K: LR.denoise_clip(frames, *LC.SUB[c["ss"]], c["bd"], **dict(LC.grid_kw(c, K), rho=1.0)) for K in (0, 1, 2)}


def idle_tiles(a_clip, b_clip, tw, th):
    """(frame, plane, tile column, tile row) of every tw x th tile in which the two clips do not differ"""
    out = []
    for t, (fa, fb) in enumerate(zip(a_clip, b_clip)):
        assert len(fa) == len(fb)
        for c, (a, b) in enumerate(zip(fa, fb)):
            differ = np.asarray(a) != np.asarray(b)
            H, W = differ.shape
            out += [(t, c, tx, ty) for ty in range(-(-H // th)) for tx in range(-(-W // tw)) if not differ[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].any()]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_no_tile_is_idle(name):
    """K = 1 differs from K = 0 in every 512 x 16 tile of every plane of every frame, K = 2 from K = 1 in every 1024 x 32 footprint
    of a tile of level 1"""
    ref = references(name)
    tw, th = LC.TILE_FINE
    assert len(ref[0]) == LC.grid_case(name)["n"]
    idle = idle_tiles(ref[0], ref[1], tw, th)
    assert not idle, f"{name}: level 0's tiles (frame, plane, column, row) that K = 1 leaves as K = 0 has them: {idle}"
    idle = idle_tiles(ref[1], ref[2], 2 * tw, 2 * th)
    assert not idle, f"{name}: level 1's tiles (frame, plane, column, row) that K = 2 leaves as K = 1 has them: {idle}"


def test_the_condition_can_fail():
    """a tile of K = 1's clip put back to what K = 0 has there, and the one-sample corner tile, are found, and nothing else"""
    ref = references("444 corner sample")
    skipped = [[p.copy() for p in f] for f in ref[1]]
    skipped[0][2][16:32, 512:1024] = ref[0][0][2][16:32, 512:1024]
    skipped[0][0][32, 1024] = ref[0][0][0][32, 1024]
    assert idle_tiles(ref[0], skipped, *LC.TILE_FINE) == [(0, 0, 2, 2), (0, 2, 1, 1)]
    assert idle_tiles(ref[1], ref[1], 1024, 32) == [(0, c, tx, ty) for c in range(3) for ty in range(2) for tx in range(2)]
