"""The packed estimator's strip plan (grav1synth_amd/csrc/estimate_plan.h) without a device: k_estimate_pk's launch is cut
into row strips whose height comes from the plane, the batch, the device's compute units and the kernel's occupancy, so it
is the one work partition in the tree that the frame alone does not decide.  tests/estimate_plan_host.cpp walks the plan over
a grid of all five under the sanitizers; here its production heights against a restatement of the loop, which is also where
tests/test_gpu_estimate_strips.py takes the heights it pins from."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (width, height) of the production launches: batch 32 on 256 compute units
PRODUCTION = ((1920, 1080), (3840, 2160), (7680, 4320))
PRODUCTION_BATCH, PRODUCTION_CUS = 32, 256


def col_strips(w: int) -> int:
    return (w - 1 + 495) // 496


def plan_strips(h: int, cs: int, frames: int, cus: int, wgs_per_cu: int):
    """(strip_rows, row_strips, k): the loop of estimate_plan.h restated -- k rounds of `resident` waves, the smallest k whose
    strips are at most 256 rows; then at least 8 rows."""
    resident, cols, rows = cus * (wgs_per_cu if wgs_per_cu >= 1 else 5) * 4, cs * frames, h - 2
    k = next(k for k in range(1, 1 << 30) if -(-rows // max(1, k * resident // cols)) <= 256)
    r = max(8, -(-rows // max(1, k * resident // cols)))
    return r, -(-rows // r), k


def production_heights(wgs_per_cu: int = 8):
    """Strip heights of 1080p, 4K and 8K at batch 32 on 256 compute units."""
    return [plan_strips(h, col_strips(w), PRODUCTION_BATCH, PRODUCTION_CUS, wgs_per_cu)[0] for w, h in PRODUCTION]


def test_the_restatement_on_the_launches_worked_by_hand():
    """8 workgroups a unit: 8192 resident waves.  1080p: 4 x 32 column strips, 64 row strips a frame, ceil(1078 / 64) = 17.  4K:
    8 x 32, 32 row strips, ceil(2158 / 32) = 68.  8K: 16 x 32, 16 row strips of 270 rows are too tall: two rounds, 32 of 135."""
    assert [col_strips(w) for w in (16, 497, 498, 504, 1920, 3840, 7680, 65536)] == [1, 1, 2, 2, 4, 8, 16, 133]
    assert plan_strips(1080, 4, 32, 256, 8) == (17, 64, 1)
    assert plan_strips(2160, 8, 32, 256, 8) == (68, 32, 1)
    assert plan_strips(4320, 16, 32, 256, 8) == (135, 32, 2)
    assert production_heights() == [17, 68, 135]
    assert plan_strips(70, 2, 5, 256, 8) == (8, 9, 1) and plan_strips(3, 1, 1, 304, 0)[:2] == (8, 1)   # the small cases: always 8
    assert plan_strips(1080, 4, 32, 256, 0) == plan_strips(1080, 4, 32, 256, 5)                           # the fallback


def test_the_plan_holds_on_a_grid_and_gives_the_restatements_heights(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "estimate_plan_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tests", "estimate_plan_host.cpp")]
    # (the sanitizer's runtime inside the program where the compiler can do that: it then starts under any preloaded library)
    if subprocess.call(cmd + ["-static-libasan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok"
    assert lines[-2] == "points %d" % (5 * 603 * (5 * 4 * 9 + 14))
    got = {}
    for line in lines[:-2]:
        f = line.split()
        assert f[0] == "heights" and len(f) == 3 + 8, line
        got[(int(f[1]), int(f[2]))] = [tuple(int(v) for v in x.split(":")) for x in f[3:]]
    assert sorted(got) == sorted(PRODUCTION)
    for w, h in PRODUCTION:
        want = [plan_strips(h, col_strips(w), PRODUCTION_BATCH, PRODUCTION_CUS, occ) for occ in range(1, 9)]
        print(f"{w} x {h}, batch 32, 256 CUs, 1 .. 8 workgroups a CU: strip_rows {[x[0] for x in got[(w, h)]]} k {[x[2] for x in got[(w, h)]]}")
        assert got[(w, h)] == want, (w, h)
    assert [got[wh][7][0] for wh in PRODUCTION] == production_heights()
    assert max(x[2] for x in got[(7680, 4320)]) > 1, "the 8K launch takes the loop past its first round"
