"""tests/denoise_motion_wg_host.cpp -- the motion tile functions of denoise_tile.hip.h on a host workgroup -- for the tests
that run it: how it is built (as tests/denoise_wg.py builds denoise_wg_host: a stand-alone program with the address and
undefined-behaviour sanitizers inside it), and its argument list."""
from __future__ import annotations

import os
import subprocess

from tests.denoise_wg import ENV, ROOT, SANITIZE, compiler  # noqa: F401  (ENV: what a run of the program gets)

SOURCE = os.path.join(ROOT, "tests", "denoise_motion_wg_host.cpp")


def build(exe, flags=SANITIZE, static="-static-libasan"):
    cmd = [compiler(), "-std=c++17", "-O1", "-g", *flags, "-o", str(exe), SOURCE]
    if subprocess.call(cmd + [static], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)


def command(exe, kind, bps, S, A, q, w, h, xdec, ydec, nnb, M, table, inp, out, schedule="ascending", seed=0, fill="zero", skip=-1):
    """The program's argument list (its header comment): w x h is the plane, or the luma plane of a joint kind."""
    return [str(a) for a in (exe, kind, bps, S, A, q, w, h, xdec, ydec, nnb, M, table, inp, out, schedule, seed, fill, skip)]
