"""tests/denoise_gain_wg_host.cpp -- the gain instantiations of the joint tile functions of denoise_tile.hip.h on a host
workgroup, beside rule 24 as a plain loop -- for the tests that run it: how it is built, and its argument list.  A
stand-alone program: nothing of it is loaded into Python."""
from __future__ import annotations

import os
import subprocess

from tests.denoise_wg import ENV, SANITIZE, compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "denoise_gain_wg_host.cpp")

__all__ = ["ENV", "SANITIZE", "SOURCE", "build", "command", "compiler"]


def build(exe, flags=SANITIZE, static="-static-libasan"):
    cmd = [compiler(), "-std=c++17", "-O1", "-g", *flags, "-o", str(exe), SOURCE]
    # (the sanitizer's runtime inside the program where the compiler can do that: it then starts under any preloaded library)
    if subprocess.call(cmd + [static], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)


def command(exe, kind, bps, S, A, q, w, h, xdec, ydec, nnb, shift, table, gain, inp, out, schedule="ascending", seed=0, fill="zero", skip=-1):
    """The program's argument list (its header comment): w x h is the luma plane."""
    return [str(a) for a in (exe, kind, bps, S, A, q, w, h, xdec, ydec, nnb, shift, table, gain, inp, out, schedule, seed, fill, skip)]
