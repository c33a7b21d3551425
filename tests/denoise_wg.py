"""tests/denoise_wg_host.cpp -- the tile functions of denoise_tile.hip.h on a host workgroup -- for the tests that run it:
how it is built, and one run of every tile of a frame."""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "denoise_wg_host.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = dict(ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def compiler():
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def build(exe, flags=SANITIZE, static="-static-libasan"):
    cmd = [compiler(), "-std=c++17", "-O1", "-g", *flags, "-o", str(exe), SOURCE]
    # (the sanitizer's runtime inside the program where the compiler can do that: it then starts under any preloaded library)
    if subprocess.call(cmd + [static], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)


def command(exe, kind, bps, S, A, q, w, h, xdec, ydec, nnb, table, inp, out, schedule="ascending", seed=0, fill="zero", skip=-1):
    """The program's argument list (its header comment): w x h is the plane, or the luma plane of a joint kind."""
    return [str(a) for a in (exe, kind, bps, S, A, q, w, h, xdec, ydec, nnb, table, inp, out, schedule, seed, fill, skip)]


def run_tiles(exe, kind, frames, present, xdec, ydec, A, S, T, q, timeout=600):
    """Every tile of frames[0] -- a list of planes: [plane] for tile / tile_t, [Y, Cb, Cr] for tile_j / tile_jt -- with the
    neighbours frames[1:] (present[k]: takes part), threads ascending, LDS zeroed: the bytes the program wrote."""
    d = exe.parent
    (d / "t.bin").write_bytes(np.asarray(T, np.uint16).tobytes())
    (d / "in.bin").write_bytes(b"".join(p.tobytes() for p in frames[0])
                               + b"".join(bytes([int(ok)]) + b"".join(p.tobytes() for p in f) for ok, f in zip(present, frames[1:])))
    h, w = frames[0][0].shape
    cmd = command(exe, kind, frames[0][0].dtype.itemsize, S, A, q, w, h, xdec, ydec, len(frames) - 1, d / "t.bin", d / "in.bin", d / "out.bin")
    p = subprocess.run(cmd, env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (" ".join(cmd), p.stderr[-3000:])
    return (d / "out.bin").read_bytes()
