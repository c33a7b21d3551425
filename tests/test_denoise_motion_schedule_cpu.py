"""The motion tile functions with their real barriers, without a device: dn_motion_tile, dn_tile_tm and dn_tile_jtm of
denoise_tile.hip.h -- what kd_motion, kd_nlm<kMotion> and kd_nlm_j<kMotion> call -- run unmodified on a host workgroup (tests/wg_host.h,
tests/denoise_motion_wg_host.cpp) under the schedules and LDS fills of tests/test_denoise_schedule_cpu.py, against the numpy
reference of rules 16 - 20 (tests/denoise_motion_ref.py).  The search adds three barriers (after staging, after the threads'
keys, after the groups' keys); each is load-bearing, and some committed (schedule, fill) pair shows it.  The filter's tile
functions add none: their barriers are the ones that file checks."""
from __future__ import annotations

import concurrent.futures
import functools
import itertools
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from tests import denoise_motion_ref as MR
from tests import motion_content as MC
from tests.denoise_motion_wg import ENV, build as _build, command, compiler as _compiler
from tests.test_denoise_schedule_cpu import FILLS, SCHEDULES, SEED, STRENGTH, SUB, TIMEOUT


class Case:
    """A frame (a plane, or Y / Cb / Cr under `ss`) and its neighbours: a noise world panned by `shifts` (neighbour k is the
    window moved by shifts[k] from the frame's), independent full-range noise where a shift is None."""

    def __init__(self, kind, bd, w, h, M, shifts, present=None, ss=None, A=1, S=1, seed=0):
        self.kind, self.bd, self.w, self.h, self.M, self.shifts, self.ss, self.A, self.S, self.seed = kind, bd, w, h, M, tuple(shifts), ss, A, S, seed
        self.present = tuple(present) if present is not None else (1,) * len(shifts)
        self.joint = kind in ("search_j", "tile_jtm")
        self.xdec, self.ydec = SUB[ss]
        assert self.joint == (ss is not None)

    @property
    def id(self):
        size = f"{self.ss}-luma{self.w}x{self.h}" if self.joint else f"{self.w}x{self.h}"
        return f"{self.kind}-{self.bd}bit-{size}-M{self.M}-A{self.A}S{self.S}-nb{''.join('01'[p] for p in self.present)}-content{self.seed}"

    @property
    def cw(self):
        return (self.w + self.xdec) >> self.xdec

    @property
    def ch(self):
        return (self.h + self.ydec) >> self.ydec

    def frames(self):
        """[frame, neighbour 0, ...], a frame [plane] or [Y, Cb, Cr]"""
        shapes = [(self.w, self.h)] + ([(self.cw, self.ch)] * 2 if self.joint else [])
        rng = np.random.default_rng([self.seed, 99])
        per_plane = []
        for c, (w, h) in enumerate(shapes):
            live = [s for s in self.shifts if s is not None]
            xs, ys = [0] + [s[0] for s in live], [0] + [s[1] for s in live]
            wd = MC.world([self.seed, c], w + max(xs) - min(xs), h + max(ys) - min(ys), self.bd)
            cut = lambda s: wd[s[1] - min(ys):s[1] - min(ys) + h, s[0] - min(xs):s[0] - min(xs) + w]  # noqa: E731
            per_plane.append([cut((0, 0))] + [cut(s) if s is not None else rng.integers(0, 1 << self.bd, (h, w)) for s in self.shifts])
        return [[p.astype(MC.dtype_of(self.bd)) for p in f] for f in zip(*per_plane)]

    def table(self):
        from grav1synth_amd.denoise import weight_table

        return weight_table(self.bd, self.S, STRENGTH, joint_chroma=self.joint)

    def blob(self):
        fr = self.frames()
        return b"".join(p.tobytes() for p in fr[0]) + b"".join(bytes([int(ok)]) + b"".join(p.tobytes() for p in f) for ok, f in zip(self.present, fr[1:]))

    def fields(self):
        """the field towards every neighbour, zeros for one that takes no part"""
        fr = self.frames()
        pick = (lambda f: f[1:3]) if self.joint else (lambda f: f[0])
        out = [MR.search(pick(fr[0]), pick(f), 2 * self.M) for f in fr[1:]]
        return [v if ok else np.zeros_like(v) for ok, v in zip(self.present, out)]

    def reference(self):
        if self.kind in ("search", "search_j"):
            return np.stack(self.fields()).astype(np.int8)
        fr = self.frames()
        clip = [fr[0]] + [f for ok, f in zip(self.present, fr[1:]) if ok]
        T, q = self.table()
        n = len(clip) - 1
        # the clip [frame, the neighbours that take part], frame 0, a radius that takes them all in: the sums are exact
        if self.joint:
            return np.stack(MR.denoise_chroma_clip(clip, self.xdec, self.ydec, n, self.A, self.S, T, q, 2 * self.M)[0])
        return MR.denoise_plane_clip([f[0] for f in clip], n, self.A, self.S, T, q, 2 * self.M)[0]


@functools.lru_cache(maxsize=None)
def _reference(case):
    ref = case.reference()
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def wg_host(tmp_path_factory):
    if _compiler() is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("mwg")
    exe = d / "denoise_motion_wg_host"
    _build(exe)
    written, lock, serial = {}, threading.Lock(), itertools.count()

    def run(case, schedule, fill, skip=-1):
        with lock:
            if written.get("case") is not case:
                (d / "t.bin").write_bytes(np.asarray(case.table()[0], np.uint16).tobytes())
                (d / "in.bin").write_bytes(case.blob())
                written["case"] = case
            out = d / f"out{next(serial)}.bin"
        cmd = command(exe, case.kind, 1 if case.bd == 8 else 2, case.S, case.A, case.table()[1], case.w, case.h, case.xdec, case.ydec,
                      len(case.shifts), case.M, d / "t.bin", d / "in.bin", out, schedule, SEED, fill, skip)
        p = subprocess.run(cmd, env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=TIMEOUT)
        assert p.returncode == 0, (" ".join(cmd), p.stderr[-3000:])
        m = re.fullmatch(r"syncs (\d+) tiles (\d+)\n", p.stdout)
        assert m, p.stdout
        ref = _reference(case)
        got = np.frombuffer(out.read_bytes(), ref.dtype).reshape(ref.shape)
        out.unlink()
        return got, int(m.group(1)), int(m.group(2))

    def fills(case, schedule, skip=-1):
        with concurrent.futures.ThreadPoolExecutor(len(FILLS)) as pool:
            return dict(zip(FILLS, pool.map(lambda f: run(case, schedule, f, skip), FILLS)))

    run.fills = fills
    return run


def _cases():
    c = []
    # the search: three blocks with ragged ones and an odd plane (the search plane clamps), one block exactly, planes smaller than
    # a search-plane sample pair; the range at its ends; pans at the range, one step beyond it (not found: what the key then
    # picks is still the reference's) and of odd size; a neighbour that takes no part; unrelated noise (SAD near its ceiling)
    c += [Case("search", 8, 129, 97, 8, [(16, 0), (-6, 10), (5, -3)], seed=1), Case("search", 12, 129, 97, 1, [(2, -2), (4, 0)], seed=2),
          Case("search", 12, 65, 49, 32, [(64, -64), (-66, 2)], seed=3), Case("search", 8, 64, 48, 32, [(-64, 64), None], (1, 1), seed=4),
          Case("search", 12, 1, 1, 32, [None], seed=5), Case("search", 8, 2, 2, 1, [None, None], (0, 1), seed=6),
          Case("search", 12, 63, 47, 16, [(31, 16), None], (1, 0), seed=7)]
    c += [Case("search_j", 8, 129, 97, 8, [(6, -4), (-16, 16)], ss="444", seed=11), Case("search_j", 12, 131, 99, 32, [(10, 0), None], ss="420", seed=12),
          Case("search_j", 12, 139, 49, 4, [(-8, 2)], ss="422", seed=13)]
    # the filter under the vectors: two by two tiles, the far ones partial, the pan beyond the search radius; the parameter corners
    c += [Case("tile_tm", 8, 65, 49, 8, [(10, 0), (-10, 4)], A=3, S=2, seed=21), Case("tile_tm", 12, 70, 50, 32, [(40, -22), None], (1, 0), A=1, S=1, seed=22),
          Case("tile_tm", 12, 70, 30, 4, [(8, 8)], A=7, S=4, seed=23), Case("tile_tm", 8, 3, 2, 2, [None, None], A=3, S=2, seed=24),
          Case("tile_tm", 8, 70, 50, 16, [(-30, 20), (7, -5), None], (1, 1, 0), A=2, S=1, seed=25)]
    c += [Case("tile_jtm", 8, 129, 97, 8, [(10, 0), (-6, 4)], ss="420", A=3, S=2, seed=31), Case("tile_jtm", 12, 139, 59, 32, [(30, -12), None], (1, 0), "420", A=1, S=1, seed=32),
          Case("tile_jtm", 12, 129, 49, 4, [(-8, 2)], ss="422", A=2, S=4, seed=33), Case("tile_jtm", 8, 70, 50, 16, [(20, 14)], ss="444", A=1, S=2, seed=34)]
    return c


CASES = _cases()


@pytest.mark.parametrize("schedule", SCHEDULES, ids=[f"{s}-seed{SEED}" for s in SCHEDULES])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_the_motion_tile_functions_give_the_reference_under_every_schedule_and_fill(wg_host, case, schedule):
    want = _reference(case)
    blocks = -(-(case.cw if case.joint else case.w) // 64) * -(-(case.ch if case.joint else case.h) // 48)
    for fill, (got, syncs, tiles) in wg_host.fills(case, schedule).items():
        assert np.array_equal(got, want), (fill, np.argwhere(got != want)[:5], got.reshape(-1)[:8], want.reshape(-1)[:8])
        if case.kind.startswith("search"):
            assert (syncs, tiles) == (3 if any(case.present) else 0, blocks * sum(case.present))
        else:
            n_sp, n_t = case.A + case.A * (2 * case.A + 1), (2 * case.A + 1) ** 2
            assert (syncs, tiles) == (1 + 2 * n_sp + sum(case.present) * (2 + 2 * n_t), blocks), "the barriers of dn_tile_t / dn_tile_jt, no more"


def test_the_cases_hold_vectors_beyond_the_search_radius():
    """or the filter cases would pass with the vectors ignored"""
    for case in CASES:
        if case.kind.startswith("tile") and any(s is not None for s in case.shifts):
            assert max(int(np.abs(f).max()) for f in case.fields()) > case.A, case.id


DROP_CASES = {"search": Case("search", 8, 129, 97, 8, [(16, 0), (-6, 10)], seed=41), "search_j": Case("search_j", 8, 129, 97, 8, [(6, -4)], ss="444", seed=42)}
SITES = ["after staging", "after the threads' keys", "after the groups' keys"]


@pytest.mark.parametrize("site", range(3), ids=[s.replace(" ", "_").replace("'", "") for s in SITES])
@pytest.mark.parametrize("kind", list(DROP_CASES))
def test_a_dropped_barrier_of_the_search_shows_under_some_schedule_and_fill(wg_host, kind, site):
    """sync() call `site` of every thread made a no-op: at least one committed (schedule, fill) pair gives other vectors."""
    case = DROP_CASES[kind]
    want = _reference(case)
    found = None
    for schedule in SCHEDULES:
        for fill, (got, _s, _t) in wg_host.fills(case, schedule, skip=site).items():
            if found is None and not np.array_equal(got, want):
                found = (schedule, fill, int((got != want).sum()))
        if found:
            break
    print(f"DROP {kind:8s} {SITES[site]:24s}: " + (f"{found[0]} / {found[1]}, {found[2]} components differ" if found else "NOT SEEN"))
    assert found is not None, f"{kind}, {SITES[site]}: no committed schedule and fill notices the barrier gone"
