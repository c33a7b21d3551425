"""The joint denoise tiles under a chroma gain (rules 21 - 24) with their real barriers, without a device: the gain
instantiations of dn_tile_j, dn_tile_jt and dn_tile_jtm of denoise_tile.hip.h -- what the three forms of kd_nlm_j<.., GainArg>
call -- run unmodified on a host workgroup (tests/wg_host.h, tests/denoise_gain_wg_host.cpp), as
tests/test_denoise_schedule_cpu.py runs the tiles without a gain.  The program holds rule 24 as a plain loop over pairs and
counts the samples that differ from it; the numpy restatement (tests/denoise_gain_ref.py) is compared with its bytes too.

* Under every committed schedule and fill no sample differs and the barrier count is the one of the tiles without a gain:
  the gain table is staged in front of the first weight phase, under the barrier that was there, and no barrier was lost.
* Every barrier is still load-bearing: with one sync() call made a no-op, some (schedule, fill) pair shows it.
* ThreadSanitizer over free-running threads finds only the documented overlapping stores of equal values.

Built with the host compiler under -fsanitize=address,undefined (and -fsanitize=thread); nothing is loaded into Python."""
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

from tests import denoise_gain_ref as G
from tests import denoise_joint_ref as J
from tests.denoise_gain_wg import ENV, SOURCE, build as _build, command, compiler as _compiler
from tests.test_denoise_schedule_cpu import ALLOWED_WRITE_WRITE, FILLS, PROBE, SCHEDULES, SEED, STRENGTH, SUB, TIMEOUT, TSAN_ENV, parse_tsan


def step_gain(level):
    """4 below a luma level (of the gain's 256), 16384 from it on: rule 21's two ends side by side."""
    return np.where(np.arange(256) < level, 4, 16384).astype(np.uint16)


def random_gain(seed):
    """256 values in 1 .. 16384, uniform in their logarithm: as many below the flat gain's 256 as above it, so that on
    full-range noise the weights stay spread over the table and a wrong byte in LDS shows in the output."""
    return np.rint(np.exp(np.random.default_rng(seed).uniform(0.0, np.log(16384.0), 256))).astype(np.uint16)


class Case:
    """One frame [Y, Cb, Cr] under `ss`, its neighbours and, for tile_jtm, a vector a tile and neighbour; seeded noise over
    the full sample range."""

    def __init__(self, kind, bd, w, h, A, S, gain, present=(), ss="420", seed=0):
        self.kind, self.bd, self.w, self.h, self.A, self.S, self.present, self.ss, self.seed = kind, bd, w, h, A, S, tuple(present), ss, seed
        self.gain = np.asarray(gain, np.uint16)
        self.gain.setflags(write=False)
        self.xdec, self.ydec = SUB[ss]
        assert kind in ("tile_j", "tile_jt", "tile_jtm") and (kind != "tile_j" or not present)

    @property
    def id(self):
        nb = "-nb" + "".join("01"[p] for p in self.present) if self.present else ""
        return f"{self.kind}-{self.bd}bit-{self.ss}-chroma{self.cw}x{self.ch}-A{self.A}S{self.S}{nb}-content{self.seed}"

    @property
    def cw(self):
        return (self.w + self.xdec) >> self.xdec

    @property
    def ch(self):
        return (self.h + self.ydec) >> self.ydec

    @property
    def tiles(self):
        return -(-self.cw // 64) * -(-self.ch // 48)

    def frames(self):
        dt = np.uint8 if self.bd == 8 else np.uint16
        shapes = [(self.h, self.w), (self.ch, self.cw), (self.ch, self.cw)]
        rng = np.random.default_rng([self.seed, self.w, self.h, self.bd])
        return [[rng.integers(0, 1 << self.bd, s).astype(dt) for s in shapes] for _ in range(1 + len(self.present))]

    def vectors(self):
        """(neighbours, tiles, 2) int8, even, up to 20 samples either way: past the halo, and for small planes past the plane."""
        if self.kind != "tile_jtm":
            return None
        return (2 * np.random.default_rng([self.seed, 99]).integers(-10, 11, (len(self.present), self.tiles, 2))).astype(np.int8)

    def table(self):
        from grav1synth_amd.denoise import weight_table

        return weight_table(self.bd, self.S, STRENGTH, joint_chroma=True)

    def blob(self):
        fr = self.frames()
        mv = self.vectors()
        return (b"".join(p.tobytes() for p in fr[0]) + b"".join(bytes([int(ok)]) + b"".join(p.tobytes() for p in f) for ok, f in zip(self.present, fr[1:]))
                + (mv.tobytes() if mv is not None else b""))

    def reference(self):
        """tests/denoise_gain_ref.py on the frame and the neighbours that take part, each with its vectors."""
        fr = self.frames()
        T, q = self.table()
        mv = self.vectors()
        us = J._triple(fr[0], self.xdec, self.ydec)
        (nb, nr), den = G.sums(us, None, None, self.A, self.S, T, q, self.gain, self.bd - 8)
        for k, (ok, f) in enumerate(zip(self.present, fr[1:])):
            if not ok:
                continue
            field = None if mv is None else mv[k].astype(np.int64).reshape(-(-self.ch // 48), -(-self.cw // 64), 2)
            (b, r), d = G.sums(us, J._triple(f, self.xdec, self.ydec), field, self.A, self.S, T, q, self.gain, self.bd - 8)
            nb, nr, den = nb + b, nr + r, den + d
        return np.stack([((x + (den >> 1)) // den).astype(fr[0][1].dtype) for x in (nb, nr)])

    def sync_calls(self):
        """{site: [call numbers]} and the total: the tiles without a gain have the same (tests/test_denoise_schedule_cpu.py)."""
        n_sp, n_t = self.A + self.A * (2 * self.A + 1), (2 * self.A + 1) ** 2
        sites = {"after staging": [0], "after dn_hsum": [1 + 2 * i for i in range(n_sp)], "after dn_weights": [2 + 2 * i for i in range(n_sp)]}
        total = 1 + 2 * n_sp
        if self.kind != "tile_j":
            names = ["in front of staging N", "after staging N", "after dn_hsum_t", "after dn_weights_t"]
            for nm in names:
                sites[nm] = []
            for _ in range(sum(self.present)):
                sites[names[0]].append(total)
                sites[names[1]].append(total + 1)
                sites[names[2]] += [total + 2 + 2 * i for i in range(n_t)]
                sites[names[3]] += [total + 3 + 2 * i for i in range(n_t)]
                total += 2 + 2 * n_t
        return sites, total


@functools.lru_cache(maxsize=None)
def _reference(case):
    ref = case.reference()
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def wg_host(tmp_path_factory):
    if _compiler() is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("gain_wg")
    exe = d / "denoise_gain_wg_host"
    _build(exe)
    written, lock, serial = {}, threading.Lock(), itertools.count()

    def run(case, schedule, fill, skip=-1, seed=SEED, program=exe, env=ENV):
        """(samples that differ from the program's plain loop, output as the reference shapes it, the process)"""
        with lock:
            if written.get("case") is not case:
                (d / "t.bin").write_bytes(np.asarray(case.table()[0], np.uint16).tobytes())
                (d / "g.bin").write_bytes(case.gain.tobytes())
                (d / "in.bin").write_bytes(case.blob())
                written["case"] = case
            out = d / f"out{next(serial)}.bin"
        cmd = command(program, case.kind, 1 if case.bd == 8 else 2, case.S, case.A, case.table()[1], case.w, case.h, case.xdec, case.ydec,
                      len(case.present), case.bd - 8, d / "t.bin", d / "g.bin", d / "in.bin", out, schedule, seed, fill, skip)
        p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=TIMEOUT)
        if skip >= 0 and p.returncode == 1 and "runtime error:" in p.stderr:
            return None, None, p  # without the barrier a phase read stale LDS, and the arithmetic on it was the sanitizer's
        assert p.returncode == 0, (" ".join(cmd), p.stderr[-3000:])
        m = re.fullmatch(r"syncs (\d+) tiles (\d+) differ (\d+)\n", p.stdout)
        assert m, p.stdout
        assert (int(m.group(1)), int(m.group(2))) == (case.sync_calls()[1], case.tiles), (p.stdout, case.sync_calls()[1], case.tiles)
        dt = np.uint8 if case.bd == 8 else np.uint16
        got = np.frombuffer(out.read_bytes(), dt).reshape(2, case.ch, case.cw)
        out.unlink()
        return int(m.group(3)), got, p

    def fills(case, schedule, skip=-1):
        with concurrent.futures.ThreadPoolExecutor(len(FILLS)) as pool:
            return dict(zip(FILLS, pool.map(lambda f: run(case, schedule, f, skip)[:2], FILLS)))

    run.exe, run.fills = exe, fills
    return run


def _cases():
    c = []
    # chroma 70 x 30 from 4:2:0 with odd luma sizes: two tiles, the second partial.  The step gain's level (128 of 256) lies in the
    # middle of full-range noise, so both values and their mean occur in every tile, at both ends of the half-plane walk
    c += [Case("tile_j", 8, 139, 59, 3, 2, step_gain(128), seed=71), Case("tile_j", 12, 139, 59, 3, 2, random_gain(1), seed=72),
          Case("tile_j", 10, 70, 50, 1, 1, random_gain(2), ss="444", seed=73), Case("tile_j", 10, 129, 49, 2, 4, step_gain(7), ss="422", seed=74),
          Case("tile_j", 12, 5, 3, 3, 2, random_gain(3), seed=75), Case("tile_j", 8, 139, 59, 7, 4, random_gain(4), seed=76)]
    c += [Case("tile_jt", 10, 139, 59, 3, 2, random_gain(5), (1, 0, 1), seed=81), Case("tile_jt", 8, 139, 99, 1, 2, step_gain(200), (1, 1), seed=82),
          Case("tile_jt", 12, 139, 59, 7, 1, random_gain(6), (1,), seed=83)]
    c += [Case("tile_jtm", 8, 139, 59, 3, 2, random_gain(7), (1, 1), seed=91), Case("tile_jtm", 12, 139, 99, 2, 1, step_gain(100), (0, 1, 1), seed=92),
          Case("tile_jtm", 10, 20, 12, 3, 2, random_gain(8), (1, 1), seed=93)]
    return c


CASES = _cases()


@pytest.mark.parametrize("schedule", SCHEDULES, ids=[f"{s}-seed{SEED}" for s in SCHEDULES])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_the_gain_tiles_give_the_plain_loop_under_every_schedule_and_fill(wg_host, case, schedule):
    """Every tile of the plane, 256 threads and the real barriers: no sample differs from the program's own plain loop over
    pairs, and the bytes are those of tests/denoise_gain_ref.py, whatever the order of the threads between two barriers and
    whatever the tile finds in LDS -- the gain table's 512 bytes included, which only the first barrier stands behind."""
    want = _reference(case)
    for fill, (differ, got) in wg_host.fills(case, schedule).items():
        assert differ == 0, (fill, differ)
        assert np.array_equal(got, want), (fill, np.argwhere(got != want)[:5])


def test_the_gain_does_something_and_the_flat_gain_nothing(wg_host):
    """The same content under the flat gain is tests/denoise_joint_ref.py's bytes; under the case's gain it is not."""
    case = CASES[0]
    flat = Case(case.kind, case.bd, case.w, case.h, case.A, case.S, G.FLAT, case.present, case.ss, case.seed)
    T, q = case.table()
    nb, nr, den = J.chroma_sums(case.frames(), 0, case.xdec, case.ydec, 0, case.A, case.S, T, q)
    plain = np.stack([((x + (den >> 1)) // den).astype(np.uint8) for x in (nb, nr)])
    differ, got, _p = wg_host(flat, "random", "random")
    assert differ == 0 and np.array_equal(got, plain)
    assert (_reference(case) != plain).any()


DROP_CASES = {
    "tile_j": Case("tile_j", 8, 139, 59, 3, 2, random_gain(11), seed=53),
    "tile_jt": Case("tile_jt", 8, 139, 59, 3, 2, random_gain(12), (1, 0, 1, 1), seed=54),
    "tile_jtm": Case("tile_jtm", 8, 139, 59, 3, 2, random_gain(13), (1, 0, 1, 1), seed=55),
}
# (as in tests/test_denoise_schedule_cpu.py: the barrier in front of staging the FIRST neighbour is not needed by the data flow)
NOT_NEEDED = {("tile_jt", "in front of staging N", 0), ("tile_jtm", "in front of staging N", 0)}
DROPS = [(k, site) for k, c in DROP_CASES.items() for site in c.sync_calls()[0]]


@pytest.mark.parametrize("kind,site", DROPS, ids=[f"{k}-{s.replace(' ', '_')}" for k, s in DROPS])
def test_a_dropped_barrier_still_shows_under_some_schedule_and_fill(wg_host, kind, site):
    """The k-th sync() call of every thread made a no-op: for the first, a middle and the last occurrence of the site, at
    least one committed (schedule, fill) pair gives samples that are not the plain loop's.  "after staging" is the barrier the
    gain table is staged under."""
    case = DROP_CASES[kind]
    calls = case.sync_calls()[0][site]
    for occ in sorted({0, len(calls) // 2, len(calls) - 1}):
        found = None
        for schedule in SCHEDULES:
            for fill, (differ, _got) in wg_host.fills(case, schedule, skip=calls[occ]).items():
                if found is None and differ:
                    found = (schedule, fill, differ)
            if found:
                break
        what = f"{kind:8s} {site:24s} occurrence {occ:3d} of {len(calls):3d} (sync call {calls[occ]:4d})"
        if (kind, site, occ) in NOT_NEEDED:
            assert found is None, f"{what}: marked as not needed by the data flow, and {found} sees it dropped"
        else:
            print(f"DROP {what}: {found[0]} / {found[1]}, {found[2]} samples differ" if found else f"DROP {what}: NOT SEEN")
            assert found is not None, f"{what}: no committed schedule and fill notices the barrier gone"


# ------------------------------------------------------------------------------------------------------ ThreadSanitizer
@pytest.fixture(scope="module")
def tsan_exe(tmp_path_factory):
    if _compiler() is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("gain_tsan")
    (d / "probe.cpp").write_text(PROBE)
    flags = ["-fsanitize=thread", "-pthread"]
    probe = d / "probe"
    for static in (["-static-libtsan"], []):
        b = subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", *flags, *static, "-o", str(probe), str(d / "probe.cpp")], capture_output=True, text=True)
        if b.returncode == 0:
            r = subprocess.run([str(probe)], capture_output=True, text=True, timeout=TIMEOUT)
            if r.returncode == 0 and "ThreadSanitizer" not in r.stderr:
                break
            why = f"the probe program ended with {r.returncode}: {r.stderr[-500:]}"
        else:
            why = f"the probe program did not build: {b.stderr[-500:]}"
    else:
        pytest.skip("ThreadSanitizer is not usable with the host compiler: " + why.splitlines()[0][:200])
    exe = d / "denoise_gain_wg_host_tsan"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", *flags, *static, "-DWG_FREE_RUNNING", "-o", str(exe), SOURCE])
    return exe


TSAN_CASES = [Case("tile_j", 8, 139, 99, 3, 2, random_gain(21), seed=63), Case("tile_jt", 8, 139, 99, 3, 2, random_gain(22), (1, 1), seed=64),
              Case("tile_jtm", 8, 139, 99, 3, 2, random_gain(23), (1, 1), seed=65)]


@pytest.mark.parametrize("case", TSAN_CASES, ids=[c.id for c in TSAN_CASES])
def test_thread_sanitizer_finds_only_the_overlapping_stores_of_equal_values(wg_host, tsan_exe, case):
    """256 free-running threads a tile and a plain barrier: every report is a data race between two WRITES whose phases are
    both in ALLOWED_WRITE_WRITE (tests/test_denoise_schedule_cpu.py).  The staging of the gain table and its reads in the
    weight phases are in no report."""
    differ, got, p = wg_host(case, "ascending", "random", program=tsan_exe, env=TSAN_ENV)
    assert differ == 0 and np.array_equal(got, _reference(case))
    reports = parse_tsan(p.stderr)
    assert p.stderr.count("WARNING: ThreadSanitizer") == len(reports)
    for kind, acc in reports:
        ok = kind == "data race" and len(acc) == 2 and all(rw == "write" and fn in ALLOWED_WRITE_WRITE for rw, fn in acc)
        assert ok, (kind, acc, p.stderr[-4000:])
