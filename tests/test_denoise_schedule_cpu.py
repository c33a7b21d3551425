"""The denoise tiles with their real barriers, without a device: dn_tile, dn_tile_t, dn_tile_j and dn_tile_jt of
denoise_tile.hip.h -- what the four kernels call -- run unmodified on a host workgroup (tests/wg_host.h,
tests/denoise_wg_host.cpp) whose threads run one at a time between two barriers, in an order the test names, over LDS
filled with a pattern before every tile.

* The result is the numpy reference's under every committed schedule and every fill (a phase that reads what no thread
  of this tile has written, or what another thread has not written YET, shows as a byte).
* Every barrier is load-bearing and the schedules can see it: with one sync() call made a no-op, some (schedule, fill)
  pair gives other bytes.
* ThreadSanitizer over free-running threads, as a second opinion.

test_denoise_temporal_cpu.py and test_denoise_joint_cpu.py run the same program (tests/denoise_wg.py builds it for all
three) over their own content, threads ascending: there it is the arithmetic that is looked at, here the composition --
phase order, loop ranges, barrier placement."""
from __future__ import annotations

import concurrent.futures
import functools
import itertools
import os
import re
import subprocess
import threading
import time

import numpy as np
import pytest

from tests import denoise_joint_ref as J
from tests import denoise_ref as R
from tests import denoise_temporal_ref as TR
from tests.denoise_wg import ENV, SOURCE, build as _build, command, compiler as _compiler

SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0), None: (0, 0)}
SCHEDULES = ["ascending", "descending", "waves-reversed", "random", "stragglers"]
FILLS = ["zero", "ones", "random"]
SEED = 7          # of the schedules ("random", "stragglers") and of the random fill
STRENGTH = 60.0   # full-range noise: patch distances are large, and at h = 60 the weights are spread over the table
TIMEOUT = 120     # seconds a harness process gets; barrier divergence is a message and status 3, never a hang


class Case:
    """One frame (a plane, or Y / Cb / Cr under `ss`) and its neighbours, seeded noise over the full sample range."""

    def __init__(self, kind, bd, w, h, A, S, present=(), ss=None, seed=0):
        self.kind, self.bd, self.w, self.h, self.A, self.S, self.present, self.ss, self.seed = kind, bd, w, h, A, S, tuple(present), ss, seed
        self.joint = kind in ("tile_j", "tile_jt")
        self.xdec, self.ydec = SUB[ss]
        assert self.joint == (ss is not None) and (kind in ("tile_t", "tile_jt") or not present)

    @property
    def id(self):
        nb = "-nb" + "".join("01"[p] for p in self.present) if self.kind in ("tile_t", "tile_jt") else ""
        size = f"{self.ss}-chroma{self.cw}x{self.ch}-luma{self.w}x{self.h}" if self.joint else f"{self.w}x{self.h}"
        return f"{self.kind}-{self.bd}bit-{size}-A{self.A}S{self.S}{nb}-content{self.seed}"

    @property
    def cw(self):
        return (self.w + self.xdec) >> self.xdec

    @property
    def ch(self):
        return (self.h + self.ydec) >> self.ydec

    def frames(self):
        """[frame, neighbour 0, ...]: a frame is [plane] or [Y, Cb, Cr]; every neighbour has content, taking part or not."""
        dt = np.uint8 if self.bd == 8 else np.uint16
        shapes = [(self.h, self.w)] + ([(self.ch, self.cw)] * 2 if self.joint else [])
        rng = np.random.default_rng([self.seed, self.w, self.h, self.bd])
        return [[rng.integers(0, 1 << self.bd, s).astype(dt) for s in shapes] for _ in range(1 + len(self.present))]

    def table(self):
        from grav1synth_amd.denoise import weight_table

        return weight_table(self.bd, self.S, STRENGTH, joint_chroma=self.joint)

    def blob(self):
        fr = self.frames()
        return b"".join(p.tobytes() for p in fr[0]) + b"".join(bytes([int(ok)]) + b"".join(p.tobytes() for p in f) for ok, f in zip(self.present, fr[1:]))

    def reference(self):
        """The numpy references on the clip [frame, the neighbours that take part], frame 0, a radius that takes them all in:
        the sums are exact, so neither the order of the neighbours nor the side they are on shows."""
        fr = self.frames()
        clip = [fr[0]] + [f for ok, f in zip(self.present, fr[1:]) if ok]
        T, q = self.table()
        n = len(clip) - 1
        if self.joint:
            nb, nr, den = J.chroma_sums(clip, 0, self.xdec, self.ydec, n, self.A, self.S, T, q)
            return np.stack([((x + (den >> 1)) // den).astype(fr[0][1].dtype) for x in (nb, nr)])
        if self.kind == "tile":
            return R.denoise_plane(fr[0][0], self.A, self.S, T, q)
        num, den = TR.sums_plane([f[0] for f in clip], 0, n, self.A, self.S, T, q)
        return ((num + (den >> 1)) // den).astype(fr[0][0].dtype)

    # the sync() calls of a thread in a tile, numbered as they come: where each site of the phase sequence falls
    def spatial_offsets(self):
        return self.A + self.A * (2 * self.A + 1)

    def sync_calls(self):
        """{site: [call numbers]} in the order of the issue's list, and the total."""
        n_sp, n_t = self.spatial_offsets(), (2 * self.A + 1) ** 2
        t = self.kind in ("tile_t", "tile_jt")
        sites = {"after staging": [0], "after dn_hsum": [1 + 2 * i for i in range(n_sp)], "after dn_weights": [2 + 2 * i for i in range(n_sp)]}
        total = 1 + 2 * n_sp
        if t:
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
    d = tmp_path_factory.mktemp("wg")
    exe = d / "denoise_wg_host"
    _build(exe)
    written, lock, serial = {}, threading.Lock(), itertools.count()

    def run(case, schedule, fill, skip=-1, seed=SEED, program=exe, env=ENV):
        """(output as the reference shapes it, the process): every tile of the case on the workgroup executor."""
        with lock:
            if written.get("case") is not case:
                (d / "t.bin").write_bytes(np.asarray(case.table()[0], np.uint16).tobytes())
                (d / "in.bin").write_bytes(case.blob())
                written["case"] = case
            out = d / f"out{next(serial)}.bin"
        cmd = command(program, case.kind, 1 if case.bd == 8 else 2, case.S, case.A, case.table()[1], case.w, case.h, case.xdec, case.ydec,
                      len(case.present), d / "t.bin", d / "in.bin", out, schedule, seed, fill, skip)
        p = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=TIMEOUT)
        if skip >= 0 and p.returncode == 1 and "runtime error:" in p.stderr:
            return None, p  # without the barrier a phase read stale LDS, and the arithmetic on it was the sanitizer's
        assert p.returncode == 0, (" ".join(cmd), p.stderr[-3000:])
        m = re.fullmatch(r"syncs (\d+) tiles (\d+)\n", p.stdout)
        assert m, p.stdout
        tiles = -(-(case.cw if case.joint else case.w) // 64) * -(-(case.ch if case.joint else case.h) // 48)
        assert (int(m.group(1)), int(m.group(2))) == (case.sync_calls()[1], tiles), (p.stdout, case.sync_calls()[1], tiles)
        ref = _reference(case)
        got = np.frombuffer(out.read_bytes(), ref.dtype).reshape(ref.shape)
        out.unlink()
        return got, p

    def fills(case, schedule, skip=-1):
        """{fill: output} of one case under one schedule, the three processes side by side (None: see run)"""
        with concurrent.futures.ThreadPoolExecutor(len(FILLS)) as pool:
            return dict(zip(FILLS, pool.map(lambda f: run(case, schedule, f, skip)[0], FILLS)))

    run.exe, run.fills = exe, fills
    return run


# ------------------------------------------------------------------------------------------------------- the executor
def test_the_schedules_are_what_their_names_say(wg_host):
    def orders(name, seed, n=4):
        p = subprocess.run([str(wg_host.exe), "order", name, str(seed), str(n)], env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=TIMEOUT)
        assert p.returncode == 0, p.stderr[-2000:]
        o = [[int(x) for x in line.split()] for line in p.stdout.splitlines()]
        assert len(o) == n and all(sorted(i) == list(range(256)) for i in o), "every interval runs every thread once"
        return o

    up = list(range(256))
    assert all(i == up for i in orders("ascending", SEED))
    assert all(i == up[::-1] for i in orders("descending", SEED))
    assert all(i == up[192:] + up[128:192] + up[64:128] + up[:64] for i in orders("waves-reversed", SEED))
    r = orders("random", SEED)
    assert len({tuple(i) for i in r}) == 4 and up not in r, "a fresh permutation for every interval"
    assert r == orders("random", SEED) and r != orders("random", SEED + 1), "from the seed"
    s = orders("stragglers", SEED)
    late = s[0][192:]
    assert all(i == s[0] for i in s) and late == sorted(late) and s[0][:192] == sorted(set(up) - set(late)), "the same quarter, last in every interval"
    assert late != up[192:] and late != orders("stragglers", SEED + 1)[0][192:], "drawn from the seed"
    p = subprocess.run([str(wg_host.exe), "tile", "1", "1", "1", "0", "4", "4", "0", "0", "0", "x", "x", "x", "sideways", "1", "zero", "-1"],
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 2 and "unknown schedule" in p.stderr


@pytest.mark.parametrize("what", ["early-return", "extra-sync"])
def test_barrier_divergence_is_an_error_message_and_not_a_hang(wg_host, what):
    """Thread 7 returns while the others wait at a barrier; or calls sync() once more than they do."""
    t0 = time.monotonic()
    p = subprocess.run([str(wg_host.exe), "selftest", what], env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 3, (p.returncode, p.stderr[-2000:])
    assert "barrier divergence" in p.stderr and "thread 7" in p.stderr and "no divergence found" not in p.stdout
    assert time.monotonic() - t0 < 30


# ------------------------------------------------------------------- 3: neither the schedule nor stale LDS shows in a byte
def _cases():
    c = []
    for kind, nb in (("tile", ()), ("tile_t", (1, 1))):
        # 2 x 2 tiles, both far tiles partial; a plane smaller than the window
        c += [Case(kind, 8, 65, 49, 3, 2, nb, seed=11), Case(kind, 12, 70, 50, 3, 2, nb, seed=12), Case(kind, 12, 3, 2, 3, 2, nb, seed=13)]
        # the parameter corners ((3, 2) is above) on two tiles, the second partial; the first two in both sample widths.  With
        # neighbours, one of the two takes part at A = 7: 225 offsets a neighbour
        one = nb[:1] + (0,) * (len(nb) - 1)
        c += [Case(kind, 8, 70, 30, 1, 1, nb, seed=14), Case(kind, 12, 70, 30, 1, 1, nb, seed=15), Case(kind, 8, 70, 30, 7, 4, one, seed=16),
              Case(kind, 12, 70, 30, 7, 4, one, seed=17), Case(kind, 12, 70, 30, 7, 1, one, seed=18), Case(kind, 8, 70, 30, 1, 4, nb, seed=19)]
    for kind, nb in (("tile_j", ()), ("tile_jt", (1, 1))):
        one = nb[:1] + (0,) * (len(nb) - 1)
        # chroma 65 x 49 and 70 x 50 from 4:2:0 with odd luma width and height (the guide clamps); 4:2:2 and 4:4:4; chroma 3 x 2
        c += [Case(kind, 8, 129, 97, 3, 2, nb, "420", seed=21), Case(kind, 12, 139, 99, 3, 2, nb, "420", seed=22),
              Case(kind, 12, 129, 49, 3, 2, nb, "422", seed=23), Case(kind, 8, 70, 50, 3, 2, nb, "444", seed=24),
              Case(kind, 12, 5, 3, 3, 2, nb, "420", seed=25)]
        c += [Case(kind, 8, 139, 59, 1, 1, nb, "420", seed=26), Case(kind, 12, 139, 59, 1, 1, nb, "420", seed=27),
              Case(kind, 8, 139, 59, 7, 4, one, "420", seed=28), Case(kind, 12, 139, 59, 7, 4, one, "420", seed=29),
              Case(kind, 12, 139, 59, 7, 1, one, "420", seed=30), Case(kind, 8, 139, 59, 1, 4, nb, "420", seed=31)]
    for kind, ss, (w, h) in (("tile_t", None, (70, 50)), ("tile_jt", "420", (139, 99))):
        # neighbours: one of two absent, both absent, six present (A = 1), an absent one between two present ones
        c += [Case(kind, 12, w, h, 3, 2, (0, 1), ss, seed=41), Case(kind, 8, w, h, 3, 2, (0, 0), ss, seed=42),
              Case(kind, 12, w, h, 1, 2, (1, 1, 1, 1, 1, 1), ss, seed=43), Case(kind, 8, w, h, 2, 1, (1, 0, 1, 1), ss, seed=44)]
    return c


CASES = _cases()


@pytest.mark.parametrize("schedule", SCHEDULES, ids=[f"{s}-seed{SEED}" for s in SCHEDULES])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_the_tile_functions_give_the_reference_under_every_schedule_and_fill(wg_host, case, schedule):
    """dn_tile / dn_tile_t / dn_tile_j / dn_tile_jt, every tile of the plane, 256 threads and the real barriers: equal to
    denoise_ref / denoise_temporal_ref / denoise_joint_ref whatever the order of the threads between two barriers and whatever
    the tile finds in LDS.

    This is also the test of the barrier the header leaves out on purpose ("the next dn_hsum writes Hb only, so no third
    barrier"): between dn_accumulate* of one offset and dn_hsum* of the next there is no sync(), so under `descending` or
    `stragglers` some threads are one phase ahead of others across that gap, and the bytes are still the reference's."""
    want = _reference(case)
    if case.w * case.h >= 64:
        assert (want != (case.frames()[0][1:3] if case.joint else case.frames()[0][0])).any(), "the filter did something"
    for fill, got in wg_host.fills(case, schedule).items():
        assert np.array_equal(got, want), (fill, np.argwhere(got != want)[:5])


# --------------------------------------------------------------------- 4: every barrier is load-bearing, and that shows
# 70 x 30 (chroma 70 x 30 from luma 139 x 59): two tiles, the second partial; A = 3, S = 2, 8 bit; three neighbours take part,
# so the two barriers around the staging of N have a first, a middle and a last occurrence.
DROP_CASES = {
    "tile": Case("tile", 8, 70, 30, 3, 2, seed=51),
    "tile_t": Case("tile_t", 8, 70, 30, 3, 2, (1, 0, 1, 1), seed=52),
    "tile_j": Case("tile_j", 8, 139, 59, 3, 2, (), "420", seed=53),
    "tile_jt": Case("tile_jt", 8, 139, 59, 3, 2, (1, 0, 1, 1), "420", seed=54),
}
# Not needed by the data flow, one occurrence in each temporal tile function: the barrier in front of staging the FIRST
# neighbour.  It is there because "the last dn_accumulate_t has read N", and before the first neighbour nothing has read
# N: the phase in front of it is dn_accumulate of the frame's last own offset, which reads L and Wb, the staging writes N
# only, and the barrier after the staging stands between that dn_accumulate and the first dn_hsum_t / dn_weights_t, which
# are what next write Hb and Wb.  The loop has one barrier at its head for every neighbour; giving the first a pass would
# cost a branch and save one barrier of about 2 (2A + 1)^2 a neighbour.  The kernel is left as it is.
NOT_NEEDED = {("tile_t", "in front of staging N", 0), ("tile_jt", "in front of staging N", 0)}
DROPS = [(k, site) for k, c in DROP_CASES.items() for site in c.sync_calls()[0]]


@pytest.mark.parametrize("kind,site", DROPS, ids=[f"{k}-{s.replace(' ', '_')}" for k, s in DROPS])
def test_a_dropped_barrier_shows_under_some_schedule_and_fill(wg_host, kind, site):
    """The k-th sync() call of every thread made a no-op (the same call in every thread, so the counts still match): for the
    first, a middle and the last occurrence of the site, at least one committed (schedule, fill) pair gives bytes that are
    not the reference's.  (A pair under which the undefined-behaviour sanitizer stops the run -- stale 0xFFFF samples squared
    overflow an int -- has seen the drop too, but it is bytes that are asked for.)  Prints: site, occurrence, call number, the
    first pair that exposes the drop."""
    case = DROP_CASES[kind]
    calls = case.sync_calls()[0][site]
    want = _reference(case)
    for occ in sorted({0, len(calls) // 2, len(calls) - 1}):
        found = None
        for schedule in SCHEDULES:
            for fill, got in wg_host.fills(case, schedule, skip=calls[occ]).items():
                if found is None and got is not None and not np.array_equal(got, want):
                    found = (schedule, fill, int((got != want).sum()))
            if found:
                break
        what = f"{kind:8s} {site:24s} occurrence {occ:3d} of {len(calls):3d} (sync call {calls[occ]:4d})"
        if (kind, site, occ) in NOT_NEEDED:
            print(f"DROP {what}: not needed by the data flow; no pair differs")
            assert found is None, f"{what}: marked as not needed by the data flow, and {found} sees it dropped"
        else:
            print(f"DROP {what}: {found[0]} / {found[1]}, {found[2]} samples differ" if found else f"DROP {what}: NOT SEEN")
            assert found is not None, f"{what}: no committed schedule and fill notices the barrier gone"
    # the bytes without the flag, under the schedule that was looked at last
    assert all(np.array_equal(got, want) for got in wg_host.fills(case, schedule).values())


def test_at_most_one_site_a_tile_function_is_marked_as_not_needed():
    for kind in DROP_CASES:
        assert sum(k == kind for k, _s, _o in NOT_NEEDED) <= 1
    assert all(site in DROP_CASES[k].sync_calls()[0] for k, site, _o in NOT_NEEDED)


# ------------------------------------------------------------------------------- 5: ThreadSanitizer, as a second opinion
# The writes two threads may both make to one word between two barriers: the last task of a row (dn_hsum, for one sample
# array or three) or of a column (dn_weights) starts at RW - 8 / RH - 8 and overlaps its neighbour, and both store the same
# value.  The tasks of dn_hsum_t and dn_weights_t tile kTW x kTH exactly (8 divides 64 and 48), so they never overlap and
# are not in the list.  The stores themselves are made by the bodies the spatial and the temporal phases share, so a race is
# put down to the phase that called the body: the innermost frame of the access that is not one of SHARED_BODIES.  A race
# under dn_hsum_t or dn_weights_t is reported in the same bodies and fails all the same.
ALLOWED_WRITE_WRITE = {"dn_hsum", "dn_weights"}
SHARED_BODIES = {"dn_slide8", "dn_weights8"}

PROBE = r"""
#include <mutex>
#include <thread>
#include <vector>
int main() {
  std::mutex m;
  long n = 0;
  std::vector<std::thread> t;
  for (int i = 0; i < 8; ++i) t.emplace_back([&] { std::lock_guard<std::mutex> l(m); ++n; });
  for (auto &x : t) x.join();
  return n == 8 ? 0 : 1;
}
"""


def _tsan_build(d):
    """The harness with free-running threads under ThreadSanitizer; a skip, with its reason, where a race-free probe
    program does not build or run under it with the host compiler."""
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
        print("ThreadSanitizer is not usable here:", why)
        pytest.skip("ThreadSanitizer is not usable with the host compiler: " + why.splitlines()[0][:200])
    exe = d / "denoise_wg_host_tsan"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", *flags, *static, "-DWG_FREE_RUNNING", "-o", str(exe), SOURCE])
    return exe


RACE = re.compile(r"WARNING: ThreadSanitizer: (.*?)\n(.*?)(?=\n=+\n|\Z)", re.S)
ACCESS = re.compile(r"^  (Previous )?(atomic )?(read|write) of size \d+ at \S+ by [^\n]*:\n((?:    #\d+ [^\n]*(?:\n|\Z))+)", re.M | re.I)
FRAME = re.compile(r"^    #\d+ (?:\S+ in )?([^\n]*)", re.M)


def parse_tsan(stderr):
    """[(kind of report, [(read | write, function of the innermost frame that is not one of SHARED_BODIES), ...])]"""
    out = []
    for kind, body in RACE.findall(stderr):
        acc = []
        for _prev, _atomic, rw, stack in ACCESS.findall(body):
            fns = []
            for frame in FRAME.findall(stack):
                m = re.search(r"(?:\w+::)*(\w+)[<(]", frame)  # (a return type in front, template arguments or parameters behind)
                fns.append(m.group(1) if m else frame.strip())
            acc.append((rw.lower(), next((f for f in fns if f not in SHARED_BODIES), fns[0])))
        out.append((kind.split(" (")[0], acc))
    return out


def test_the_parser_of_thread_sanitizer_reports():
    text = """==================
WARNING: ThreadSanitizer: data race (pid=1)
  Write of size 4 at 0x7b1 by thread T9:
    #0 void g1s_dn::dn_hsum<2>(int, g1s_dn::TileGeom const&, unsigned short const*, unsigned int*, int, int, int, int, unsigned int) /x/denoise_tile.hip.h:120 (a+0x1)
    #1 foo

  Previous write of size 4 at 0x7b1 by thread T8:
    #0 g1s_dn::dn_hsum<2>(int, g1s_dn::TileGeom const&) /x/denoise_tile.hip.h:116 (a+0x2)

SUMMARY: ThreadSanitizer: data race /x/denoise_tile.hip.h:120 in dn_hsum
==================
==================
WARNING: ThreadSanitizer: data race (pid=1)
  Read of size 2 at 0x7b2 by thread T3:
    #0 g1s_dn::dn_weights<2>(int) /x/denoise_tile.hip.h:138 (a+0x3)

  Previous write of size 2 at 0x7b2 by thread T4:
    #0 g1s_dn::dn_weights<2>(int) /x/denoise_tile.hip.h:151 (a+0x3)
==================
==================
WARNING: ThreadSanitizer: data race (pid=1)
  Write of size 4 at 0x7b3 by thread T9:
    #0 void g1s_dn::dn_slide8<2, 3>(unsigned short const*, unsigned short const*, int, unsigned int*) /x/denoise_tile.hip.h:212 (a+0x4)
    #1 void g1s_dn::dn_hsum<2, 3>(int, g1s_dn::TileGeom const&, int, unsigned short const*, unsigned int*, int, int, int, int, unsigned int) /x/denoise_tile.hip.h:231 (a+0x4)
    #2 void g1s_dn::dn_spatial<2, 1, g1s_dn::JointSrc, g1s_dn::JointGeom, wg::Sync>(int, g1s_dn::TileGeom const&, g1s_dn::JointGeom const&, unsigned char*, unsigned short const*, int, g1s_dn::JointSrc const&, int, int, wg::Sync, unsigned int*, unsigned int* const (&) [g1s_dn::JointSrc::NP]) /x/denoise_tile.hip.h:391 (a+0x4)
    #3 operator() tests/denoise_wg_host.cpp:90 (a+0x5)

  Previous write of size 4 at 0x7b3 by thread T8:
    #0 void g1s_dn::dn_slide8<2, 3>(unsigned short const*, unsigned short const*, int, unsigned int*) /x/denoise_tile.hip.h:216 (a+0x6)
    #1 void g1s_dn::dn_hsum<2, 3>(int, g1s_dn::TileGeom const&, int, unsigned short const*, unsigned int*, int, int, int, int, unsigned int) /x/denoise_tile.hip.h:231 (a+0x6)

  Location is heap block of size 49520 at 0x7b0 allocated by main thread:
    #0 operator new(unsigned long) tsan_new_delete.cpp:64 (libtsan.so.0+0x8f162)
    #1 main tests/denoise_wg_host.cpp:209 (a+0x7)

SUMMARY: ThreadSanitizer: data race /x/denoise_tile.hip.h:212 in void g1s_dn::dn_slide8<2, 3>(unsigned short const*, unsigned short const*, int, unsigned int*)
==================
==================
WARNING: ThreadSanitizer: data race (pid=1)
  Write of size 4 at 0x7b4 by thread T5:
    #0 void g1s_dn::dn_slide8<2, 1>(unsigned short const*, unsigned short const*, int, unsigned int*) /x/denoise_tile.hip.h:212 (a+0x8)
    #1 void g1s_dn::dn_hsum_t<2, 1>(int, g1s_dn::TileGeom const&, int, unsigned short const*, unsigned short const*, unsigned int*, int, int) /x/denoise_tile.hip.h:245 (a+0x8)
    #2 void g1s_dn::dn_temporal<2, 1, 1, g1s_dn::TileGeom, int, wg::Sync>(int) /x/denoise_tile.hip.h:420 (a+0x8)

  Previous write of size 4 at 0x7b4 by thread T6:
    #0 void g1s_dn::dn_weights8<2, g1s_dn::dn_weights_t<2>(int, int)::{lambda(int)#1}>(g1s_dn::TileGeom const&, g1s_dn::dn_weights_t<2>(int, int)::{lambda(int)#1}) /x/denoise_tile.hip.h:263 (a+0x9)
    #1 void g1s_dn::dn_weights_t<2>(int, int) /x/denoise_tile.hip.h:293 (a+0x9)
==================
"""
    got = parse_tsan(text)
    assert got == [("data race", [("write", "dn_hsum"), ("write", "dn_hsum")]), ("data race", [("read", "dn_weights"), ("write", "dn_weights")]),
                   ("data race", [("write", "dn_hsum"), ("write", "dn_hsum")]), ("data race", [("write", "dn_hsum_t"), ("write", "dn_weights_t")])]
    # the shared bodies under dn_hsum are the documented overlap; under the temporal phases, whose tasks never overlap, they are a finding
    allowed = [all(rw == "write" and fn in ALLOWED_WRITE_WRITE for rw, fn in acc) for _kind, acc in got]
    assert allowed == [True, False, True, False]
    assert not SHARED_BODIES & ALLOWED_WRITE_WRITE


TSAN_CASES = [Case("tile", 8, 70, 50, 3, 2, seed=61), Case("tile_t", 8, 70, 50, 3, 2, (1, 1), seed=62),
              Case("tile_j", 8, 139, 99, 3, 2, (), "420", seed=63), Case("tile_jt", 8, 139, 99, 3, 2, (1, 1), "420", seed=64)]


TSAN_ENV = dict(ENV, TSAN_OPTIONS="halt_on_error=0:exitcode=0:report_thread_leaks=0")


@pytest.fixture(scope="module")
def tsan_exe(tmp_path_factory):
    if _compiler() is None:
        pytest.skip("no C++ compiler")
    return _tsan_build(tmp_path_factory.mktemp("tsan"))


@pytest.mark.parametrize("case", TSAN_CASES, ids=[c.id for c in TSAN_CASES])
def test_thread_sanitizer_finds_only_the_overlapping_stores_of_equal_values(wg_host, tsan_exe, case):
    """256 free-running threads a tile and a plain barrier, no serialisation: every report is a data race between two WRITES
    whose phases (parse_tsan: the innermost frame that is not a shared body) are both in ALLOWED_WRITE_WRITE -- the documented
    overlap of a row's or a column's last task with its neighbour.  No suppression file: a read/write race in the same
    functions fails this."""
    got, p = wg_host(case, "ascending", "random", program=tsan_exe, env=TSAN_ENV)
    assert np.array_equal(got, _reference(case))
    reports = parse_tsan(p.stderr)
    assert p.stderr.count("WARNING: ThreadSanitizer") == len(reports)
    seen = set()
    for kind, acc in reports:
        ok = kind == "data race" and len(acc) == 2 and all(rw == "write" and fn in ALLOWED_WRITE_WRITE for rw, fn in acc)
        assert ok, (kind, acc, p.stderr[-4000:])
        seen.add(tuple(sorted(fn for _rw, fn in acc)))
    print(f"ThreadSanitizer, {case.kind}: write/write pairs seen:", sorted(seen))


def test_thread_sanitizer_reports_a_dropped_barrier_as_a_read_against_a_write(wg_host, tsan_exe):
    """The probe of the parser's other half, and of the build: the same program with one barrier gone."""
    case = TSAN_CASES[0]
    calls = case.sync_calls()[0]["after dn_hsum"]
    _got, p = wg_host(case, "ascending", "random", skip=calls[len(calls) // 2], program=tsan_exe, env=TSAN_ENV)
    assert any(any(rw == "read" for rw, _fn in acc) for _k, acc in parse_tsan(p.stderr)), p.stderr[-3000:]
