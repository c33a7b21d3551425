"""The seeded sweep of tests/sweep.py on the device: every drawn case of every operation against the reference the fixed
tests of that operation use, bit for bit.  One test per operation and chunk; inside a chunk every case runs and the failure
message lists every failing case as the record to paste into `tools/fuzz_parity.py OP --case 'RECORD'`.

  diff       every frame's record (tests/helpers.py) and the `.tbl` bytes against the oracle; the device refuses with
             G1S_ERR_NOT_ENOUGH_FLAT exactly when the oracle raises "Not enough flat blocks" -- both are always asked; from
             1 000 blocks a frame also the per-frame latest states of the device half of the fold (k4_latest, chunks of
             1 024 blocks) against the host half's, byte for byte
  render     templates, scaling tables and rendered planes against tests/grain_ref.py
  denoise    tests/denoise_ref.py; denoise_t: clips against tests/denoise_temporal_ref.py
  estimate   tests/oracle_binding.estimate_plane_noise
  resize     tests/oracle_binding.resize_planes

`run_cases(op, cases, env)` is the whole comparison (tools/fuzz_parity.py calls it too).  A GrainSynthesizer (keyed by depth
and clipping) and a Denoiser (keyed by its parameters, which a list draws from a pool of eight sets) are kept across the cases
of a call, so that what one geometry leaves behind meets the next: tests/test_sweep_cpu.py counts how often that happens in
the committed lists.  A DiffGenerator and a NoiseEstimator hold one geometry, a FilterChain one target size: made per case.

G1S_K3 is read once per process, so the diff cases that ask for the stream chain run in a child, `python -m
tests.sweep_worker`, started with it set.  The child has ten minutes; one that runs out of them, or dies, fails every stream
case of the call and is not started again.
"""
from __future__ import annotations

import os
import subprocess
import sys
import time
from fractions import Fraction
from typing import List, Tuple

import numpy as np
import pytest

from tests import sweep as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = Fraction(30000, 1001)
NOT_ENOUGH_FLAT = -3  # G1S_ERR_NOT_ENOUGH_FLAT
WORKER_MARK = "SWEEP-WORKER-RESULT "  # the one line of tests/sweep_worker.py that is read: repr of [(case, message)]


class ProcessEnv:
    """monkeypatch's setenv / delenv for a caller without pytest (tools/fuzz_parity.py)."""

    def setenv(self, name, value):
        os.environ[name] = value

    def delenv(self, name, raising=False):
        os.environ.pop(name, None)


def _to_dev(planes):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(p)).to("cuda") for p in planes]


def _host(p):
    return p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)


def first_difference(got, want, what: str):
    """None, or where planes `got` first differ from `want`: plane, row, column and both values."""
    if len(got) != len(want):
        return f"{what}: {len(got)} planes for {len(want)}"
    for c, (a, b) in enumerate(zip(got, want)):
        a, b = _host(a), np.asarray(b)
        if a.shape != b.shape or (a.dtype != b.dtype and a.dtype.kind == b.dtype.kind == "u"):
            return f"{what} plane {c}: {a.shape} {a.dtype} for {b.shape} {b.dtype}"
        bad = np.argwhere(a != b)
        if len(bad):
            at = tuple(bad[0])
            return f"{what} plane {c}: {len(bad)} samples differ, first at row {at[0]} column {at[1]}: {a[at]} for {b[at]}"
    return None


# ---- diff ---------------------------------------------------------------------------------------------------------------

def _diff_case(c: dict, env) -> List[str]:
    from grav1synth_amd._lib import G1SError
    from grav1synth_amd.diff import DiffGenerator, Frame, Record, format_tbl
    from tests.helpers import oracle_shadow, record_mismatches
    from tests.oracle_binding import OracleDiff, format_tbl as oracle_tbl

    xd, yd = S.SUBSAMPLINGS[c["ss"]]
    nplanes = 3 if c["chroma"] else 1
    frames = S.diff_frames(c)
    o = OracleDiff(FPS.numerator, FPS.denominator, c["src_bd"], c["den_bd"], c["lag"], c["chroma"])
    shadows, refusal = [], None
    for k, (s, d) in enumerate(frames):
        try:
            o.diff_frame(s, d, xd, yd)
        except RuntimeError as e:
            refusal = f"frame {k}: {e}"
            break
        shadows.append(oracle_shadow(o, nplanes))
    want = oracle_tbl(o.finish()) if refusal is None else None
    o.close()
    feed = [(_to_dev(s), _to_dev(d)) if c["where"] == "device" else (s, d) for s, d in frames]
    if c["latest"]:
        env.setenv("G1S_LATEST", c["latest"])
    else:
        env.delenv("G1S_LATEST", raising=False)
    kw = dict(ar_coeff_lag=c["lag"], luma_only=not c["chroma"], batch_frames=c["batch"])
    out = []
    try:
        # every frame's record (a records-only generator keeps the per-frame half of the fold on the host)
        g = DiffGenerator(FPS, c["src_bd"], c["den_bd"], records_only=True, **kw)
        recs, n = None, 0
        try:
            for s, d in feed:
                g.diff_frame(Frame(s, xd, yd), Frame(d, xd, yd))
            recs, n = g.take_records(c["w"], c["h"], nplanes, len(frames))
        except G1SError as e:
            out.append(f"the records-only generator fails: {e}")
        finally:
            g.close()
        if recs is not None and n != len(frames):
            out.append(f"{n} records for {len(frames)} frames")
        for i in range(min(n, len(shadows))):
            out.extend(record_mismatches(shadows[i], Record(recs[i]), f"frame {i} (batch {i // c['batch']}, position {i % c['batch']})"))
        # the table, or the refusal
        g = DiffGenerator(FPS, c["src_bd"], c["den_bd"], **kw)
        err, got = None, None
        try:
            for s, d in feed:
                g.diff_frame(Frame(s, xd, yd), Frame(d, xd, yd))
            got = format_tbl(g.finish())
        except G1SError as e:
            err = e
        finally:
            g.close()
        if c["blocks"] >= 1000:  # (last: it sets G1S_LATEST itself)
            out.extend(_latest_mismatches(c, feed, xd, yd, kw, env))
    finally:
        env.delenv("G1S_LATEST", raising=False)
    if refusal is None:
        if err is not None:
            out.append(f"the oracle gives a table, the device refuses: {err}")
        elif got != want:
            a, b = got.split(b"\n"), want.split(b"\n")
            line = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            out.append(f".tbl differs ({len(got)} bytes for {len(want)}), first at line {line}: {a[line:line + 1]} for {b[line:line + 1]}")
    elif "Not enough flat blocks" in refusal:
        if err is None:
            out.append(f"the oracle refuses ({refusal}), the device emits a table of {len(got)} bytes")
        elif err.code != NOT_ENOUGH_FLAT:
            out.append(f"the oracle refuses ({refusal}), the device fails with {err}")
    elif err is None or err.code == NOT_ENOUGH_FLAT:
        out.append(f"the oracle fails ({refusal}), the device: {err or 'a table'}")
    return out


def _latest_mismatches(c, feed, xd, yd, kw, env) -> List[str]:
    """The per-frame latest states (status, message, the luma and chroma systems as far as they got) of the device half of
    the fold against the host half's, byte for byte: what k4_latest makes of every chunk of 1 024 blocks, a short last one
    included, where a table may not move."""
    from grav1synth_amd._lib import G1SError
    from grav1synth_amd.diff import DiffGenerator, Frame

    blobs = {}
    for where in ("host", "device"):
        env.setenv("G1S_LATEST", where)
        g = DiffGenerator(FPS, c["src_bd"], c["den_bd"], records_only=2, **kw)
        try:
            for s, d in feed:
                g.diff_frame(Frame(s, xd, yd), Frame(d, xd, yd))
            blobs[where] = g.take_latest(len(feed) + 8, sync=True).copy()
        except G1SError as e:
            return [f"latest states, {where} half: {e}"]
        finally:
            g.close()
    host, dev = blobs["host"], blobs["device"]
    if host.shape != dev.shape or host.shape[0] != len(feed):
        return [f"latest states: {dev.shape} from the device half, {host.shape} from the host half, {len(feed)} frames"]
    out = []
    for i in range(len(feed)):
        bad = np.flatnonzero(host[i] != dev[i])
        if bad.size:
            out.append(f"frame {i}: the device half's latest state differs from the host half's in {bad.size} bytes, first at {bad[0]} of {host.shape[1]}")
    return out


def _diff_stream_child(cases, env) -> List[Tuple[dict, str]]:
    """G1S_K3 is read once per process: the cases that ask for the stream chain run in a child that starts with it set."""
    import ast

    env.setenv("G1S_K3", "stream")
    try:
        cmd = [sys.executable, "-m", "tests.sweep_worker", "diff"] + [repr(c) for c in cases]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        except subprocess.TimeoutExpired:
            return [(c, "the G1S_K3=stream child did not end within 600 s") for c in cases]
    finally:
        env.delenv("G1S_K3", raising=False)
    marks = [line[len(WORKER_MARK):] for line in p.stdout.splitlines() if line.startswith(WORKER_MARK)]
    if p.returncode != 0 or len(marks) != 1:
        return [(c, f"the G1S_K3=stream child ended with {p.returncode}: {(p.stderr or p.stdout)[-400:]}") for c in cases]
    return [(c, m) for c, m in ast.literal_eval(marks[0])]


def _run_diff(cases, env):
    fails = []
    in_child = {k for k, c in enumerate(cases) if c["k3"] == "stream" and os.environ.get("G1S_K3") != "stream"}
    for k, c in enumerate(cases):
        if k not in in_child:
            fails += [(c, m) for m in _diff_case(c, env)]
    if in_child:
        fails += _diff_stream_child([cases[k] for k in sorted(in_child)], env)
    return fails


# ---- render -------------------------------------------------------------------------------------------------------------

def _run_render(cases, env):
    from grav1synth_amd.grain import GrainSynthesizer
    from tests import grain_ref as R

    synths, fails = {}, []
    try:
        for c in cases:
            key = (c["bd"], c["clip"], c["mc_identity"])
            if key not in synths:
                synths[key] = GrainSynthesizer(c["bd"], clip_to_restricted_range=c["clip"], mc_identity=c["mc_identity"])
            syn = synths[key]
            seg, planes = S.segment_of(c), S.render_planes(c)
            mono = c["ss"] == "mono"
            subx, suby = S.SUBSAMPLINGS[c["ss"]]
            grain = R.generate_grain(seg, c["bd"], subx, suby)
            dev = _to_dev(planes)

            def templates():
                luma, cb, cr, lut = syn.templates(seg, subx, suby)
                return (first_difference([luma, cb, cr], [g.astype(np.int16) for g in grain], "template")
                        or first_difference([lut], [R.scaling_luts(seg).astype(np.uint8)], "scaling tables"))

            def rendered():
                got = syn.apply(dev, seg, subx, suby)
                want = R.add_noise(planes, seg, c["bd"], subx, suby, c["clip"], c["mc_identity"], grain=(grain[0], None, None) if mono else grain)
                return first_difference(got, want, "rendered") or first_difference(dev, planes, "the input after the call")

            # (a template call before any frame has set the geometry, and one after a frame of another geometry)
            for step in ((templates, rendered) if c["i"] & 1 else (rendered, templates)):
                msg = step()
                if msg:
                    fails.append((c, msg))
    finally:
        for s in synths.values():
            s.close()
    return fails


# ---- denoise ------------------------------------------------------------------------------------------------------------

def _tables(c):
    from grav1synth_amd.denoise import weight_table

    return weight_table(c["bd"], c["S"], c["strength"]), weight_table(c["bd"], c["S"], c["chroma_strength"])


def _denoiser(made, c, **kw):
    from grav1synth_amd.denoise import Denoiser

    key = (c["bd"], c["A"], c["S"], c["strength"], c["chroma_strength"], tuple(sorted(kw.items())))
    if key not in made:
        made[key] = Denoiser(c["bd"], search_radius=c["A"], patch_radius=c["S"], strength=c["strength"], chroma_strength=c["chroma_strength"], **kw)
    return made[key]


def _dn_sub(c):
    return (1, 1) if c["ss"] == "mono" else S.SUBSAMPLINGS[c["ss"]]


def _run_denoise(cases, env):
    from tests import denoise_ref as R

    made, fails = {}, []
    try:
        for c in cases:
            planes = S.denoise_frames(c, 1)[0]
            dev = _to_dev(planes)
            got = _denoiser(made, c).apply(dev, *_dn_sub(c))
            want = R.denoise_frame(planes, c["A"], c["S"], *_tables(c))
            msg = first_difference(got, want, "denoised") or first_difference(dev, planes, "the input after the call")
            if msg:
                fails.append((c, msg))
    finally:
        for d in made.values():
            d.close()
    return fails


def temporal_reference(c, frames):
    from tests import denoise_temporal_ref as TR

    return TR.denoise_clip(frames, c["D"], c["A"], c["S"], *_tables(c))


def _run_denoise_t(cases, env):
    made, fails = {}, []
    try:
        for c in cases:
            frames = S.denoise_frames(c, c["nframes"])
            dev = [_to_dev(f) for f in frames]
            dn = _denoiser(made, c, temporal_radius=c["D"], batch_frames=c["batch"])
            sub, k = _dn_sub(c), c["split"]
            msgs = []
            if c["split_kind"] == "sync":
                got = dn.denoise_clip(dev[:k], *sub) + dn.denoise_clip(dev[k:], *sub)
                want = temporal_reference(c, frames[:k]) + temporal_reference(c, frames[k:])
            elif c["split_kind"] == "geometry":  # a host frame of another geometry inside the queue: three clips
                oc, other = S.other_geometry(c)
                got = [dn.apply(f, *sub, sync=False) for f in dev[:k]]
                got_other = dn.apply(other, *_dn_sub(oc), sync=False)
                got += [dn.apply(f, *sub, sync=False) for f in dev[k:]]
                dn.sync()
                want = temporal_reference(c, frames[:k]) + temporal_reference(c, frames[k:])
                msgs.append(first_difference(got_other, temporal_reference(c, [other])[0], "the frame of the other geometry"))
            else:
                got = dn.denoise_clip(dev, *sub)
                want = temporal_reference(c, frames)
            for t in range(len(frames)):
                msgs.append(first_difference(got[t], want[t], f"frame {t}") or first_difference(dev[t], frames[t], f"input frame {t} after the call"))
            fails += [(c, m) for m in msgs if m]
    finally:
        for d in made.values():
            d.close()
    return fails


# ---- estimate -----------------------------------------------------------------------------------------------------------

def _run_estimate(cases, env):
    import torch

    from grav1synth_amd.estimate import NoiseEstimator
    from tests.oracle_binding import estimate_plane_noise

    fails = []
    for c in cases:  # (an estimator refuses a new geometry mid-stream -- G1S_ERR_DIM_MISMATCH -- so every case makes its own)
        p = S.estimate_plane(c)
        want = [estimate_plane_noise(p, c["bd"])] * 4
        est = NoiseEstimator(c["bd"], batch_frames=3)
        try:
            keep = []
            for _ in want:  # the same plane four times: a full batch of three and a short one
                if c["where"] == "host":
                    est.estimate_frame(p)
                elif c["where"] == "strided":  # a view into a wider device plane: odd pointer, pitch != width
                    big = torch.zeros((p.shape[0] + 2, p.shape[1] + 7), dtype=torch.from_numpy(p).dtype, device="cuda")
                    big[1:-1, 3:3 + p.shape[1]] = torch.from_numpy(p).cuda()
                    keep.append(big)
                    est.estimate_frame(big[1:-1, 3:3 + p.shape[1]])
                else:
                    keep.append(torch.from_numpy(p).cuda())
                    est.estimate_frame(keep[-1])
            got = est.finish()
        finally:
            est.close()
        if got != want:
            fails.append((c, f"estimates {got!r} for {want!r}"))
    return fails


# ---- resize -------------------------------------------------------------------------------------------------------------

def _run_resize(cases, env):
    from grav1synth_amd.diff import Frame
    from grav1synth_amd.filters import FilterChain
    from tests.oracle_binding import resize_planes

    fails = []
    for c in cases:  # (a chain's target size is part of its text: a chain a case)
        chain = FilterChain(f"resize:width={c['tw']},height={c['th']},alg={c['alg']}")
        try:
            planes = S.resize_planes_of(c)
            xd, yd = S.SUBSAMPLINGS[c["ss"]]
            want = resize_planes(planes, xd, yd, c["tw"], c["th"], c["bd"], c["alg"])
            src = _to_dev(planes) if c["where"] == "device" else [p.copy() for p in planes]
            got = chain.apply(Frame(src, xd, yd), c["bd"]).planes
        finally:
            chain.close()
        msg = first_difference(got, want, "resized") or first_difference(src, planes, "the input after the call")
        if msg:
            fails.append((c, msg))
    return fails


def run_cases(op: str, cases, env=None) -> List[Tuple[dict, str]]:
    """Every case of the list on the device and through its reference: [(case, what differs)], empty when all agree."""
    return globals()["_run_" + op](list(cases), env or ProcessEnv())


def report(fails) -> str:
    return "\n".join(f"FAIL {c!r} :: {m}" for c, m in fails)


def _chunk(op, chunk, monkeypatch):
    seed, n, chunks = S.SUITE[op]
    every = S.cases(op, seed, n)
    mine = S.chunk_of(every, chunk, chunks)
    t0 = time.time()
    fails = run_cases(op, mine, monkeypatch)
    print(f"sweep {op} seed {seed}: chunk {chunk} of {chunks}, {len(mine)} of {n} cases, list sha256 {S.digest(every)}, "
          f"{len(fails)} failures, {time.time() - t0:.1f} s")
    bad = {c["i"] for c, _ in fails}
    assert not fails, f"{len(bad)} of {len(mine)} {op} cases differ from the reference:\n" + report(fails)


@pytest.mark.parametrize("chunk", range(S.SUITE["diff"][2]))
def test_diff(chunk, monkeypatch):
    _chunk("diff", chunk, monkeypatch)


@pytest.mark.parametrize("chunk", range(S.SUITE["render"][2]))
def test_render(chunk, monkeypatch):
    _chunk("render", chunk, monkeypatch)


@pytest.mark.parametrize("chunk", range(S.SUITE["denoise"][2]))
def test_denoise(chunk, monkeypatch):
    _chunk("denoise", chunk, monkeypatch)


@pytest.mark.parametrize("chunk", range(S.SUITE["denoise_t"][2]))
def test_denoise_t(chunk, monkeypatch):
    _chunk("denoise_t", chunk, monkeypatch)


@pytest.mark.parametrize("chunk", range(S.SUITE["estimate"][2]))
def test_estimate(chunk, monkeypatch):
    _chunk("estimate", chunk, monkeypatch)


@pytest.mark.parametrize("chunk", range(S.SUITE["resize"][2]))
def test_resize(chunk, monkeypatch):
    _chunk("resize", chunk, monkeypatch)
