"""The accumulation chains at the int8 edge of a residual and at the int32 bound of a workgroup's slice: every frame's record
against the oracle's integers, exactly, on residual fields designed sample by sample (tests/int8_content.py).

Both chains -- the wide one (k3w_pass, k3w_tail) and the stream one (k3s_fused, k3m_finish, k3_ar_generic) -- multiply a residual
on the matrix cores only if it lies in -128 .. 127 and leave every other unit to the exact kernel; the chroma regressor L (the sum
of the luma residuals under a chroma sample) is held to the same range; and a workgroup's int32 accumulators are safe only because
its slice is capped (kWMaxUnits = 100, kWMaxUnitsC = 32, kMMaxUnits = 240, enforced by the engine's workgroups a frame).

  A  single residuals of -129, -128, 127 and 128 in a benign field (|d| <= 3): a unit's interior, its words 0 and 15, the last own
     word of a stream unit, the rows the block below reads as its halo, the plane's first and last row and column, both halves of a 16-bit pair at once
     (-129 beside -128 and beside 127); luma, Cb alone, Cr alone; in units that are the ghost in front of and behind a slice,
     the last unit of an odd slice, a slice's interior, by the workgroups a frame of the case.
  B  L of 127, 128, -128 and -129 with every luma residual under it well inside int8: under the first and the second luma unit of a
     chroma unit, under the half-covered last chroma unit of a row, in a chroma unit's words 0 and 15.
  C  every sample of a plane at -128 or 127, whole units at one of them: chroma over such a luma (L = +-512: every chroma unit is
     deferred) and over a luma whose L stays inside int8 (none is).
  D  slices of exactly the cap's length: 100 luma units, 32 chroma units (16 and 32 steps a unit), the stream chain's 224, on fields
     of -128 / 127, where an accumulator's top two bits are live and the int64 partial sums carry past 32 bits; workgroups a frame
     below what the cap asks for (the engine raises them, the record does not change); one frame over a cap.

"Was deferred" is not visible in a record.  These tests see the sums only: a residual outside int8 must give the oracle's integers,
and so must one inside it.  A kernel that defers -128 needlessly passes; one that keeps 128 as int8 (sum_d2 right, every cross
product's sign flipped) does not.

The oracle runs once per geometry and its shadows are shared by the cases.  What the content reaches -- the flat masks, the
residuals recomputed from the planes, the slices the cases cut, the magnitudes -- is asserted without a device in
tests/test_int8_content_cpu.py."""
import functools
from typing import NamedTuple

import numpy as np
import pytest

from tests import int8_content as IC
from tests.helpers import oracle_shadow, record_mismatches
from tests.oracle_binding import OracleDiff
from tests.test_gpu_records import CHAIN_KERNEL, FPS, SLOTS, Geom, _feed, _generator

pytestmark = pytest.mark.gpu

BATCH = 3
UNIT_W = 128  # samples a unit row of the wide chain (k3w.hip.h kWUnitW); a stream unit is 64
VALUES = (-129, -128, 127, 128)

# ---- A, B, C: small frames ------------------------------------------------------------------------------------------------------
# 640 x 96: 5 luma units and (4:2:0, 4:2:2) 2 1/2 chroma units a block row, three block rows
GEOMS = {
    "8b420": (Geom(640, 96, 8, 8, 1, 1, 2), "wide"),
    "10b420": (Geom(640, 96, 10, 10, 1, 1, 3), "wide"),
    "10b_luma_only": (Geom(640, 96, 10, 10, 1, 1, 3, False), "wide"),
    "10b444": (Geom(640, 96, 10, 10, 0, 0, 2), "wide"),
    "8b422": (Geom(640, 96, 8, 8, 1, 0, 2), "wide"),
    "8b420_646x102": (Geom(646, 102, 8, 8, 1, 1, 2), "stream"),   # nothing a multiple of 8
    "10_8_444": (Geom(640, 96, 10, 8, 0, 0, 1), "stream"),        # a mixed pair: the general residual
}
# workgroups a frame.  wide: (G1S_W_WGS, G1S_W_WGS_C), the counts of tests/test_gpu_k3w_slices.py for this size; stream: G1S_F_WGS
WGS = {"wide": (("4", "2"), ("5", "4"), ("7", "6")), "stream": (("8",), ("64",))}
# the units a design pokes, (block row, cell) on the grid of 128-sample cells of the plane kind, by cells a row: what they are to
# the slices of WGS -- ghost in front, ghost behind, last of an odd slice, interior -- tests/test_int8_content_cpu.py asserts
POKED_UNITS = {5: ((0, 2), (1, 2), (2, 0)), 6: ((0, 2), (1, 2), (2, 0)), 3: ((0, 1), (1, 0), (1, 1), (2, 1))}


class Spec(NamedTuple):
    section: str   # "A", "B", "C"
    label: str
    pokes: tuple   # ((plane, y, x, value), ...) single residuals
    lsets: tuple   # ((cy, cx, value), ...) L under chroma samples
    fields: tuple  # per plane "benign" | "extremes" | "quads"
    fills: tuple   # ((plane, block row, cell, value), ...) whole units


def plane_dims(geom: Geom, c: int):
    """(width, height, block width, block height) of plane c."""
    if c == 0:
        return geom.w, geom.h, 32, 32
    return geom.w >> geom.xd, geom.h >> geom.yd, 32 >> geom.xd, 32 >> geom.yd


def _whole_units(geom: Geom, c: int):
    """The poked units of plane c that lie wholly inside it."""
    pw, ph, _, bh = plane_dims(geom, c)
    gx = -(-pw // UNIT_W)
    return [(by, cell) for by, cell in POKED_UNITS[gx] if (cell + 1) * UNIT_W <= pw and (by + 1) * bh <= ph]


# a kind of poke: (row offset from the middle row of the unit, column in the unit)
IN_UNIT = {
    "interior": (0, 45),
    "word0": (-3, 1),      # inside the first `lag` columns: the unit before reads it
    "word15": (2, 126),    # inside the last `lag` columns
    "word7": (1, 62),      # the last own word of the first stream unit in the cell
}


def poke_positions(geom: Geom, c: int, kind: str):
    """[(y, x)] of the design `kind` in plane c."""
    pw, ph, _, bh = plane_dims(geom, c)
    if kind == "borders":  # the plane's first and last row and column: its corners, and a sample along each side
        return [(0, 0), (0, pw - 1), (ph - 1, 0), (ph - 1, pw - 1), (0, pw // 2 + 3), (ph - 1, pw // 4 + 1), (ph // 2 + 5, 0), (ph // 4, pw - 1)]
    out = []
    for by, cell in _whole_units(geom, c):
        if kind == "halo":  # the last rows of the block: what the block below reads above its own
            out.append((by * bh + bh - 2, cell * UNIT_W + 70))
        else:
            dy, x = IN_UNIT[kind]
            out.append((by * bh + bh // 2 + dy, cell * UNIT_W + x))
    return out


def specs(geom: Geom):
    nplanes = 3 if geom.chroma else 1
    benign = ("benign",) * nplanes
    out = []
    for c in range(nplanes):
        name = ("Y", "Cb", "Cr")[c]
        for kind in ("interior", "word0", "word15", "word7", "halo", "borders"):
            for v in VALUES:
                out.append(Spec("A", f"{name} {kind} {v}", tuple((c, y, x, v) for y, x in poke_positions(geom, c, kind)), (), benign, ()))
        # both halves of a 16-bit pair: -129 in the low half (sample 0 of a word), its partner -- sample 2 of the word in 8-bit
        # planes, sample 1 in 16-bit ones and in the general form; both are set -- at -128 / 127
        for partner in (-128, 127):
            pk = []
            for y, x in poke_positions(geom, c, "interior"):
                x0 = (x & ~7) + 8
                pk += [(c, y - 1, x0, -129), (c, y - 1, x0 + 1, partner), (c, y - 1, x0 + 2, partner)]
            out.append(Spec("A", f"{name} pair -129 beside {partner}", tuple(pk), (), benign, ()))
    if geom.chroma:
        cw, ch, _, cbh = plane_dims(geom, 1)
        units = _whole_units(geom, 1)
        gx = -(-cw // UNIT_W)
        lkinds = {
            "under the first luma unit": [(by * cbh + cbh // 2, cell * UNIT_W + 20) for by, cell in units],
            "under the second luma unit": [(by * cbh + cbh // 2 - 1, cell * UNIT_W + 64 + 20) for by, cell in units],
            "chroma word 0": [(by * cbh + cbh // 2 + 1, cell * UNIT_W + 1) for by, cell in units],
            "chroma word 15": [(by * cbh + cbh // 2 - 2, cell * UNIT_W + 126) for by, cell in units],
            # (the last cell of a row: half covered where the chroma plane is 2 1/2 cells wide)
            "last cell of a row": [(by * cbh + cbh // 2, (gx - 1) * UNIT_W + 30) for by in range(3)],
        }
        for kind, pos in lkinds.items():
            for v in (127, 128, -128, -129):
                out.append(Spec("B", f"L {kind} {v}", (), tuple((cy, cx, v) for cy, cx in pos), benign, ()))
        fy = ((0, 0, 1, -128), (0, 2, 3, 127))
        fc = ((1, 0, 0, -128), (1, 2, 1, 127), (2, 1, 1, -128), (2, 2, 0, 127))
        out.append(Spec("C", "extremes over extremes, filled units", (), (), ("extremes",) * 3, fy + fc))
        out.append(Spec("C", "extremes over L inside int8, filled chroma units", (), (), ("quads", "extremes", "extremes"), fc))
        out.append(Spec("C", "benign chroma over extremes, filled luma units", (), (), ("extremes", "benign", "benign"), fy))
    else:
        out.append(Spec("C", "extremes, filled units", (), (), ("extremes",), ((0, 0, 1, -128), (0, 2, 3, 127))))
        out.append(Spec("C", "extremes", (), (), ("extremes",), ()))
    return out


def residuals(geom: Geom, k: int, sp: Spec):
    """The residual fields of frame k."""
    res = []
    for c, field in enumerate(sp.fields):
        pw, ph, _, _ = plane_dims(geom, c)
        rng = np.random.default_rng([geom.w, geom.h, k, c])
        if field == "benign":
            res.append(IC.benign((ph, pw), rng))
        elif field == "extremes":
            res.append(IC.extremes((ph, pw), rng))
        else:
            res.append(IC.quads_inside((ph, pw), rng, geom.xd, geom.yd))
    for c, by, cell, v in sp.fills:
        IC.fill_unit(res[c], by, cell, v, UNIT_W, plane_dims(geom, c)[3])
    for cy, cx, v in sp.lsets:
        IC.set_L(res[0], cy, cx, v, geom.xd, geom.yd)
    for c, y, x, v in sp.pokes:
        IC.poke(res[c], y, x, v)
    return res


def _run_oracle(geom: Geom, fields_of_frames):
    o = OracleDiff(FPS.numerator, FPS.denominator, geom.src_bd, geom.den_bd, geom.lag, geom.chroma)
    frames, shadows = [], []
    for k, res in enumerate(fields_of_frames):
        s, d = IC.make_frames(res, geom.src_bd, geom.den_bd, k)
        o.diff_frame(s, d, geom.xd, geom.yd)  # (raises if the oracle does not accept the frame)
        frames.append((s, d))
        shadows.append(oracle_shadow(o, len(s)))
    return frames, shadows


@functools.lru_cache(maxsize=None)
def _job(name: str):
    """The specs of the geometry's frames, the frames (host planes), the oracle's shadows of every frame."""
    geom = GEOMS[name][0]
    sps = specs(geom)
    frames, shadows = _run_oracle(geom, (residuals(geom, k, sp) for k, sp in enumerate(sps)))
    return sps, frames, shadows


def _records(geom: Geom, frames, batch: int):
    """Feed the frames to a records-only generator; the records' bytes."""
    g = _generator(geom, batch, records_only=True)
    try:
        _feed(g, geom, frames)
        recs, n = g.take_records(geom.w, geom.h, 3 if geom.chroma else 1, len(frames))
        assert n == len(frames), f"{n} records for {len(frames)} frames"
        return [np.array(recs[i], copy=True) for i in range(n)]
    finally:
        g.close()


def _check(geom: Geom, frames, shadows, labels, batch: int):
    from grav1synth_amd.diff import Record

    recs = _records(geom, frames, batch)
    bad = []
    for i, rec in enumerate(recs):
        j = i // batch
        bad.extend(record_mismatches(shadows[i], Record(rec), f"frame {i} ({labels[i]}; batch {j}, position {i % batch}, slot {j % SLOTS})"))
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:40])
    return recs


def _set_wgs(monkeypatch, chain: str, wgs):
    if chain == "wide":
        monkeypatch.setenv("G1S_W_WGS", wgs[0])
        monkeypatch.setenv("G1S_W_WGS_C", wgs[1])
    else:
        monkeypatch.setenv("G1S_F_WGS", wgs[0])


CASES = [(name, wgs) for name, (_, chain) in GEOMS.items() for wgs in WGS[chain]]


def _section(monkeypatch, name, wgs, section):
    geom, chain = GEOMS[name]
    _set_wgs(monkeypatch, chain, wgs)
    sps, frames, shadows = _job(name)
    idx = [i for i, sp in enumerate(sps) if sp.section == section]
    _check(geom, [frames[i] for i in idx], [shadows[i] for i in idx], [sps[i].label for i in idx], BATCH)


@pytest.mark.parametrize("name,wgs", CASES, ids=[f"{n}-{'_'.join(w)}" for n, w in CASES])
def test_a_single_residuals_at_the_int8_edge(monkeypatch, name, wgs):
    _section(monkeypatch, name, wgs, "A")


@pytest.mark.parametrize("name,wgs", [c for c in CASES if GEOMS[c[0]][0].chroma], ids=[f"{n}-{'_'.join(w)}" for n, w in CASES if GEOMS[n][0].chroma])
def test_b_luma_sums_at_the_int8_edge(monkeypatch, name, wgs):
    _section(monkeypatch, name, wgs, "B")


@pytest.mark.parametrize("name,wgs", CASES, ids=[f"{n}-{'_'.join(w)}" for n, w in CASES])
def test_c_whole_fields_at_the_extremes(monkeypatch, name, wgs):
    _section(monkeypatch, name, wgs, "C")


def _chain_run(geom: Geom, frames):
    g = _generator(geom, 2, records_only=True)
    try:
        g.set_timing(True)
        _feed(g, geom, frames[:2])
        g.sync()
        names = set(g.kernel_times())
    finally:
        g.close()
    return {c for c, k in CHAIN_KERNEL.items() if any(n.startswith(k) for n in names)}, names


@pytest.mark.parametrize("name", list(GEOMS))
def test_geometry_runs_the_chain_its_cases_mean(monkeypatch, name):
    geom, chain = GEOMS[name]
    _set_wgs(monkeypatch, chain, WGS[chain][0])
    ran, names = _chain_run(geom, _job(name)[1])
    assert ran == {chain}, f"{name}: kernels {sorted(names)}"


# ---- D: the caps ----------------------------------------------------------------------------------------------------------------

class Bound(NamedTuple):
    geom: Geom
    chain: str
    fields: tuple   # per plane
    frames: int
    env: tuple      # ((variable, value), ...)
    kind: int       # the list the case is about: 0 luma, 1 chroma (stream: the one list of both launches)
    units: int      # the designed length of that list
    longest: int    # ... of its longest slice (stream: see the CPU test)


BOUNDS = {
    # 6 x 50 = 300 luma cells, three workgroups a frame: slices of exactly kWMaxUnits = 100 whose cuts fall mid-row
    "wide_luma_100": Bound(Geom(768, 1600, 10, 10, 1, 1, 3, False), "wide", ("extremes",), 2, (("G1S_W_WGS", "3"),), 0, 300, 100),
    # 3 x 32 = 96 chroma cells of 8 blocks, three workgroups: slices of kWMaxUnitsC = 32 (16 steps a unit)
    "wide_chroma_32_420": Bound(Geom(768, 1024, 8, 8, 1, 1, 3), "wide", ("quads", "extremes", "extremes"), 2, (("G1S_W_WGS_C", "3"),), 1, 96, 32),
    # 6 x 16 = 96 chroma cells of 4 blocks: 32 steps a unit, the header's 2^30
    "wide_chroma_32_444": Bound(Geom(768, 512, 8, 8, 0, 0, 3), "wide", ("extremes",) * 3, 2, (("G1S_W_WGS_C", "3"),), 1, 96, 32),
    # 28 x 64 = 1792 stream units = 8 x (kMMaxUnits - 16): eight workgroups a frame is the fewest the engine allows
    "stream_224": Bound(Geom(1790, 2046, 8, 8, 1, 1, 2), "stream", ("quads", "extremes", "extremes"), 1, (("G1S_F_WGS", "8"),), 0, 1792, 224),
    # 3 x 101 = 303 luma cells: one row of cells over three workgroups' cap -- the engine must cut four slices
    "wide_luma_over": Bound(Geom(384, 3232, 10, 10, 1, 1, 3, False), "wide", ("extremes",), 1, (("G1S_W_WGS", "3"),), 0, 303, 76),
}


@functools.lru_cache(maxsize=None)
def _bound_job(name: str):
    b = BOUNDS[name]
    sp = Spec("D", name, (), (), b.fields, ())
    fields = [residuals(b.geom, k, sp) for k in range(b.frames)]
    frames, shadows = _run_oracle(b.geom, fields)
    return fields, frames, shadows


def _bound_check(monkeypatch, name, env=None):
    b = BOUNDS[name]
    for var, val in (b.env if env is None else env):
        monkeypatch.setenv(var, val)
    _, frames, shadows = _bound_job(name)
    return _check(b.geom, frames, shadows, [f"{name}, {dict(b.env if env is None else env)}"] * len(frames), 2)


@pytest.mark.parametrize("name", list(BOUNDS))
def test_d_slices_of_the_caps_length(monkeypatch, name):
    _bound_check(monkeypatch, name)


def test_d_fewer_workgroups_than_the_cap_allows_are_raised(monkeypatch):
    """G1S_W_WGS = 1 on 300 cells: the engine must raise it to 3 (w_wgs_per_frame's gmin) -- one slice of 300 would overflow the
    int32 accumulators and the parked entries.  The records equal the oracle's and, byte for byte, those of the run with 3."""
    three = _bound_check(monkeypatch, "wide_luma_100")
    one = _bound_check(monkeypatch, "wide_luma_100", (("G1S_W_WGS", "1"),))
    for i, (a, b) in enumerate(zip(three, one)):
        diff = np.flatnonzero(a.view(np.uint8).ravel() != b.view(np.uint8).ravel())
        assert diff.size == 0, f"frame {i}: {diff.size} record bytes differ between G1S_W_WGS=3 and =1, first at {diff[0]}"


@pytest.mark.parametrize("name", list(BOUNDS))
def test_bound_geometry_runs_the_chain_it_means(monkeypatch, name):
    b = BOUNDS[name]
    for var, val in b.env:
        monkeypatch.setenv(var, val)
    ran, names = _chain_run(b.geom, _bound_job(name)[1])
    assert ran == {b.chain}, f"{name}: kernels {sorted(names)}"
