"""Every frame's record against the oracle's integers on DESIGNED flat-block masks (tests/mask_content.py): isolated flat
blocks, columns, rows, pairs across unit boundaries, one block a unit, stairs, random masks from sparse to nearly full -- a
different design in every frame of a job, so the pattern changes inside a batch.  What the accumulation kernels decide from the
pattern around a flat block (observation windows, the fast path, whether a list neighbour is a spatial neighbour, what is
deferred beside what) is met on purpose here and only by accident of the finder on the rectangles of tests/content.py.

Compared per frame, exactly: mask bytes, f32 score bits, S, Sb and nobs of every plane, luma_sum, sum_d and sum_d2.  What the
oracle's masks of these jobs reach is asserted without a device in tests/test_mask_content_cpu.py; the oracle runs once per
geometry here and its shadows are shared by the cases."""
import functools

import pytest

from tests import mask_content as MC
from tests.helpers import oracle_shadow, record_mismatches
from tests.oracle_binding import OracleDiff, format_tbl as oracle_tbl
from tests.test_gpu_records import CHAIN_KERNEL, FPS, SLOTS, Geom, _feed, _generator

pytestmark = pytest.mark.gpu

BATCH = 5
# the smallest sizes with at least 5 luma units and 2 whole chroma units and a part of one in a block row (4:4:4: 4 and 4)
GEOMS = {
    "8b420_640x352_lag3": (Geom(640, 352, 8, 8, 1, 1, 3), "wide"),
    "10b420_656x340_lag2": (Geom(656, 340, 10, 10, 1, 1, 2), "wide"),     # a 16-sample last block column, a 20-row last block row
    "10b444_512x256_lag3": (Geom(512, 256, 10, 10, 0, 0, 3), "wide"),     # chroma units of 4 blocks
    "10b422_640x328_lag1": (Geom(640, 328, 10, 10, 1, 0, 1), "wide"),     # an 8-row last block row
    "8b_luma_only_640x352_lag3": (Geom(640, 352, 8, 8, 1, 1, 3, False), "wide"),
    # the last luma block column 6 samples wide (whether it counts depends on its left neighbour), the last chroma column 3
    "8b420_646x342_lag2_stream": (Geom(646, 342, 8, 8, 1, 1, 2), "stream"),
    "10_8_444_512x256_lag3_stream": (Geom(512, 256, 10, 8, 0, 0, 3), "stream"),
}
WIDE, STREAM = "8b420_640x352_lag3", "8b420_646x342_lag2_stream"


def job_designs(geom: Geom):
    """[(name, design)] of the geometry's job, one frame each: every design of mask_content.designs, in its order."""
    return list(MC.designs((geom.h + 31) // 32, (geom.w + 31) // 32).items())


@functools.lru_cache(maxsize=None)
def _job(geom: Geom, damage: bool = False):
    """Frame k carries design k (host planes); the oracle's shadows of every frame, and its table."""
    o = OracleDiff(FPS.numerator, FPS.denominator, geom.src_bd, geom.den_bd, geom.lag, geom.chroma)
    frames, shadows = [], []
    for k, (_, design) in enumerate(job_designs(geom)):
        s = MC.make_frames(design, geom.w, geom.h, geom.src_bd, geom.xd, geom.yd, k, damage=damage)[0]
        d = MC.make_frames(design, geom.w, geom.h, geom.den_bd, geom.xd, geom.yd, k, damage=damage)[1]
        if not geom.chroma:
            s, d = s[:1], d[:1]
        o.diff_frame(s, d, geom.xd, geom.yd)
        frames.append((s, d))
        shadows.append(oracle_shadow(o, len(s)))
    return frames, shadows, oracle_tbl(o.finish())


def _check_job(geom: Geom, damage: bool = False):
    from grav1synth_amd.diff import Record

    frames, shadows, _ = _job(geom, damage)
    names = [n for n, _ in job_designs(geom)]
    assert len(frames) % BATCH and len(frames) > 2 * BATCH, "a short last batch behind full ones"
    g = _generator(geom, BATCH, records_only=True)
    try:
        _feed(g, geom, frames)
        recs, n = g.take_records(geom.w, geom.h, 3 if geom.chroma else 1, len(frames))
        assert n == len(frames), f"{n} records for {len(frames)} frames"
        bad = []
        for i in range(n):
            j = i // BATCH
            where = f"design {names[i]}, frame {i} (batch {j}, position {i % BATCH}, slot {j % SLOTS})"
            bad.extend(record_mismatches(shadows[i], Record(recs[i]), where))
    finally:
        g.close()
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("name", list(GEOMS))
def test_geometry_runs_the_chain_its_cases_mean(name):
    """As tests/test_gpu_records.py holds its geometries: k3w_pass in the timed kernels is the wide chain, k3s_fused the stream
    chain."""
    geom, chain = GEOMS[name]
    frames = _job(geom)[0][:2]
    g = _generator(geom, 2, records_only=True)
    try:
        g.set_timing(True)
        _feed(g, geom, frames)
        g.sync()
        names = set(g.kernel_times())
    finally:
        g.close()
    ran = {c for c, k in CHAIN_KERNEL.items() if any(n.startswith(k) for n in names)}
    assert ran == {chain}, f"{name}: kernels {sorted(names)}"


@pytest.mark.parametrize("name", list(GEOMS))
def test_every_record_of_a_job_of_designed_masks(name):
    _check_job(GEOMS[name][0])


@pytest.mark.parametrize("reuse,f_wgs,w_wgs", [("1", "8", "8"), ("0", "64", "264"), ("0", "8", "8"), ("1", "64", "264")])
@pytest.mark.parametrize("name", [WIDE, STREAM])
def test_every_record_with_few_and_with_many_workgroups(monkeypatch, name, reuse, f_wgs, w_wgs):
    """G1S_W_WGS[_C] 8 and 264 (the wide chain), G1S_F_WGS 8 and 64 with G1S_F_REUSE 1 and 0 (the stream chain): the slices'
    boundaries fall between adjacent units and between units that are no neighbours."""
    monkeypatch.setenv("G1S_F_REUSE", reuse)
    monkeypatch.setenv("G1S_F_WGS", f_wgs)
    monkeypatch.setenv("G1S_W_WGS", w_wgs)
    monkeypatch.setenv("G1S_W_WGS_C", w_wgs)
    _check_job(GEOMS[name][0])


@pytest.mark.parametrize("name", [WIDE, STREAM])
def test_every_record_with_deferred_units_beside_multiplied_ones(name):
    """damage=True: residuals outside int8 in every third 4-block cell of a block row -- a deferred unit beside flat units that are
    still multiplied, a deferred luma unit above chroma units that are (k3w_tail / k3_ar_generic take the deferred blocks)."""
    _check_job(GEOMS[name][0], damage=True)


@pytest.mark.parametrize("where", ["host", "device"])
def test_folding_generator_gives_the_oracles_table(monkeypatch, where):
    """The whole job's .tbl under both halves of the per-frame fold."""
    from grav1synth_amd.diff import format_tbl

    geom = GEOMS[WIDE][0]
    monkeypatch.setenv("G1S_LATEST", where)
    frames, _, want = _job(geom)
    g = _generator(geom, BATCH)
    try:
        g.set_timing(True)
        _feed(g, geom, frames)
        got = format_tbl(g.finish())
        on_device = "k4_latest" in g.kernel_times()
    finally:
        g.close()
    assert got == want
    assert on_device == (where == "device")
