"""A chroma gain for the joint chroma filter (include/g1s_diff.h, "denoise", rules 21 - 24 and N9) without a device:
the numpy restatement (tests/denoise_gain_ref.py) against a plain loop over pairs, the host-only builders of the library
against the restatement byte for byte, every refusal with its text, the identities the rules state, the cases that show
that the GPU tests' content bites, and one statistical test of the definition."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from grav1synth_amd import _lib
from grav1synth_amd.diff import GrainTableSegment
from tests import denoise_gain_ref as G
from tests import denoise_joint_ref as J
from tests import nlf_ref as NR


def seg(y=(), cb=(), cr=(), cbm=(128, 192, 256), crm=(128, 192, 256), csfl=False):
    """A segment with the given scaling points; (mult, luma_mult, offset) a chroma plane.  The defaults are what fold.cpp writes."""
    return GrainTableSegment(random_seed=1, start_time=0, end_time=1 << 62, scaling_points_y=list(y), scaling_points_cb=list(cb),
                             scaling_points_cr=list(cr), scaling_shift=8, ar_coeff_lag=0, ar_coeffs_y=[], ar_coeffs_cb=[0], ar_coeffs_cr=[0],
                             ar_coeff_shift=6, cb_mult=cbm[0], cb_luma_mult=cbm[1], cb_offset=cbm[2], cr_mult=crm[0], cr_luma_mult=crm[1],
                             cr_offset=crm[2], chroma_scaling_from_luma=csfl, grain_scale_shift=0, overlap_flag=False)


def random_points(rng, most):
    n = int(rng.integers(0, most + 1))
    xs = np.sort(rng.choice(256, n, replace=False))
    return [(int(x), int(rng.integers(0, 256))) for x in xs]


def lib_gain(segments, range_=0, segment=None):
    from grav1synth_amd.denoise import chroma_gain

    return chroma_gain(segments, range_, segment)


# ------------------------------------------------------------------------------- the restatement against a plain loop
def _small(seed, bd, n=1):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, 1 << bd, (7, 9)).astype(np.int64) for _ in range(3)] for _ in range(n)]


@pytest.mark.parametrize("bd,A,S", [(8, 3, 2), (12, 2, 1), (10, 1, 4)])
def test_the_restatement_equals_a_plain_loop_over_pairs_on_a_9_x_7_chroma_plane(bd, A, S):
    from grav1synth_amd.denoise import weight_table

    T, q = weight_table(bd, S, 80.0, joint_chroma=True)
    gain = np.random.default_rng(bd).integers(1, 16385, 256).astype(np.uint16)
    cur, nb = _small(bd, bd, 2)
    for vs, mv in ((None, None), (nb, None), (nb, np.array([[[2, -2]]])), (nb, np.array([[[-6, 4]]]))):
        (a, b), d = G.sums(cur, vs, mv, A, S, T, q, gain, bd - 8)
        (a2, b2), d2 = G.sums_pairs(cur, vs, mv, A, S, T, q, gain, bd - 8)
        assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(d, d2), (vs is None, mv)


# ---------------------------------------------------------------------------------------------------------- the builders
RAMP = [(0, 20), (64, 60), (128, 140), (255, 250)]
BUMP = [(16, 200), (100, 30), (235, 90)]


def test_rule_21_bounds_and_the_flat_gain():
    rng = np.random.default_rng(21)
    for R in range(1, 9):
        for _ in range(400):
            s = np.array(G.scaling_lut(random_points(rng, 10)), np.uint8)
            m = G.gain_from_s(s, R)
            assert 256 // (R * R) <= int(m.min()) and int(m.max()) <= 256 * R * R <= 16384, (R, m.min(), m.max())
            assert int(m.min()) >= 4
    assert np.array_equal(G.gain_from_s(np.zeros(256, np.uint8)), G.FLAT)
    assert np.array_equal(G.gain_from_s(np.array(G.scaling_lut(RAMP), np.uint8), 1), G.FLAT)


@pytest.mark.parametrize("R", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_the_table_builder_equals_the_restatement_byte_for_byte(R):
    own = seg(y=RAMP, cb=RAMP, cr=BUMP)                                   # a table of diff's own kind: idx = v
    assert [G.chroma_index(v, 192, 128, 256) for v in range(256)] == list(range(256))
    from_luma = seg(y=BUMP, cb=RAMP, cr=RAMP, csfl=True)                  # the luma points', whatever the chroma points say
    low = seg(y=RAMP, cb=RAMP, cr=BUMP, cbm=(100, 160, 230), crm=(128, 255, 200))   # idx clips at 0 ...
    high = seg(y=RAMP, cb=RAMP, cr=BUMP, cbm=(200, 255, 300), crm=(160, 64, 256))   # ... and at 255; a negative luma slope
    idx_low = [G.chroma_index(v, 160, 100, 230) for v in range(256)]
    idx_high = [G.chroma_index(v, 255, 200, 300) for v in range(256)]
    assert idx_low[0] == 0 and idx_low.count(0) > 1 and idx_high[-1] == 255 and idx_high.count(255) > 1
    none = seg(y=RAMP)                                                    # no chroma points: all zeros, the flat gain
    for segs in ([own], [from_luma], [low], [high], [none], [own, high], [own, from_luma, low]):
        want = G.chroma_gain(segs, R)
        got = lib_gain(segs, R)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (R, np.argwhere(got != want)[:4])
    assert np.array_equal(lib_gain([none], R), G.FLAT)
    assert np.array_equal(G.s_from_segments([from_luma]), np.array(G.scaling_lut(BUMP), np.uint8))
    two = lib_gain([own, high], R)
    if R not in (1,):
        assert not np.array_equal(two, lib_gain([own], R)) and not np.array_equal(two, lib_gain([high], R))
    assert np.array_equal(lib_gain([own, high], R, segment=1), lib_gain([high], R))


def test_the_table_builder_on_random_point_sets_and_its_bounds():
    rng = np.random.default_rng(22)
    steep = 0
    for i in range(2000):
        mults = lambda: (int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 512)))  # noqa: E731
        s = seg(y=random_points(rng, 14), cb=random_points(rng, 10), cr=random_points(rng, 10), cbm=mults(), crm=mults(), csfl=bool(rng.integers(0, 4) == 0))
        R = int(rng.integers(1, 9))
        got = lib_gain([s], R)
        assert np.array_equal(got, G.chroma_gain([s], R)), i
        assert 4 <= int(got.min()) and int(got.max()) <= 16384
        steep += int(got.max()) == 16384
    print("random point sets that reach 16384:", steep)


def test_rule_21_on_a_given_s_equals_the_restatement():
    L = _lib.lib()
    rng = np.random.default_rng(23)
    for R in range(0, 9):
        s = rng.integers(0, 256, 256).astype(np.uint8)
        got = np.zeros(256, np.uint16)
        assert L.g1s_denoise_chroma_gain_sigma(s.ctypes.data, R, got.ctypes.data) == 0
        assert np.array_equal(got, G.gain_from_s(s, R))
    # a steep one: s' is the floor ceil(255 / 8) = 32 below 200 and 255 from there on, so the two multipliers are (255 / 32)^2 =
    # 63.5 apart, up to their rounding
    s = np.full(256, 1, np.uint8)
    s[200:] = 255
    m = G.gain_from_s(s, 8)
    assert m.min() >= 4 and m.max() <= 16384 and 60 * int(m[255]) < int(m[0]) < 66 * int(m[255])


# ---------------------------------------------------------------------------------------------------------------- rule 23
def _record(n1, q1, n2=None, q2=None):
    rec = NR.empty_record()
    rec["n"][1], rec["q"][1] = n1, q1
    rec["n"][2], rec["q"][2] = (n1 if n2 is None else n2), (q1 if q2 is None else q2)
    rec["n"][0, :] = 10 ** 6  # (luma takes no part in N9)
    rec["q"][0, :] = 10 ** 9
    return rec


def _lib_chroma_sigma(rec, min_count=0):
    from grav1synth_amd.estimate import NLF_RECORD, noise_chroma_sigma

    return noise_chroma_sigma(NR.to_struct(rec, NLF_RECORD), min_count)


def test_rule_23_equals_the_restatement_on_designed_records():
    from grav1synth_amd._lib import G1SError

    rng = np.random.default_rng(24)
    z = np.zeros(32, np.uint64)
    with pytest.raises(G1SError, match="no chroma bin has enough smooth samples for a prior"):
        _lib_chroma_sigma(_record(z, z))
    with pytest.raises(ValueError, match="no chroma bin has enough smooth samples for a prior"):
        G.chroma_sigma(_record(z, z))
    # one valid bin: s is flat at 255
    n = z.copy()
    n[9] = 3000
    q = (n * 36 * 40).astype(np.uint64)
    one = _lib_chroma_sigma(_record(n, q))   # pooled: 6000 >= 4096
    assert np.array_equal(one, G.chroma_sigma(_record(n, q))) and (one == 255).all()
    # the count one below and on Nmin, pooled over the two planes
    for nmin in (0, 777):
        edge = nmin or 4096
        a, b = z.copy(), z.copy()
        a[3], b[3] = edge // 2, edge - edge // 2 - 1
        a[20], b[20] = edge, 0
        qa, qb = (a * 36 * 9).astype(np.uint64), (b * 36 * 400).astype(np.uint64)
        below = _lib_chroma_sigma(_record(a, qa, b, qb), nmin)
        assert np.array_equal(below, G.chroma_sigma(_record(a, qa, b, qb), nmin)) and (below == 255).all(), "bin 3 is one short: bin 20 alone"
        b[3] += 1
        qb = (b * 36 * 400).astype(np.uint64)
        on = _lib_chroma_sigma(_record(a, qa, b, qb), nmin)
        assert np.array_equal(on, G.chroma_sigma(_record(a, qa, b, qb), nmin)) and on[0] != on[255], "on Nmin the bin takes part"
    # gaps between valid bins, random levels
    for _ in range(50):
        n = np.where(rng.random(32) < 0.4, rng.integers(4096, 10 ** 6, 32), rng.integers(0, 2048, 32)).astype(np.uint64)
        q = (n * rng.integers(1, 5000, 32).astype(np.uint64)).astype(np.uint64)
        n2 = rng.integers(0, 2048, 32).astype(np.uint64)
        q2 = (n2 * rng.integers(1, 5000, 32).astype(np.uint64)).astype(np.uint64)
        rec = _record(n, q, n2, q2)
        try:
            want = G.chroma_sigma(rec)
        except ValueError:
            continue
        got = _lib_chroma_sigma(rec)
        assert np.array_equal(got, want) and got.min() >= 1


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_rule_23_on_the_record_of_a_clip_of_any_depth(bd):
    """The record of tests/nlf_ref.py on a small grainy 4:2:0 frame whose chroma grain grows with the luma under it: the same
    256-entry function at every depth's own record, rising with v -- a 12-bit clip included."""
    from grav1synth_amd.estimate import NLF_RECORD, noise_chroma_prior

    rng = np.random.default_rng(bd)
    top = (1 << bd) - 1
    yy = np.repeat(np.linspace(0.1, 0.9, 64)[None, :], 48, 0)
    luma = np.repeat(np.repeat(yy, 2, 0), 2, 1) * top
    sig = (1.0 + 5.0 * yy) * (1 << (bd - 8))
    frame = [np.clip(np.rint(luma), 0, top).astype(np.uint16 if bd > 8 else np.uint8)]
    frame += [np.clip(np.rint(top / 2 + rng.normal(0, 1, yy.shape) * sig), 0, top).astype(frame[0].dtype) for _ in range(2)]
    rec = NR.nlf_frame(frame, bd, 1, 1)
    want = G.chroma_sigma(rec, 64)
    got = _lib_chroma_sigma(rec, 64)
    assert np.array_equal(got, want)
    assert int(want[240]) > 2 * int(want[16]), (want[16], want[240])
    assert np.array_equal(noise_chroma_prior(NR.to_struct(rec, NLF_RECORD), 8, 64), G.gain_from_s(want, 8))


# -------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_with_its_text():
    from grav1synth_amd._lib import G1SError
    from grav1synth_amd.denoise import Denoiser

    L = _lib.lib()
    err = lambda: L.g1s_last_global_error().decode()  # noqa: E731
    gain = np.zeros(256, np.uint16)
    good = seg(y=RAMP, cb=RAMP, cr=BUMP)
    arr = (_lib.G1SSegment * 1)(good.to_c())
    assert L.g1s_denoise_chroma_gain(arr, 0, 0, gain.ctypes.data) != 0 and err() == "a grain prior needs at least one segment"
    assert L.g1s_denoise_chroma_gain(arr, 1, 9, gain.ctypes.data) != 0 and err() == "chroma gain range must be 1..8 (0 = the default)"
    assert L.g1s_denoise_chroma_gain(arr, 1, 8, gain.ctypes.data) == 0
    s = np.zeros(256, np.uint8)
    assert L.g1s_denoise_chroma_gain_sigma(s.ctypes.data, 9, gain.ctypes.data) != 0 and err() == "chroma gain range must be 1..8 (0 = the default)"
    for field, text in (("scaling_points_y", "luma"), ("scaling_points_cb", "chroma"), ("scaling_points_cr", "chroma")):
        bad = seg(y=RAMP, cb=RAMP, cr=BUMP)
        setattr(bad, field, [(10, 5), (10, 9)])
        with pytest.raises(G1SError, match=f"segment 1: {text} scaling points must have increasing values"):
            lib_gain([good, bad])
    with pytest.raises(G1SError, match=r"segment 3 is not in the table \(2 segments\)"):
        lib_gain([good, good], segment=3)
    # the constructor: checked before a device is looked for, so they read the same on a machine without one
    flat = G.FLAT.copy()
    for i, v in ((0, 0), (255, 16385), (77, 65535)):
        g = flat.copy()
        g[i] = v
        with pytest.raises(G1SError, match=rf"chroma gain must be 1\.\.16384 \(at {i}\)"):
            Denoiser(10, joint_chroma=True, chroma_gain=g)
    with pytest.raises(G1SError, match="a chroma gain needs joint chroma"):
        Denoiser(10, chroma_gain=flat)
    with pytest.raises(G1SError, match="a chroma gain needs joint chroma"):
        Denoiser(12, temporal_radius=1, motion_range=8, chroma_gain=flat)
    with pytest.raises(G1SError, match="256 entries"):
        Denoiser(10, joint_chroma=True, chroma_gain=flat[:255])
    with pytest.raises(G1SError, match="256 entries"):
        Denoiser(10, joint_chroma=True, chroma_gain=np.full(256, 70000))


def test_the_file_calls_refuse_before_they_look_for_a_device(tmp_path):
    import os

    from grav1synth_amd.denoise import denoise_opts

    L = _lib.lib()
    example = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference-example-table.tbl").encode()
    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 C420\nFRAME\n" + bytes(12))
    opts, err = denoise_opts(), C.create_string_buffer(512)
    JOINT, AUTO_PRIOR = _lib.G1S_DENOISE_JOINT_CHROMA, _lib.G1S_AUTO_PRIOR

    def dn(flags, tbl, rng, auto, chroma):
        rc = L.g1s_denoise_y4m_file_chroma(str(src).encode(), str(tmp_path / "o.y4m").encode(), C.byref(opts), 0, flags, tbl, rng, -1, 0, auto, 0, 0, chroma,
                                           err, len(err))
        return rc, err.value.decode()

    def df(flags, tbl, rng, auto, chroma):
        n = C.c_uint64()
        rc = L.g1s_diff_y4m_file_denoised_chroma(str(src).encode(), str(tmp_path / "o.tbl").encode(), None, None, C.byref(opts), 0, flags, tbl, rng, -1, 0,
                                                 auto, 0, 0, chroma, C.byref(n), err, len(err))
        return rc, err.value.decode()

    for call in (dn, df):
        rc, text = call(JOINT, None, 0, 0, 1)
        assert rc < 0 and text == "a chroma prior needs a grain prior (a table or the clip's own levels)"
        rc, text = call(0, example, 0, 0, 1)
        assert rc < 0 and text == "a chroma gain needs joint chroma"
        rc, text = call(0, None, 0, AUTO_PRIOR, 1)
        assert rc < 0 and text == "a chroma gain needs joint chroma"
        rc, text = call(JOINT, example, 0, 0, 2)
        assert rc < 0 and text == "chroma_prior is 0 or 1"
        rc, text = call(JOINT, example, 9, 0, 1)   # valid for luma at 8 bits, refused for chroma with rule 21's text
        assert rc < 0 and text == "chroma gain range must be 1..8 (0 = the default)"
    assert not (tmp_path / "o.y4m").exists() and not (tmp_path / "o.tbl").exists()


def test_the_command_line_refusals_are_one_logged_line(tmp_path, caplog):
    import os

    from grav1synth_amd import cli

    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 C420\nFRAME\n" + bytes(12))
    example = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference-example-table.tbl")
    out, tbl = tmp_path / "o.y4m", tmp_path / "t.tbl"

    def one_line(text, call):
        caplog.clear()
        with caplog.at_level("INFO", logger="grav1synth"):
            assert call() == -1
        assert [r.getMessage() for r in caplog.records] == [text]

    dn = lambda **kw: cli.denoise_command(str(src), str(out), **kw)  # noqa: E731
    df = lambda **kw: cli.diff_command(str(src), None, str(tbl), denoise=True, **kw)  # noqa: E731
    for run in (dn, df):
        one_line(cli.CHROMA_PRIOR_NEEDS_PRIOR, lambda: run(chroma_prior=True, joint_chroma=True))
        one_line(cli.CHROMA_PRIOR_NEEDS_JOINT, lambda: run(chroma_prior=True, grain_prior=example))
        one_line(cli.CHROMA_PRIOR_NEEDS_JOINT, lambda: run(chroma_prior=True, auto_prior=True))
        one_line(cli.CHROMA_PRIOR_BAD_RANGE, lambda: run(chroma_prior=True, joint_chroma=True, grain_prior=example, prior_range=9))
    assert not out.exists() and not tbl.exists()
    a = cli.build_parser().parse_args(["diff", "s.y4m", "--denoise", "-o", "t.tbl", "--joint-chroma", "--auto-prior", "--chroma-prior"])
    assert cli._denoise_parameters(a)["chroma_prior"] is True
    a = cli.build_parser().parse_args(["denoise", "in.y4m", "-o", "out.y4m"])
    assert cli._denoise_parameters(a)["chroma_prior"] is False


# ------------------------------------------------------------------------------------------------------------ identities
def test_the_flat_gain_gives_the_bytes_of_the_joint_reference():
    from grav1synth_amd.denoise import weight_table

    bd, sub = 10, (1, 1)
    clean, noisy = J.edge_content(seed=9)
    clip = [noisy, [np.ascontiguousarray(np.roll(p, 1, 1)) for p in noisy]]
    T, q = weight_table(bd, 2, 6.0, joint_chroma=True)
    want = J.denoise_chroma_clip(clip, *sub, 1, 3, 2, T, q)
    got = G.denoise_chroma_clip(clip, *sub, 1, 3, 2, T, q, G.FLAT, bd)
    for (a, b), (c, d) in zip(got, want):
        assert np.array_equal(a, c) and np.array_equal(b, d)
    other = G.denoise_chroma_clip(clip, *sub, 1, 3, 2, T, q, np.where(np.arange(256) < 128, 64, 1024).astype(np.uint16), bd)
    assert (other[0][0] != want[0][0]).any()


def test_mp_is_symmetric_so_one_weight_serves_both_ends_of_a_pair():
    """w(p, d) = w(p + d, -d) for every pair that takes part: what the half-plane walk of dn_spatial relies on.  Read off a
    one-offset window: with the search reduced to {0, d} the denominator is 4096 + w(p, d)."""
    from grav1synth_amd.denoise import weight_table

    bd, S = 8, 1
    T, q = weight_table(bd, S, 40.0, joint_chroma=True)
    us = _small(5, bd)[0]
    gain = np.where(np.arange(256) < 100, 4, 16384).astype(np.uint16)
    h, w = us[0].shape

    def weight(y, x, dy, dx):
        D = 0
        cl = lambda v, n: min(max(v, 0), n - 1)  # noqa: E731
        for ky in range(-S, S + 1):
            for kx in range(-S, S + 1):
                for a in us:
                    D += (int(a[cl(y + ky, h), cl(x + kx, w)]) - int(a[cl(y + dy + ky, h), cl(x + dx + kx, w)])) ** 2
        mp = (int(gain[int(us[2][y, x])]) + int(gain[int(us[2][y + dy, x + dx])]) + 1) >> 1
        return int(T[min((D * mp) >> (q + 8), 1023)])

    seen = set()
    for y in range(h):
        for x in range(w):
            for dy, dx in ((0, 1), (1, -2), (2, 2), (1, 0)):
                if 0 <= y + dy < h and 0 <= x + dx < w:
                    assert weight(y, x, dy, dx) == weight(y + dy, x + dx, -dy, -dx)
                    seen.add((int(us[2][y, x]) < 100, int(us[2][y + dy, x + dx]) < 100))
    assert len(seen) == 4, "pairs with equal and with different gains at their ends"
    # and a restatement that swaps the ends gives the same sums
    swapped = lambda m, ga, gb, sh: G.pair_gain(m, gb, ga, sh)  # noqa: E731
    (a, b), d = G.sums(us, None, None, 2, S, T, q, gain, 0)
    (a2, b2), d2 = G.sums(us, None, None, 2, S, T, q, gain, 0, pair=swapped)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(d, d2)


# ------------------------------------------------------------------------------------- the GPU tests' content bites
def step_guide_frame(bd=10, w=200, h=120, seed=3):
    """4:2:0, chroma 100 x 60 (two tiles across, two down): the guide's level changes inside the first tile (x = 40), across
    the tile boundary (x = 64 is one level, x = 63 another: a second step at 64) and along y = 30; grainy chroma."""
    rng = np.random.default_rng(seed)
    top = (1 << bd) - 1
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    level = np.where((xx < 80) | ((xx >= 128) & (yy >= 60)), top // 4, 3 * top // 4)
    luma = np.clip(level + rng.integers(-3, 4, (h, w)), 0, top)
    dt = np.uint16 if bd > 8 else np.uint8
    chroma = [np.clip(np.rint(top / 2 + rng.normal(0, 6.0 * (1 << (bd - 8)), (h // 2, w // 2))), 0, top).astype(dt) for _ in range(2)]
    return [luma.astype(dt)] + chroma


def step_gain(level=128):
    return np.where(np.arange(256) < level, 4, 16384).astype(np.uint16)


def test_a_gain_taken_at_p_alone_differs_on_the_step_gain_content():
    from grav1synth_amd.denoise import weight_table

    bd = 10
    frame = step_guide_frame(bd)
    T, q = weight_table(bd, 2, 6.0, joint_chroma=True)
    right = G.denoise_chroma_clip([frame], 1, 1, 0, 3, 2, T, q, step_gain(), bd)[0]
    at_p = lambda m, ga, gb, sh: m[np.minimum(ga >> sh, 255)] + 0 * gb  # noqa: E731
    wrong = G.denoise_chroma_clip([frame], 1, 1, 0, 3, 2, T, q, step_gain(), bd, pair=at_p)[0]
    diff = np.argwhere(right[0] != wrong[0])
    assert len(diff) > 0
    assert (np.abs(diff[:, 1] - 40) <= 3).any() and (np.abs(diff[:, 1] - 64) <= 3).any(), "inside a tile and across a tile boundary"
    flat = G.denoise_chroma_clip([frame], 1, 1, 0, 3, 2, T, q, G.FLAT, bd)[0]
    assert (flat[0] != right[0]).any()


@pytest.mark.parametrize("strength", [1000.0, 100.0])
def test_a_product_wrapped_to_32_bits_differs_on_the_ceiling_content(strength):
    """12 bit, S = 4, Cb, Cr and G 0 / 4095 checkerboards, gain 16384: D_J mp = 4 074 873 075 x 2^14 passes 2^32.  At strength
    1000 (q_J = 30) the right weight is T_J[242] = 62, at strength 100 it is T_J[1023] = 0; a product wrapped to 32 bits looks up
    T_J[0] = 4096 at either."""
    from grav1synth_amd.denoise import weight_table
    from tests.test_denoise_joint_cpu import ceiling_frame

    A, S, sub, bd = 1, 4, (1, 1), 12
    frame = ceiling_frame(40, 30, *sub)
    assert J.max_distance(frame, *sub, A, S) == 4074873075
    T, q = weight_table(bd, S, strength, joint_chroma=True)
    gain = np.full(256, 16384, np.uint16)
    prod = 4074873075 * 16384
    assert prod >= 2 ** 32 and prod < 2 ** 47
    assert int(T[min(prod >> (q + 8), 1023)]) == (62 if strength == 1000.0 else 0) and int(T[min((prod & 0xFFFFFFFF) >> (q + 8), 1023)]) == 4096
    right = G.denoise_chroma_clip([frame], *sub, 0, A, S, T, q, gain, bd)[0]
    wrong = G.denoise_chroma_clip([frame], *sub, 0, A, S, T, q, gain, bd, wrap32=True)[0]
    assert (right[0] != wrong[0]).any() or (right[1] != wrong[1]).any()


def pan_clip(n, w, h, bd, shift=(3, -2), seed=4, sigma=2.0):
    """n frames of 4:2:0 on tests/motion_content.py's pan: the chroma planes (full-range noise: a block matches at one place
    only) move by `shift` an interval, the luma plane (texture: the guide runs over about half of the gain's entries) by twice
    that; independent grain on every frame."""
    from tests import motion_content as MC

    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    y = MC.pan([seed, 0], w, h, bd, [(2 * shift[0], 2 * shift[1])] * (n - 1), sigma, "texture")[1]
    cb = MC.pan([seed, 1], cw, ch, bd, [shift] * (n - 1), sigma)[1]
    cr = MC.pan([seed, 2], cw, ch, bd, [shift] * (n - 1), sigma)[1]
    return MC.clip([y, cb, cr])


def test_a_gain_looked_up_at_the_unmoved_place_differs_under_motion():
    from grav1synth_amd.denoise import weight_table
    from tests import denoise_motion_ref as M

    bd, mr = 10, 8
    clip = pan_clip(2, 136, 104, bd)
    us, vs = J._triple(clip[0], 1, 1), J._triple(clip[1], 1, 1)
    mv = M.search(us[:2], vs[:2], mr)
    assert np.abs(mv).max() > 0, "the search finds the pan"
    T, q = weight_table(bd, 2, 6.0, joint_chroma=True)
    gain = np.random.default_rng(8).integers(1, 16385, 256).astype(np.uint16)
    right = G.sums(us, vs, mv, 3, 2, T, q, gain, 2)
    wrong = G.sums(us, vs, mv, 3, 2, T, q, gain, 2, unmoved_guide=True)
    assert (right[1] != wrong[1]).any()


# ----------------------------------------------------------------------------------- the definition, statistically
def two_halves(seed=7):
    """10-bit 4:2:0, luma 128 x 96, chroma 64 x 48.  Left half: dark luma (200), chroma grain sigma 4; right half: bright luma
    (800), chroma grain sigma 16; luma grain sigma 6 on both.  A weak chroma edge, co-located in Cb and Cr, runs along y = 24
    through both halves: 12 code values.  Returns (clean, noisy)."""
    rng = np.random.default_rng(seed)
    xx, yy = np.arange(128)[None, :], np.arange(96)[:, None]
    cx, cy = np.arange(64)[None, :], np.arange(48)[:, None]
    luma = np.where(xx < 64, 200, 800) + 0 * yy
    step = np.where(cy < 24, -6, 6) + 0 * cx
    clean = [luma, 512 + step, 512 - step]
    sig = [6.0, np.where(cx < 32, 4.0, 16.0) + 0 * cy, np.where(cx < 32, 4.0, 16.0) + 0 * cy]
    noisy = [np.clip(np.rint(p + rng.normal(0.0, 1.0, p.shape) * s), 0, 1023).astype(np.uint16) for p, s in zip(clean, sig)]
    return [p.astype(np.uint16) for p in clean], noisy


def test_the_gain_from_the_clips_own_levels_helps_where_the_definition_says():
    """Pooled h from N7, with and without the gain of rule 23 (R = 4, Nmin = 200), A = 3, S = 2, the reference alone.

    Measured on this content (seed 7): residual chroma noise (rms error away from the edge) in the grainy half
    0.919 with the gain over without; mean absolute error in the four rows across the weak edge in the quiet half
    0.758 with the gain over without.  Only the direction is asserted: nobody has derived a magnitude."""
    from grav1synth_amd.denoise import weight_table

    bd = 10
    clean, noisy = two_halves()
    rec = NR.nlf_frame(noisy, bd, 1, 1)
    h = NR.strength(rec, bd, 200, 1)
    assert h is not None
    gain = G.gain_from_s(G.chroma_sigma(rec, 200), 4)
    assert int(gain[200]) < 256 < int(gain[50]), "bright luma, more grain: a smaller multiplier of the distance, a larger strength"
    T, q = weight_table(bd, 2, h, joint_chroma=True)
    out = {name: G.denoise_chroma_clip([noisy], 1, 1, 0, 3, 2, T, q, g, bd)[0] for name, g in (("flat", G.FLAT), ("gain", gain))}
    away = np.r_[4:18, 30:44]

    def noise(o):
        return float(np.sqrt(np.mean([(o[c][away, 36:60].astype(float) - clean[c + 1][away, 36:60]) ** 2 for c in (0, 1)])))

    def edge(o):
        return float(np.mean([np.abs(o[c][22:26, 4:28].astype(float) - clean[c + 1][22:26, 4:28]) for c in (0, 1)]))

    rn, re_ = noise(out["gain"]) / noise(out["flat"]), edge(out["gain"]) / edge(out["flat"])
    print(f"h_chroma {h:.3f}; grainy half, residual noise: gain / flat = {rn:.3f}; quiet half, error across the edge: gain / flat = {re_:.3f}")
    assert rn < 1.0, "residual chroma noise in the grainy half is lower with the gain"
    assert re_ < 1.0, "error across the weak edge in the quiet half is lower with the gain"
