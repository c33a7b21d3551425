"""Luma-guided joint chroma (`denoise`, rules 8 - 11t) without a device: the numpy restatement against the rules written out,
the table of rule 10, the joint tiles of denoise_tile.hip.h (dn_tile_j and dn_tile_jt as they stand) run on a host workgroup,
what the filter is for, the refusals and the commands' wiring."""
from __future__ import annotations

import ctypes as C
import inspect

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import denoise_joint_ref as J
from tests import denoise_ref as R
from tests import denoise_temporal_ref as TR
from tests import denoise_wg as WG

SUB = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}


def clip(n, w, h, bd, xdec, ydec, seed=0, amp=5, full_range=False):
    """n frames [Y, Cb, Cr] of luma size w x h: moving gradients, different on every plane, fresh noise on each."""
    top = (1 << bd) - 1
    cw, ch = (w + xdec) >> xdec, (h + ydec) >> ydec
    out = []
    for t in range(n):
        rng = np.random.default_rng([seed, t, w, h, bd])
        planes = []
        for c, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch))):
            if full_range:
                planes.append(rng.integers(0, top + 1, (ph, pw)).astype(np.uint8 if bd == 8 else np.uint16))
                continue
            base = ((np.arange(pw)[None, :] + 2 * t) * (5 - c) + (np.arange(ph)[:, None] + t * t) * (3 + c)) * (1 << (bd - 8))
            p = np.clip(base % (top + 1) + rng.integers(-(amp << (bd - 8)), (amp << (bd - 8)) + 1, (ph, pw)), 0, top)
            planes.append(p.astype(np.uint8 if bd == 8 else np.uint16))
        out.append(planes)
    return out


def direct(frames, t, xdec, ydec, D, A, S, T, q):
    """Rules 8 - 11t as they are written: loops over samples, frames, offsets, planes and patch terms."""
    def guide(y):
        H, W = y.shape
        cw, ch = (W + xdec) >> xdec, (H + ydec) >> ydec
        g = np.zeros((ch, cw), np.int64)
        for yy in range(ch):
            for xx in range(cw):
                s = sum(int(y[min((yy << ydec) + j, H - 1), min((xx << xdec) + i, W - 1)]) for j in range(ydec + 1) for i in range(xdec + 1))
                g[yy, xx] = (s + ((1 << (xdec + ydec)) >> 1)) >> (xdec + ydec)
        return g

    def triple(f):
        return [np.asarray(f[1]).astype(np.int64), np.asarray(f[2]).astype(np.int64), guide(np.asarray(f[0]))]

    us = triple(frames[t])
    h, w = us[0].shape
    at = lambda p, x, y: int(p[min(max(y, 0), h - 1), min(max(x, 0), w - 1)])
    outs = [np.zeros_like(frames[t][1]), np.zeros_like(frames[t][2])]
    for y in range(h):
        for x in range(w):
            nb = nr = den = 0
            for k in range(-D, D + 1):
                if not 0 <= t + k < len(frames):
                    continue
                vs = triple(frames[t + k])
                for dy in range(-A, A + 1):
                    for dx in range(-A, A + 1):
                        if not (0 <= x + dx < w and 0 <= y + dy < h):
                            continue
                        DJ = sum((at(u, x + kx, y + ky) - at(v, x + dx + kx, y + dy + ky)) ** 2
                                 for u, v in zip(us, vs) for ky in range(-S, S + 1) for kx in range(-S, S + 1))
                        wgt = int(T[min(DJ >> q, 1023)])
                        nb += wgt * int(vs[0][y + dy, x + dx])
                        nr += wgt * int(vs[1][y + dy, x + dx])
                        den += wgt
            outs[0][y, x] = (nb + (den >> 1)) // den
            outs[1][y, x] = (nr + (den >> 1)) // den
    return outs


@pytest.mark.parametrize("ss", ["420", "422", "444"])
@pytest.mark.parametrize("bd,w,h,n,D,A,S,strength", [(8, 5, 3, 1, 0, 2, 1, 6.0), (10, 9, 5, 1, 0, 3, 2, 9.0), (12, 5, 3, 3, 1, 2, 1, 30.0),
                                                     (8, 9, 5, 3, 2, 1, 2, 8.0)])
def test_the_vectorised_reference_equals_the_rules_written_out(ss, bd, w, h, n, D, A, S, strength):
    xdec, ydec = SUB[ss]
    T, q = J.joint_table_from_formula(bd, S, strength)
    frames = clip(n, w, h, bd, xdec, ydec, seed=3)
    got = J.denoise_chroma_clip(frames, xdec, ydec, D, A, S, T, q)
    for t in range(n):
        want = direct(frames, t, xdec, ydec, D, A, S, T, q)
        assert np.array_equal(got[t][0], want[0]) and np.array_equal(got[t][1], want[1]), t
    # luma is not the joint filter's business, and a luma-only clip is filtered as without the flag
    tl = R.table_from_formula(bd, S, strength)
    full = J.denoise_clip(frames, xdec, ydec, D, A, S, tl, (T, q))
    ys = TR.denoise_plane_clip([f[0] for f in frames], D, A, S, *tl)
    assert all(np.array_equal(f[0], y) for f, y in zip(full, ys))
    mono = J.denoise_clip([f[:1] for f in frames], xdec, ydec, D, A, S, tl, (T, q))
    assert all(len(f) == 1 and np.array_equal(f[0], y) for f, y in zip(mono, ys))


def test_the_guide_clamps_in_luma_coordinates_and_is_luma_at_444():
    y = np.arange(15, dtype=np.uint16).reshape(3, 5) * 7
    assert np.array_equal(J.guide(y, 0, 0), y)
    g = J.guide(y, 1, 1)
    assert g.shape == (2, 3)
    assert g[0, 0] == (0 + 7 + 35 + 42 + 2) >> 2
    assert g[0, 2] == (28 + 28 + 63 + 63 + 2) >> 2, "the column past the plane repeats the last one"
    assert g[1, 2] == 98, "the corner: four times the last sample"
    g = J.guide(y, 1, 0)
    assert g.shape == (3, 3) and g[2, 2] == 98 and g[1, 0] == (35 + 42 + 1) >> 1


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_the_joint_table_is_rule_3_with_3n(bd, S):
    from grav1synth_amd.denoise import weight_table

    n3 = 3 * (2 * S + 1) ** 2
    for h in (0.001, 0.05, 0.7, 4.0, 12.5, 100.0, 1000.0):
        T, q = weight_table(bd, S, h, joint_chroma=True)
        assert T.dtype == np.uint16 and T.shape == (1024,) and T[0] == 4096 and T[1023] == 0
        assert np.all(np.diff(T.astype(np.int64)) <= 0), "non-increasing"
        entry = lambda i, qq: 4096.0 * np.exp(-min(((i + 0.5) * 2.0 ** qq) / (n3 * h * h * 4.0 ** (bd - 8)), 700.0))
        assert np.abs(T.astype(np.float64) - np.array([4096.0] + [entry(i, q) for i in range(1, 1024)])).max() <= 1.0, (bd, S, h)
        assert q == 0 or entry(1023, q - 1) >= 0.5, "q is minimal"
        ft, fq = J.joint_table_from_formula(bd, S, h)
        assert fq == q and np.abs(ft.astype(np.int64) - T.astype(np.int64)).max() <= 1
        # without the flag: rule 3's table, through either entry point
        T0, q0 = weight_table(bd, S, h)
        T1, q1 = weight_table(bd, S, h, joint_chroma=False)
        old = np.zeros(1024, np.uint16)
        qo = C.c_uint32()
        assert _lib.lib().g1s_denoise_weights(bd, S, h, old.ctypes.data, C.byref(qo)) == 0
        assert q0 == q1 == qo.value and np.array_equal(T0, T1) and np.array_equal(T0, old)
        assert h < 0.5 or not np.array_equal(T, T0) or q != q0, "three times the patch: another table"


def test_refusals_of_the_table_and_the_constructor_need_no_device():
    from grav1synth_amd.denoise import Denoiser, denoise_opts, weight_table

    L = _lib.lib()
    for name in ("g1s_denoise_new_ex", "g1s_denoise_weights_ex", "g1s_denoise_y4m_file_ex", "g1s_diff_y4m_file_denoised_ex"):
        assert hasattr(L, name) and name in [s[0] for s in _lib.SYMBOLS]
    assert _lib.G1S_DENOISE_JOINT_CHROMA == 1
    for args, text in (((9, 2, 4.0), "8, 10 and 12"), ((8, 0, 4.0), "patch_radius"), ((8, 5, 4.0), "patch_radius"), ((8, 2, 0.0), "strength"),
                       ((8, 2, 1001.0), "strength"), ((8, 2, float("nan")), "strength")):
        with pytest.raises(_lib.G1SError) as e:
            weight_table(*args, joint_chroma=True)
        assert text in str(e.value), args
    T = np.zeros(1024, np.uint16)
    q = C.c_uint32()
    for flags in (2, 3, 0x80000000):
        assert L.g1s_denoise_weights_ex(8, 2, 4.0, flags, T.ctypes.data, C.byref(q)) == -1 and b"unknown denoise flags" in L.g1s_last_global_error()
        assert not L.g1s_denoise_new_ex(10, C.byref(denoise_opts()), 0, flags) and b"unknown denoise flags" in L.g1s_last_global_error()
        assert not L.g1s_denoise_new_ex(10, None, 1, flags) and b"unknown denoise flags" in L.g1s_last_global_error()
    assert L.g1s_denoise_weights_ex(8, 2, 4.0, 1, None, C.byref(q)) == -1
    # the other refusals hold under the flag, and come first where they did
    o = denoise_opts()
    assert not L.g1s_denoise_new_ex(10, C.byref(o), 4, 1) and b"temporal_radius must be 0..3" in L.g1s_last_global_error()
    assert not L.g1s_denoise_new_ex(10, C.byref(denoise_opts(search_radius=8)), 0, 1) and b"search_radius" in L.g1s_last_global_error()
    assert not L.g1s_denoise_new_ex(9, C.byref(o), 0, 1) and b"8, 10 and 12" in L.g1s_last_global_error()
    assert not L.g1s_denoise_new_ex(12, C.byref(denoise_opts(chroma_strength=-1.0)), 0, 1) and b"chroma_strength" in L.g1s_last_global_error()
    # the struct has not grown to carry the flag
    assert C.sizeof(_lib.G1SDenoiseOpts) == 40
    o.struct_size = 44
    assert not L.g1s_denoise_new_ex(8, C.byref(o), 0, 1) and b"struct_size" in L.g1s_last_global_error()
    err = C.create_string_buffer(256)
    assert L.g1s_diff_y4m_file_denoised_ex(b"/nonexistent.y4m", b"/nonexistent.tbl", None, None, None, 0, 4, None, err, len(err)) == -1
    assert b"unknown denoise flags" in err.value
    with pytest.raises(_lib.G1SError) as e:
        Denoiser(10, temporal_radius=4, joint_chroma=True)
    assert "temporal_radius must be 0..3" in str(e.value)


# ---------------------------------------------------------------------------------------------- the tile on the host
@pytest.fixture(scope="module")
def tile_host(tmp_path_factory):
    if WG.compiler() is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("jtile") / "denoise_wg_host"
    WG.build(exe)

    def run(frames, present, xdec, ydec, A, S, T, q):
        """The frame frames[0] and its neighbours frames[1:] (present[k]: takes part) through every tile: (out_Cb, out_Cr)."""
        kind = "tile_jt" if len(frames) > 1 else "tile_j"
        out = WG.run_tiles(exe, kind, frames, present, xdec, ydec, A, S, T, q)
        out = np.frombuffer(out, frames[0][1].dtype).reshape((2,) + frames[0][1].shape)
        return out[0], out[1]

    return run


def neighbours(frames, t, D):
    """(frame, the 2 D frames around it in the kernel's order, which of them the clip has)"""
    ks = [k for k in range(-D, D + 1) if k]
    present = [0 <= t + k < len(frames) for k in ks]
    return [frames[t]] + [frames[t + k] if ok else [np.zeros_like(p) for p in frames[t]] for k, ok in zip(ks, present)], present


TILE_CASES = [
    # bd, ss, luma w, luma h, frames, t, D, A, S, strength
    (8, "420", 128, 96, 1, 0, 0, 3, 2, 6.0),       # one chroma tile, spatial
    (10, "420", 383, 287, 1, 0, 0, 3, 2, 6.0),     # chroma 192 x 144: an interior tile and every edge; odd luma, the guide clamps
    (10, "420", 259, 195, 3, 1, 1, 2, 1, 8.0),     # chroma 130 x 98: tiles off the plane's size, both neighbours
    (12, "422", 129, 49, 1, 0, 0, 3, 3, 9.0),      # chroma 65 x 49
    (8, "444", 65, 49, 3, 0, 1, 2, 2, 8.0),        # G = Y; the first frame of a clip: nothing before it
    (12, "420", 140, 100, 3, 2, 1, 3, 3, 9.0),     # the last: nothing after it
    (10, "420", 9, 5, 5, 2, 2, 3, 2, 6.0),         # planes smaller than the window
    (8, "420", 1, 1, 3, 1, 1, 7, 4, 4.0),
    (12, "422", 3, 60, 1, 0, 0, 7, 1, 30.0),
    (8, "420", 5, 3, 1, 0, 0, 7, 4, 12.0),
    (12, "444", 66, 20, 2, 1, 3, 7, 4, 1000.0),    # a two-frame clip at D = 3, the largest tile
]


@pytest.mark.parametrize("bd,ss,w,h,n,t,D,A,S,strength", TILE_CASES)
def test_the_joint_tile_on_the_host_equals_the_reference(tile_host, bd, ss, w, h, n, t, D, A, S, strength):
    xdec, ydec = SUB[ss]
    T, q = J.joint_table_from_formula(bd, S, strength)
    frames = clip(n, w, h, bd, xdec, ydec, seed=w + h)
    args, present = neighbours(frames, t, D)
    got = tile_host(args, present, xdec, ydec, A, S, T, q)
    want = J.denoise_chroma_clip(frames, xdec, ydec, D, A, S, T, q)[t]
    for c in (0, 1):
        assert np.array_equal(got[c], want[c]), (c, np.argwhere(got[c] != want[c])[:5])
    ind = R.denoise_plane(frames[t][1], A, S, T, q)
    assert (got[0] != ind).any() or frames[t][1].size < 4, "the other planes did something"


def ceiling_frame(w, h, xdec, ydec):
    """12 bit: Cb, Cr and luma 0 / 4095 checkerboards, luma in cells of 2^xdec x 2^ydec, so the guide is a checkerboard too."""
    cw, ch = (w + xdec) >> xdec, (h + ydec) >> ydec
    chk = (((np.arange(ch)[:, None] + np.arange(cw)[None, :]) & 1) * 4095).astype(np.uint16)
    y = np.repeat(np.repeat(chk, 1 << ydec, 0), 1 << xdec, 1)[:h, :w]
    return [np.ascontiguousarray(y), chk.copy(), chk.copy()]


@pytest.mark.parametrize("strength", [1000.0, 4.0])
def test_the_tile_on_the_host_at_the_32_bit_ceiling(tile_host, strength):
    A, S = 3, 4
    frame = ceiling_frame(150, 110, 1, 1)
    assert J.max_distance(frame, 1, 1, A, S) == 4074873075 > 2 ** 31
    T, q = J.joint_table_from_formula(12, S, strength)
    if strength == 1000.0:  # the ceiling's own entry is neither end of the table: a sum read as signed lands on another one
        assert 0 < 4074873075 >> q < 1023 and 0 < T[4074873075 >> q] < 4096
    want = J.denoise_chroma_clip([frame], 1, 1, 0, A, S, T, q)[0]
    got = tile_host([frame], [], 1, 1, A, S, T, q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # and through the temporal kernel: the same checkerboard one sample on, so the ZERO offset is at the ceiling
    other = [np.ascontiguousarray(4095 - p) for p in frame]
    clip3 = [other, frame, other]
    want = J.denoise_chroma_clip(clip3, 1, 1, 1, A, S, T, q)[1]
    args, present = neighbours(clip3, 1, 1)
    got = tile_host(args, present, 1, 1, A, S, T, q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_the_tile_on_the_host_in_64_bits_and_without_neighbours(tile_host):
    T, q = J.joint_table_from_formula(12, 1, 1000.0)
    wild = clip(3, 70, 30, 12, 0, 0, seed=4, full_range=True)
    for f in wild:
        f[1][5:25, 5:60] = 4095 - (f[1][5:25, 5:60] & 3)
    nb, _nr, den = J.chroma_sums(wild, 1, 0, 0, 1, 7, 1, T, q)
    assert nb.max() >= 2 ** 32 and den.max() < 2 ** 32
    args, present = neighbours(wild, 1, 1)
    got = tile_host(args, present, 0, 0, 7, 1, T, q)
    want = J.denoise_chroma_clip(wild, 0, 0, 1, 7, 1, T, q)[1]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # no neighbour takes part: the spatial joint filter, through the 64-bit store
    got = tile_host(args, [False, False], 0, 0, 7, 1, T, q)
    want = J.denoise_chroma_clip(wild[1:2], 0, 0, 0, 7, 1, T, q)[0]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------------ what it is for
def test_a_weak_chroma_edge_under_grain_survives_the_joint_filter():
    """Seed 5, 10-bit 4:2:0, luma cells at 300 / 700, co-located chroma cells 60 apart, grain of sigma 16 on every plane,
    A = 3, S = 2, h = 8: the joint filter's mean squared error against the clean chroma is below half the independent
    filter's, on Cb and on Cr."""
    clean, noisy = J.edge_content(seed=5, step=60, sigma=16.0)
    assert noisy[0].shape == (96, 128) and noisy[1].shape == noisy[2].shape == (48, 64)
    tc, tj = R.table_from_formula(10, 2, 8.0), J.joint_table_from_formula(10, 2, 8.0)
    ind = R.denoise_frame(noisy, 3, 2, tc, tc)
    joint = J.denoise_frame(noisy, 1, 1, 3, 2, tc, tj)
    mse = lambda a, b: float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).mean())
    for c in (1, 2):
        e_ind, e_joint = mse(ind[c], clean[c]), mse(joint[c], clean[c])
        print(f"plane {c}: independent {e_ind:.1f}, joint {e_joint:.1f}, ratio {e_joint / e_ind:.3f}")
        assert e_joint < 0.5 * e_ind, (c, e_ind, e_joint)
    assert np.array_equal(joint[0], ind[0]), "luma is filtered as without the flag"


# ------------------------------------------------------------------------------------------------------ the commands
def test_commands_under_the_flag_refuse_with_one_logged_line(tmp_path, caplog):
    from grav1synth_amd import cli

    src = tmp_path / "a.y4m"
    src.write_bytes(b"x")
    den = tmp_path / "d.y4m"
    den.write_bytes(b"y")
    out, tbl = tmp_path / "o.y4m", tmp_path / "t.tbl"

    def one_line(text, call):
        caplog.clear()
        with caplog.at_level("INFO", logger="grav1synth"):
            assert call() == -1
        assert [r.getMessage() for r in caplog.records] == [text]

    one_line(cli.BAD_TEMPORAL_RADIUS, lambda: cli.denoise_command(str(src), str(out), temporal_radius=4, joint_chroma=True))
    one_line(cli.SAME_AS_OUTPUT, lambda: cli.denoise_command(str(src), str(src), joint_chroma=True))
    one_line(cli.BAD_TEMPORAL_RADIUS, lambda: cli.diff_command(str(src), None, str(tbl), denoise=True, temporal_radius=-1, joint_chroma=True))
    one_line(cli.BOTH_DENOISED, lambda: cli.diff_command(str(src), str(den), str(tbl), denoise=True, joint_chroma=True))
    one_line(cli.SAME_AS_OUTPUT, lambda: cli.diff_command(str(src), None, str(src), denoise=True, joint_chroma=True))
    assert not out.exists() and not tbl.exists()
    # without --denoise the flag is carried and not used, as --temporal-radius is: the two-file command's own refusals
    assert cli.main(["diff", str(src), str(src), "--joint-chroma", "-o", str(tbl)]) == 0 and not tbl.exists()
    assert cli.main(["diff", str(src), "--joint-chroma", "-o", str(tbl)]) == 0 and not tbl.exists()


def test_argument_wiring(monkeypatch, tmp_path):
    from grav1synth_amd import cli, denoise, ingest

    p = cli.build_parser()
    a = p.parse_args(["denoise", "in.y4m", "-o", "out.y4m", "--joint-chroma", "--temporal-radius", "2"])
    assert a.joint_chroma is True and cli._denoise_parameters(a)["joint_chroma"] is True and cli._denoise_parameters(a)["temporal_radius"] == 2
    a = p.parse_args(["diff", "s.y4m", "--denoise", "-o", "t.tbl", "--joint-chroma"])
    assert a.joint_chroma is True and a.denoise
    assert p.parse_args(["denoise", "in.y4m", "-o", "out.y4m"]).joint_chroma is False
    assert p.parse_args(["diff", "s.y4m", "d.y4m", "-o", "t.tbl"]).joint_chroma is False
    for f in (denoise.Denoiser.__init__, denoise.denoise_y4m_file, denoise.weight_table, ingest.diff_y4m_file_denoised):
        assert inspect.signature(f).parameters["joint_chroma"].default is False
    seen = {}
    monkeypatch.setattr(denoise, "denoise_y4m_file", lambda i, o, **kw: seen.update(denoise=kw) or 3)
    monkeypatch.setattr(ingest, "diff_y4m_file_denoised", lambda s, o, **kw: seen.update(diff=kw) or 3)
    src = tmp_path / "a.y4m"
    src.write_bytes(b"x")
    assert cli.main(["denoise", str(src), "-o", str(tmp_path / "o.y4m"), "--joint-chroma", "--chroma-strength", "8"]) == 0
    assert seen["denoise"]["joint_chroma"] is True and seen["denoise"]["chroma_strength"] == 8.0 and seen["denoise"]["temporal_radius"] == 0
    assert cli.main(["denoise", str(src), "-o", str(tmp_path / "o2.y4m")]) == 0 and seen["denoise"]["joint_chroma"] is False
    assert cli.main(["diff", str(src), "--denoise", "-o", str(tmp_path / "t.tbl"), "--joint-chroma", "--temporal-radius", "1"]) == 0
    assert seen["diff"]["joint_chroma"] is True and seen["diff"]["temporal_radius"] == 1
