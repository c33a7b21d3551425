"""The temporal radius of `denoise` without a device: the numpy restatement of rules 5 - 7 against the rules written out,
its properties, the temporal tile of denoise_tile.hip.h (dn_tile_t as it stands) run on a host workgroup, the refusals and
the commands' wiring."""
from __future__ import annotations

import ctypes as C
import inspect

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import denoise_ref as R
from tests import denoise_temporal_ref as TR
from tests import denoise_wg as WG
from tests.test_denoise_cpu import plane


def clip(n, w, h, bd, seed=0, shift=(2, 1)):
    """n planes of the gradient of test_denoise_cpu.plane moving by `shift` a frame, fresh noise on each."""
    top = (1 << bd) - 1
    out = []
    for t in range(n):
        rng = np.random.default_rng([seed, t, w, h, bd])
        base = ((np.arange(w)[None, :] + shift[0] * t) * 5 + (np.arange(h)[:, None] + shift[1] * t * t) * 3) * (1 << (bd - 8))
        p = np.clip(base % (top + 1) + rng.integers(-(5 << (bd - 8)), (5 << (bd - 8)) + 1, (h, w)), 0, top)
        out.append(p.astype(np.uint8 if bd == 8 else np.uint16))
    return out


def direct(planes, t, D, A, S, T, q):
    """Rules 1 - 7 as they are written: a loop over samples, frames, offsets and patch terms."""
    u = planes[t].astype(np.int64)
    h, w = u.shape
    out = np.zeros_like(planes[t])
    for y in range(h):
        for x in range(w):
            num = den = 0
            for k in range(-D, D + 1):
                if not 0 <= t + k < len(planes):
                    continue
                v = planes[t + k].astype(np.int64)
                cu = lambda xx, yy: u[min(max(yy, 0), h - 1), min(max(xx, 0), w - 1)]
                cv = lambda xx, yy: v[min(max(yy, 0), h - 1), min(max(xx, 0), w - 1)]
                for dy in range(-A, A + 1):
                    for dx in range(-A, A + 1):
                        if not (0 <= x + dx < w and 0 <= y + dy < h):
                            continue
                        Dk = sum((cu(x + kx, y + ky) - cv(x + dx + kx, y + dy + ky)) ** 2 for ky in range(-S, S + 1) for kx in range(-S, S + 1))
                        assert k != 0 or dx != 0 or dy != 0 or Dk == 0
                        wgt = int(T[min(Dk >> q, 1023)])
                        num += wgt * int(v[y + dy, x + dx])
                        den += wgt
            out[y, x] = (num + (den >> 1)) // den
    return out


@pytest.mark.parametrize("bd,w,h,n,D,A,S,strength", [(8, 5, 3, 3, 1, 2, 1, 6.0), (12, 3, 5, 4, 2, 2, 1, 9.0), (8, 6, 4, 5, 3, 1, 2, 30.0),
                                                     (12, 1, 1, 3, 1, 2, 1, 4.0), (10, 7, 2, 2, 3, 3, 1, 8.0)])
def test_the_vectorised_reference_equals_the_rules_written_out(bd, w, h, n, D, A, S, strength):
    T, q = R.table_from_formula(bd, S, strength)
    planes = clip(n, w, h, bd, seed=3)
    got = TR.denoise_plane_clip(planes, D, A, S, T, q)
    for t in range(n):
        assert np.array_equal(got[t], direct(planes, t, D, A, S, T, q)), t


def test_radius_0_and_a_one_frame_clip_are_the_spatial_filter():
    for bd in (8, 12):
        T, q = R.table_from_formula(bd, 2, 6.0)
        planes = clip(3, 37, 23, bd, seed=1)
        want = [R.denoise_plane(p, 3, 2, T, q) for p in planes]
        got = TR.denoise_plane_clip(planes, 0, 3, 2, T, q)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        for D in (1, 2, 3):
            assert np.array_equal(TR.denoise_plane_clip(planes[:1], D, 3, 2, T, q)[0], want[0])
    frames = [[p, p[::2, ::2].copy(), p[1::2, 1::2].copy()] for p in clip(2, 20, 12, 8)]
    tl, tc = R.table_from_formula(8, 2, 6.0), R.table_from_formula(8, 2, 3.0)
    assert all(np.array_equal(a, b) for f, g in zip(TR.denoise_clip(frames, 0, 3, 2, tl, tc), [R.denoise_frame(f, 3, 2, tl, tc) for f in frames])
               for a, b in zip(f, g))


def test_properties_of_the_temporal_filter():
    for bd in (8, 12):
        T, q = R.table_from_formula(bd, 2, 6.0)
        top = (1 << bd) - 1
        dt = np.uint8 if bd == 8 else np.uint16
        for value in (0, 77 << (bd - 8), top):  # a constant clip stays constant
            c = [np.full((15, 19), value, dt)] * 4
            assert all(np.array_equal(o, c[0]) for o in TR.denoise_plane_clip(c, 2, 3, 2, T, q))
        planes = clip(5, 31, 22, bd, seed=2)
        out = TR.denoise_plane_clip(planes, 2, 3, 2, T, q)
        back = TR.denoise_plane_clip(planes[::-1], 2, 3, 2, T, q)  # time has no direction
        assert all(np.array_equal(a, b) for a, b in zip(back[::-1], out))
        assert any((a != b).any() for a, b in zip(out, TR.denoise_plane_clip(planes, 1, 3, 2, T, q)))
    # the point of the feature: a static picture with independent noise comes out closer to the clean one
    rng = np.random.default_rng(5)
    clean = ((np.arange(48)[None, :] * 3 + np.arange(40)[:, None] * 2) % 200 + 20).astype(np.int64)
    clean[10:30, 12:20] += 25
    noisy = [np.clip(clean + np.rint(rng.normal(0, 4.0, clean.shape)), 0, 255).astype(np.uint8) for _ in range(5)]
    T, q = R.table_from_formula(8, 2, 4.0)
    mse = lambda p: float(((p.astype(np.int64) - clean) ** 2).mean())
    e0 = mse(TR.denoise_plane_clip(noisy, 0, 3, 2, T, q)[2])
    e2 = mse(TR.denoise_plane_clip(noisy, 2, 3, 2, T, q)[2])
    assert e2 < 0.8 * e0 < 0.8 * mse(noisy[2]), (e0, e2)


def test_a_numerator_beyond_32_bits():
    T, q = R.table_from_formula(12, 1, 1000.0)
    full = [np.full((16, 16), 4095, np.uint16)] * 3
    num, den = TR.sums_plane(full, 1, 1, 7, 1, T, q)
    assert num.max() >= 2 ** 32 and den.max() == 3 * 225 * 4096 < 2 ** 32
    assert all(np.array_equal(o, full[0]) for o in TR.denoise_plane_clip(full, 1, 7, 1, T, q))
    rng = np.random.default_rng(9)
    wild = [rng.integers(3500, 4096, (16, 16)).astype(np.uint16) for _ in range(3)]
    assert TR.sums_plane(wild, 1, 1, 7, 1, T, q)[0].max() >= 2 ** 32
    assert np.array_equal(TR.denoise_plane_clip(wild, 1, 7, 1, T, q)[1], direct(wild, 1, 1, 7, 1, T, q))


def test_the_new_symbols_and_the_refusal_of_a_radius_of_4_need_no_device():
    from grav1synth_amd.denoise import denoise_opts

    L = _lib.lib()
    for name in ("g1s_denoise_new_temporal", "g1s_denoise_drain", "g1s_denoise_y4m_file_temporal", "g1s_diff_y4m_file_denoised_temporal"):
        assert hasattr(L, name) and name in [s[0] for s in _lib.SYMBOLS]
    o = denoise_opts()
    for radius in (4, 7, 0xFFFFFFFF):
        assert not L.g1s_denoise_new_temporal(10, C.byref(o), radius)
        assert b"temporal_radius must be 0..3" in L.g1s_last_global_error()
    assert not L.g1s_denoise_new_temporal(10, C.byref(denoise_opts(search_radius=8)), 1) and b"search_radius" in L.g1s_last_global_error()
    assert not L.g1s_denoise_new_temporal(9, C.byref(o), 1) and b"8, 10 and 12" in L.g1s_last_global_error()
    # the struct has not grown to carry the radius
    assert C.sizeof(_lib.G1SDenoiseOpts) == 40
    o.struct_size = 44
    assert not L.g1s_denoise_new(8, C.byref(o)) and b"struct_size" in L.g1s_last_global_error()
    assert not L.g1s_denoise_new_temporal(8, C.byref(o), 1) and b"struct_size" in L.g1s_last_global_error()
    assert L.g1s_denoise_drain(None, None) < 0


def test_python_refuses_a_radius_of_4_without_a_device():
    from grav1synth_amd.denoise import Denoiser

    with pytest.raises(_lib.G1SError) as e:
        Denoiser(10, temporal_radius=4)
    assert "temporal_radius must be 0..3" in str(e.value)


# ---------------------------------------------------------------------------------------------- the tile on the host
@pytest.fixture(scope="module")
def tile_host(tmp_path_factory):
    if WG.compiler() is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("tile") / "denoise_wg_host"
    WG.build(exe)

    def run(planes, present, A, S, T, q):
        """The frame planes[0] and its neighbours planes[1:] (present[k]: takes part) through every tile of the plane."""
        kind = "tile_t" if len(planes) > 1 else "tile"
        out = WG.run_tiles(exe, kind, [[p] for p in planes], present, 0, 0, A, S, T, q)
        return np.frombuffer(out, planes[0].dtype).reshape(planes[0].shape)

    return run


def neighbours(planes, t, D):
    """(frame, the 2 D planes around it in the kernel's order, which of them the clip has)"""
    ks = [k for k in range(-D, D + 1) if k]
    present = [0 <= t + k < len(planes) for k in ks]
    return [planes[t]] + [planes[t + k] if ok else np.zeros_like(planes[t]) for k, ok in zip(ks, present)], present


TILE_CASES = [
    # bd, w, h, frames, t, D, A, S, strength
    (8, 64, 48, 3, 1, 1, 3, 2, 6.0),      # one tile, both neighbours
    (10, 150, 110, 3, 1, 1, 3, 2, 6.0),   # interior tile and every edge, tiles off the plane's size
    (8, 65, 49, 4, 0, 2, 2, 1, 8.0),      # the first frame of a clip: nothing before it
    (12, 70, 50, 4, 3, 2, 3, 3, 9.0),     # the last: nothing after it
    (10, 5, 3, 5, 2, 2, 3, 2, 6.0),       # planes smaller than the window
    (8, 1, 1, 3, 1, 1, 7, 4, 4.0),
    (12, 2, 60, 3, 1, 1, 7, 1, 30.0),
    (8, 90, 9, 7, 3, 3, 4, 4, 12.0),      # D = 3, all six neighbours
    (12, 66, 20, 2, 1, 3, 7, 4, 1000.0),  # a two-frame clip at D = 3
]


@pytest.mark.parametrize("bd,w,h,n,t,D,A,S,strength", TILE_CASES)
def test_the_temporal_tile_on_the_host_equals_the_reference(tile_host, bd, w, h, n, t, D, A, S, strength):
    T, q = R.table_from_formula(bd, S, strength)
    planes = clip(n, w, h, bd, seed=w + h)
    args, present = neighbours(planes, t, D)
    got = tile_host(args, present, A, S, T, q)
    want = TR.denoise_plane_clip(planes, D, A, S, T, q)[t]
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (got != R.denoise_plane(planes[t], A, S, T, q)).any() or w * h < 4


def test_the_tile_on_the_host_in_64_bits_and_without_neighbours(tile_host):
    T, q = R.table_from_formula(12, 1, 1000.0)
    rng = np.random.default_rng(4)
    wild = [rng.integers(0, 4096, (30, 70)).astype(np.uint16) for _ in range(3)]
    wild[1][5:25, 5:60] = 4095
    assert TR.sums_plane(wild, 1, 1, 7, 1, T, q)[0].max() >= 2 ** 32
    args, present = neighbours(wild, 1, 1)
    assert np.array_equal(tile_host(args, present, 7, 1, T, q), TR.denoise_plane_clip(wild, 1, 7, 1, T, q)[1])
    full = [np.full((50, 66), 4095, np.uint16)] * 7
    args, present = neighbours(full, 3, 3)
    assert np.array_equal(tile_host(args, present, 7, 1, T, q), full[0])
    # no neighbour takes part: the spatial filter, through the 64-bit store
    args, _ = neighbours(wild, 1, 1)
    assert np.array_equal(tile_host(args, [False, False], 7, 1, T, q), R.denoise_plane(wild[1], 7, 1, T, q))


# ------------------------------------------------------------------------------------------------------ the commands
def test_commands_refuse_a_radius_outside_0_to_3_with_one_logged_line(tmp_path, caplog):
    from grav1synth_amd import cli

    src = tmp_path / "a.y4m"
    src.write_bytes(b"x")
    out, tbl = tmp_path / "o.y4m", tmp_path / "t.tbl"
    for call in (lambda r: cli.denoise_command(str(src), str(out), temporal_radius=r),
                 lambda r: cli.diff_command(str(src), None, str(tbl), denoise=True, temporal_radius=r)):
        for radius in (4, -1):
            caplog.clear()
            with caplog.at_level("INFO", logger="grav1synth"):
                assert call(radius) == -1
            assert [r.getMessage() for r in caplog.records] == [cli.BAD_TEMPORAL_RADIUS]
    assert not out.exists() and not tbl.exists()
    assert cli.main(["denoise", str(src), "-o", str(out), "--temporal-radius", "4"]) == 0 and not out.exists()
    assert cli.main(["diff", str(src), "--denoise", "-o", str(tbl), "--temporal-radius", "5"]) == 0 and not tbl.exists()


def test_argument_wiring(monkeypatch, tmp_path):
    from grav1synth_amd import cli, denoise, ingest

    p = cli.build_parser()
    a = p.parse_args(["denoise", "in.y4m", "-o", "out.y4m", "--temporal-radius", "2", "--search-radius", "5"])
    assert (a.temporal_radius, a.search_radius) == (2, 5) and cli._denoise_parameters(a)["temporal_radius"] == 2
    a = p.parse_args(["diff", "s.y4m", "--denoise", "-o", "t.tbl", "--temporal-radius", "1"])
    assert a.temporal_radius == 1 and a.denoise
    assert p.parse_args(["denoise", "in.y4m", "-o", "out.y4m"]).temporal_radius == 0
    assert p.parse_args(["diff", "s.y4m", "d.y4m", "-o", "t.tbl"]).temporal_radius == 0
    # the library calls behind them take the radius as an argument of their own
    for f in (denoise.Denoiser.__init__, denoise.denoise_y4m_file, ingest.diff_y4m_file_denoised):
        assert inspect.signature(f).parameters["temporal_radius"].default == 0
    seen = {}
    monkeypatch.setattr(denoise, "denoise_y4m_file", lambda i, o, **kw: seen.update(denoise=kw) or 3)
    monkeypatch.setattr(ingest, "diff_y4m_file_denoised", lambda s, o, **kw: seen.update(diff=kw) or 3)
    src = tmp_path / "a.y4m"
    src.write_bytes(b"x")
    assert cli.main(["denoise", str(src), "-o", str(tmp_path / "o.y4m"), "--temporal-radius", "3", "--strength", "2"]) == 0
    assert seen["denoise"]["temporal_radius"] == 3 and seen["denoise"]["strength"] == 2.0
    assert cli.main(["diff", str(src), "--denoise", "-o", str(tmp_path / "t.tbl"), "--temporal-radius", "2", "--keep-denoised", str(tmp_path / "k.y4m")]) == 0
    assert seen["diff"]["temporal_radius"] == 2 and seen["diff"]["keep_denoised"] == str(tmp_path / "k.y4m")
