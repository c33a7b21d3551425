"""`denoise` without a device: the weight table the library exposes, the numpy restatement's own properties, the command
line's refusals and the parameter refusals of g1s_denoise_new."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import denoise_ref as R


def plane(w, h, bd, seed=0):
    """A gradient with noise on it, full dtype range allowed."""
    rng = np.random.default_rng([seed, w, h, bd])
    top = (1 << bd) - 1
    base = (np.arange(w)[None, :] * 5 + np.arange(h)[:, None] * 3) * (1 << (bd - 8))
    p = np.clip(base % (top + 1) + rng.integers(-(5 << (bd - 8)), (5 << (bd - 8)) + 1, (h, w)), 0, top)
    return p.astype(np.uint8 if bd == 8 else np.uint16)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_the_exposed_weight_table_is_rule_3(bd, S):
    from grav1synth_amd.denoise import weight_table

    for h in (0.001, 0.05, 0.7, 4.0, 12.5, 100.0, 1000.0):
        T, q = weight_table(bd, S, h)
        assert T.dtype == np.uint16 and T.shape == (1024,)
        assert T[0] == 4096 and T[1023] == 0
        assert np.all(np.diff(T.astype(np.int64)) <= 0), "non-increasing"
        want = np.array([4096.0] + [R.table_entry(i, q, bd, S, h) for i in range(1, 1024)])
        assert np.abs(T.astype(np.float64) - want).max() <= 1.0, (bd, S, h)
        # q is minimal: one less and the last entry would not round to 0
        assert q == 0 or R.table_entry(1023, q - 1, bd, S, h) >= 0.5, (bd, S, h, q)
        assert R.table_entry(1023, q, bd, S, h) < 0.5 + 1e-9
        ft, fq = R.table_from_formula(bd, S, h)
        assert fq == q and np.abs(ft.astype(np.int64) - T.astype(np.int64)).max() <= 1


def test_table_refusals_and_a_q_of_zero():
    from grav1synth_amd.denoise import weight_table

    T, q = weight_table(8, 1, 0.01)
    assert q == 0 and T[1] == 0
    for args, text in (((9, 2, 4.0), "8, 10 and 12"), ((8, 0, 4.0), "patch_radius"), ((8, 5, 4.0), "patch_radius"),
                       ((8, 2, 0.0), "strength"), ((8, 2, -1.0), "strength"), ((8, 2, 1001.0), "strength"),
                       ((8, 2, float("nan")), "strength")):
        with pytest.raises(_lib.G1SError) as e:
            weight_table(*args)
        assert text in str(e.value), args


def test_parameter_refusals_of_the_constructor_need_no_device():
    from grav1synth_amd.denoise import denoise_opts

    L = _lib.lib()
    for bd, kw, text in ((9, {}, b"8, 10 and 12"), (16, {}, b"8, 10 and 12"), (8, dict(search_radius=8), b"search_radius must be 1..7"),
                         (8, dict(patch_radius=5), b"patch_radius must be 1..4"), (10, dict(strength=-2.0), b"strength"),
                         (10, dict(strength=2000.0), b"strength"), (12, dict(chroma_strength=-1.0), b"chroma_strength")):
        o = denoise_opts(**kw)
        assert not L.g1s_denoise_new(bd, C.byref(o)), (bd, kw)
        assert text in L.g1s_last_global_error(), (bd, kw, L.g1s_last_global_error())
    o = denoise_opts()
    o.struct_size += 4
    assert not L.g1s_denoise_new(8, C.byref(o)) and b"struct_size" in L.g1s_last_global_error()
    assert C.sizeof(_lib.G1SDenoiseOpts) == 40 and _lib.G1SDenoiseOpts.strength.offset == 24


def test_no_gpu_means_the_denoiser_refuses():
    import torch

    if torch.cuda.is_available():
        return  # (the device tests cover the other side)
    from grav1synth_amd.denoise import Denoiser

    with pytest.raises(_lib.G1SError) as e:
        Denoiser(10)
    assert "no CPU fallback" in str(e.value)


def direct(u, A, S, T, q):
    """Rules 1 - 4 as they are written: a loop over samples, offsets and patch terms."""
    h, w = u.shape
    v = u.astype(np.int64)
    out = np.zeros_like(u)
    cl = lambda x, y: v[min(max(y, 0), h - 1), min(max(x, 0), w - 1)]
    for y in range(h):
        for x in range(w):
            num = den = 0
            for dy in range(-A, A + 1):
                for dx in range(-A, A + 1):
                    if not (0 <= x + dx < w and 0 <= y + dy < h):
                        continue
                    D = sum((cl(x + kx, y + ky) - cl(x + dx + kx, y + dy + ky)) ** 2 for ky in range(-S, S + 1) for kx in range(-S, S + 1))
                    wgt = int(T[min(D >> q, 1023)])
                    num += wgt * int(v[y + dy, x + dx])
                    den += wgt
            assert den >= 4096 and num + (den >> 1) < 2 ** 32
            out[y, x] = (num + (den >> 1)) // den
    return out


@pytest.mark.parametrize("bd,w,h,A,S,strength", [(8, 5, 3, 3, 2, 6.0), (12, 3, 5, 3, 1, 9.0), (8, 7, 5, 4, 2, 30.0), (12, 9, 5, 5, 3, 4.0),
                                                 (8, 1, 1, 2, 1, 4.0), (12, 13, 11, 7, 4, 20.0)])
def test_the_vectorised_reference_equals_the_rules_written_out(bd, w, h, A, S, strength):
    T, q = R.table_from_formula(bd, S, strength)
    u = plane(w, h, bd, seed=3)
    got = R.denoise_plane(u, A, S, T, q)
    assert np.array_equal(got, direct(u, A, S, T, q))
    assert (got != u).any() or w * h == 1


def test_properties_of_the_filter():
    for bd in (8, 12):
        T, q = R.table_from_formula(bd, 2, 6.0)
        top = (1 << bd) - 1
        dt = np.uint8 if bd == 8 else np.uint16
        for value in (0, 77 << (bd - 8), top):  # a constant plane comes back unchanged
            c = np.full((19, 23), value, dt)
            assert np.array_equal(R.denoise_plane(c, 3, 2, T, q), c)
        u = plane(41, 29, bd, seed=1)
        out = R.denoise_plane(u, 3, 2, T, q)
        assert (out != u).any() and out.min() >= u.min() and out.max() <= u.max()
        # rule 2 makes the filter symmetric: transposed and mirrored input, transposed and mirrored output
        assert np.array_equal(R.denoise_plane(np.ascontiguousarray(u.T), 3, 2, T, q), out.T)
        assert np.array_equal(R.denoise_plane(np.ascontiguousarray(u[:, ::-1]), 3, 2, T, q), out[:, ::-1])
        assert np.array_equal(R.denoise_plane(np.ascontiguousarray(u[::-1]), 3, 2, T, q), out[::-1])
        # a strength so small that T[1] = 0: q = 0, only identical patches count, and they have the same centre
        Ti, qi = R.table_from_formula(bd, 2, 0.001)
        assert qi == 0 and Ti[1] == 0
        assert np.array_equal(R.denoise_plane(u, 3, 2, Ti, qi), u)
        # a checkerboard of 0 and max
        chk = (((np.arange(29)[:, None] + np.arange(41)[None, :]) & 1) * top).astype(dt)
        assert np.array_equal(R.denoise_plane(chk, 3, 2, T, q), chk)
    # the ceiling of rule 4: all-max at 12 bit, A = 7, every weight 4096
    T, q = R.table_from_formula(12, 4, 1000.0)
    full = np.full((20, 20), 4095, np.uint16)
    assert np.array_equal(R.denoise_plane(full, 7, 4, T, q), full)


def test_commands_refuse_with_one_logged_line(tmp_path, caplog):
    from grav1synth_amd import cli

    src = tmp_path / "a.y4m"
    src.write_bytes(b"x")
    den = tmp_path / "d.y4m"
    den.write_bytes(b"y")
    out = tmp_path / "o.y4m"
    tbl = tmp_path / "t.tbl"

    def one_line(text, call):
        caplog.clear()
        with caplog.at_level("INFO", logger="grav1synth"):
            assert call() == -1
        assert [r.getMessage() for r in caplog.records] == [text]

    one_line(cli.SAME_AS_OUTPUT, lambda: cli.denoise_command(str(src), str(src)))
    out.write_bytes(b"keep")
    one_line(cli.NOT_OVERWRITING, lambda: cli.denoise_command(str(src), str(out), confirm=lambda prompt: False))
    assert out.read_bytes() == b"keep"
    one_line(cli.NO_DENOISED, lambda: cli.diff_command(str(src), None, str(tbl)))
    one_line(cli.BOTH_DENOISED, lambda: cli.diff_command(str(src), str(den), str(tbl), denoise=True))
    one_line(cli.DENOISE_NO_FILTERS, lambda: cli.diff_command(str(src), None, str(tbl), filters="crop:top=2", denoise=True))
    one_line(cli.DENOISE_ONE_DEVICE, lambda: cli.diff_command(str(src), None, str(tbl), devices=[0, 1], denoise=True))
    one_line(cli.KEEP_NEEDS_DENOISE, lambda: cli.diff_command(str(src), str(den), str(tbl), keep_denoised=str(out)))
    one_line(cli.SAME_AS_OUTPUT, lambda: cli.diff_command(str(src), None, str(src), denoise=True))
    one_line(cli.SAME_AS_OUTPUT, lambda: cli.diff_command(str(src), None, str(tbl), denoise=True, keep_denoised=str(src)))
    one_line(cli.SAME_AS_OUTPUT, lambda: cli.diff_command(str(src), None, str(tbl), denoise=True, keep_denoised=str(tbl)))
    one_line(cli.NOT_OVERWRITING, lambda: cli.diff_command(str(src), None, str(tbl), denoise=True, keep_denoised=str(out),
                                                           confirm=lambda prompt: False))
    assert out.read_bytes() == b"keep" and not tbl.exists()
    # through main(): a refusal is a logged line and a normal exit
    assert cli.main(["diff", str(src), "-o", str(tbl)]) == 0
    assert cli.main(["diff", str(src), "--denoise", "--gpus", "2", "-o", str(tbl)]) == 0
    assert cli.main(["diff", str(src), "--denoise", "--devices", "0,1", "-o", str(tbl)]) == 0
    assert cli.main(["diff", str(src), "--denoise", "-f", "crop:top=2", "-o", str(tbl)]) == 0
    assert not tbl.exists()
    p = cli.build_parser()
    a = p.parse_args(["denoise", "in.y4m", "-o", "out.y4m", "-y", "--search-radius", "5", "--patch-radius", "3", "--strength", "2.5",
                      "--chroma-strength", "1.5", "--device", "1"])
    assert (a.input, a.output, a.overwrite, a.search_radius, a.patch_radius, a.strength, a.chroma_strength, a.device) == \
        ("in.y4m", "out.y4m", True, 5, 3, 2.5, 1.5, 1)
    a = p.parse_args(["diff", "s.y4m", "--denoise", "-o", "t.tbl", "--keep-denoised", "d.y4m", "--strength", "3"])
    assert (a.source, a.denoised, a.denoise, a.keep_denoised, a.strength, a.search_radius) == ("s.y4m", None, True, "d.y4m", 3.0, 0)
    a = p.parse_args(["diff", "s.y4m", "d.y4m", "-o", "t.tbl"])
    assert (a.source, a.denoised, a.denoise, a.keep_denoised) == ("s.y4m", "d.y4m", False, None)
