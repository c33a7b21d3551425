"""The grain prior of `denoise` (rules 12 - 15) without a device: the library's curve builder against the numpy
restatement, the curve's properties, the refusals, what the option is for, the lane body of kd_curve on the host under the
sanitizers, and the commands' wiring."""
from __future__ import annotations

import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from grav1synth_amd import _lib
from grav1synth_amd.denoise import Denoiser, denoise_opts, grain_curve
from grav1synth_amd.diff import GrainTableSegment
from grav1synth_amd.tbl import parse_tbl
from tests import denoise_curve_ref as CR
from tests import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "tests", "golden", "reference-example-table.tbl")


def segment(points) -> GrainTableSegment:
    return GrainTableSegment(random_seed=1, start_time=0, end_time=1 << 40, scaling_points_y=[tuple(p) for p in points], scaling_points_cb=[],
                             scaling_points_cr=[], scaling_shift=8, ar_coeff_lag=0, ar_coeffs_y=[], ar_coeffs_cb=[0], ar_coeffs_cr=[0], ar_coeff_shift=6,
                             cb_mult=128, cb_luma_mult=192, cb_offset=256, cr_mult=128, cr_luma_mult=192, cr_offset=256,
                             chroma_scaling_from_luma=False, grain_scale_shift=0, overlap_flag=False)


def random_points(rng, npoints):
    """npoints luma scaling points: increasing values, 0 and 255 among them and among the scalings."""
    xs = sorted(rng.choice(256, npoints, replace=False).tolist())
    if npoints and rng.integers(2):
        xs[0] = 0
    if npoints > 1 and rng.integers(2):
        xs[-1] = 255
    return [(x, int(rng.choice([0, 255, int(rng.integers(0, 256))]))) for x in xs]


def tables():
    """(name, the luma points of each segment)"""
    out = [("example", [s.scaling_points_y for s in parse_tbl(open(EXAMPLE, "rb").read())])]
    rng = np.random.default_rng(15)
    for n in range(1, 6):
        for k in range(3):
            out.append((f"random-{n}-{k}", [random_points(rng, int(rng.integers(0, 15))) for _ in range(n)]))
    out.append(("fourteen-points", [random_points(rng, 14)]))
    out.append(("no-luma-points", [[]]))
    out.append(("one-of-two-without-points", [[], [(0, 20), (255, 80)]]))
    out.append(("single-point", [[(128, 40)]]))
    out.append(("all-255", [[(0, 255), (255, 255)]]))
    out.append(("two-level-step", [[(0, 10), (127, 10), (128, 200), (255, 200)]]))
    return out


TABLES = tables()


def check_properties(fwd, inv, bd):
    M = (1 << bd) - 1
    assert fwd.shape == (M + 1,) and inv.shape == (4096,)
    assert fwd[0] == 0 and fwd[M] == 4095
    assert (np.diff(fwd.astype(np.int64)) > 0).all(), "f is strictly increasing"
    assert np.array_equal(inv[fwd], np.arange(M + 1)), "g(f(x)) = x"
    assert (np.diff(inv.astype(np.int64)) >= 0).all() and inv.max() <= M, "g is non-decreasing and stays in the clip's range"


@pytest.mark.parametrize("name,points", TABLES, ids=[t[0] for t in TABLES])
@pytest.mark.parametrize("bd", [8, 10])
def test_the_library_curve_equals_the_restatement(name, points, bd):
    segs = [segment(p) for p in points]
    for rng in (0, 1, CR.max_range(bd)):
        fwd, inv = grain_curve(segs, bd, rng)
        wf, wi = CR.curve(points, bd, rng)
        assert np.array_equal(fwd, wf), (rng, np.argwhere(fwd != wf)[:5])
        assert np.array_equal(inv, wi), (rng, np.argwhere(inv != wi)[:5])
        check_properties(fwd, inv, bd)


@pytest.mark.parametrize("bd", [8, 10])
def test_every_range_up_to_the_bound(bd):
    points = [[(0, 3), (40, 9), (41, 255), (200, 0), (255, 77)], [(10, 1)]]
    segs = [segment(p) for p in points]
    seen = set()
    for rng in range(0, CR.max_range(bd) + 1):
        fwd, inv = grain_curve(segs, bd, rng)
        wf, wi = CR.curve(points, bd, rng)
        assert np.array_equal(fwd, wf) and np.array_equal(inv, wi), rng
        check_properties(fwd, inv, bd)
        seen.add(fwd.tobytes())
    assert len(seen) > CR.max_range(bd) // 2, "the range matters (two ranges with one floor, ceil(max s / R), share a curve)"
    assert np.array_equal(grain_curve(segs, bd, 0)[0], grain_curve(segs, bd, min(4, CR.max_range(bd)))[0])


@pytest.mark.parametrize("bd", [8, 10])
def test_the_flat_curve_and_one_segment_of_a_table(bd):
    M = (1 << bd) - 1
    flat = ((4095 * np.arange(M + 1, dtype=np.int64) + (M >> 1)) // M).astype(np.uint16)
    step = [(0, 10), (127, 10), (128, 200), (255, 200)]
    assert np.array_equal(grain_curve([segment(step)], bd, 1)[0], flat), "R = 1 is the flat curve"
    assert np.array_equal(grain_curve([segment([])], bd)[0], flat), "and so is a table without luma grain"
    assert np.array_equal(grain_curve([segment([(0, 255), (255, 255)])], bd, CR.max_range(bd))[0], flat)
    # the slopes follow 1 / s(v), clamped to a factor R
    fwd, _ = grain_curve([segment(step)], bd, 4)
    slope = np.diff(fwd.astype(np.int64))
    lo, hi = slope[: 100 << (bd - 8)].mean(), slope[-(100 << (bd - 8)):].mean()
    assert 3.9 < lo / hi < 4.1, (lo, hi)
    # segment = K: that segment alone
    segs = [segment(step), segment([(0, 50)]), segment([(0, 9), (255, 90)])]
    for k in range(3):
        a, b = grain_curve(segs, bd, 0, segment=k), grain_curve([segs[k]], bd)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(grain_curve(segs, bd)[0], grain_curve(segs, bd, segment=0)[0])
    with pytest.raises(_lib.G1SError) as e:
        grain_curve(segs, bd, segment=3)
    assert "segment 3 is not in the table (3 segments)" in str(e.value)


# ---------------------------------------------------------------------------------------------------------- refusals
def test_the_builder_refuses_with_code_and_text():
    L = _lib.lib()
    seg = (_lib.G1SSegment * 1)(segment([(0, 20), (255, 80)]).to_c())
    fwd, inv = np.zeros(4096, np.uint16), np.zeros(4096, np.uint16)

    def refused(text, n, bd, rng, f=fwd, i=inv):
        assert L.g1s_denoise_curve(seg, n, bd, rng, f.ctypes.data if f is not None else None, i.ctypes.data if i is not None else None) == -1
        assert L.g1s_last_global_error().decode() == text

    no12 = "a grain prior needs headroom above the clip's bit depth: the stabilised domain is 12 bits, so a 12-bit clip is refused"
    refused(no12, 1, 12, 0)
    refused("a grain prior is defined for bit depths 8 and 10", 1, 9, 0)
    refused("prior range must be 1..16 at 8 bits (0 = the default)", 1, 8, 17)
    refused("prior range must be 1..4 at 10 bits (0 = the default)", 1, 10, 5)
    refused("a grain prior needs at least one segment", 0, 10, 0)
    refused("g1s_denoise_curve needs both output tables", 1, 10, 0, None)
    refused("g1s_denoise_curve needs both output tables", 1, 10, 0, fwd, None)
    bad = segment([(9, 20), (9, 80)])
    seg[0] = bad.to_c()
    refused("segment 0: luma scaling points must have increasing values", 1, 10, 0)
    with pytest.raises(_lib.G1SError) as e:
        grain_curve([segment([])], 12)
    assert no12 in str(e.value)


@pytest.mark.parametrize("bd", [8, 10])
def test_the_constructor_checks_the_pair_before_it_looks_for_a_device(bd):
    L = _lib.lib()
    M = (1 << bd) - 1
    good_f, good_i = grain_curve([segment([(0, 20), (255, 80)])], bd)
    opts = denoise_opts()

    def new(f, i, depth=bd, D=0, flags=0):
        h = L.g1s_denoise_new_curve(depth, C.byref(opts), D, flags, f.ctypes.data if f is not None else None, i.ctypes.data if i is not None else None)
        text = L.g1s_last_global_error().decode()
        if h:
            L.g1s_denoise_free(h)
        return bool(h), text

    def mutated(a, at, value):
        b = a.copy()
        b[at] = value
        return b

    cases = [
        ("curve: fwd must run from 0 to 4095", mutated(good_f, 0, 1), good_i),
        ("curve: fwd must run from 0 to 4095", mutated(good_f, M, 4094), good_i),
        (f"curve: fwd must be strictly increasing (at {M // 2})", mutated(good_f, M // 2, good_f[M // 2 - 1]), good_i),
        ("curve: fwd must be strictly increasing (at 7)", mutated(good_f, 7, 0), good_i),
        ("curve: inv must be non-decreasing (at 2001)", good_f, mutated(good_i, 2001, good_i[2000] - 1)),
        ("curve: inv must stay within the clip's bit depth (at 4095)", good_f, mutated(good_i, 4095, M + 1)),
        ("g1s_denoise_new_curve needs both tables of the curve", None, good_i),
        ("g1s_denoise_new_curve needs both tables of the curve", good_f, None),
    ]
    # inv[fwd[x]] != x with inv still non-decreasing and in range: the entries up to fwd[x] take the value before
    x = M // 3
    shifted = good_i.copy()
    shifted[int(good_f[x - 1]):int(good_f[x]) + 1] = x - 1
    cases.append((f"curve: inv[fwd[x]] must be x (at {x})", good_f, shifted))
    for text, f, i in cases:
        made, got = new(f, i)
        assert not made and got == text, (text, got)
    # the other refusals keep their place in front: parameters first, then the curve
    assert new(good_f, good_i, D=4) == (False, "temporal_radius must be 0..3")
    assert new(good_f, good_i, flags=2) == (False, "unknown denoise flags")
    assert new(mutated(good_f, 0, 1), good_i, flags=2) == (False, "unknown denoise flags")
    made, got = new(good_f, good_i, depth=12)
    assert not made and got.startswith("a grain prior needs headroom above the clip's bit depth")
    # and a pair that is fine gets as far as the device
    import torch

    made, got = new(good_f, good_i)
    if torch.cuda.is_available():
        assert made, got
    else:
        assert not made and got == "no HIP device available: denoise has no CPU fallback"
    with pytest.raises(_lib.G1SError) as e:
        Denoiser(bd, curve=(good_f[:-1], good_i))
    assert f"fwd must have {M + 1} entries and inv 4096" in str(e.value)
    with pytest.raises(_lib.G1SError) as e:
        Denoiser(bd, curve=(mutated(good_f, 0, 1), good_i))
    assert "curve: fwd must run from 0 to 4095" in str(e.value)


def test_the_file_calls_refuse_a_bad_prior_before_anything_else(tmp_path):
    L = _lib.lib()
    err = C.create_string_buffer(512)
    bad = tmp_path / "bad.tbl"
    bad.write_bytes(b"not a table\n")
    assert L.g1s_denoise_y4m_file_curve(b"/nonexistent.y4m", b"/nonexistent.out", None, 0, 0, str(bad).encode(), 0, -1, err, len(err)) == -1
    assert err.value.startswith(b"grain prior: ")
    assert L.g1s_denoise_y4m_file_curve(b"/nonexistent.y4m", b"/nonexistent.out", None, 0, 0, b"/nonexistent.tbl", 0, -1, err, len(err)) == -1
    assert err.value == b"grain prior: cannot open /nonexistent.tbl"
    assert L.g1s_denoise_y4m_file_curve(b"/nonexistent.y4m", b"/nonexistent.out", None, 0, 0, EXAMPLE.encode(), 0, 1, err, len(err)) == -1
    assert err.value == b"grain prior: segment 1 is not in the table (1 segments)"
    frames = C.c_uint64(7)
    assert L.g1s_diff_y4m_file_denoised_curve(b"/nonexistent.y4m", b"/nonexistent.tbl", None, None, None, 0, 0, str(bad).encode(), 0, -1, C.byref(frames), err,
                                              len(err)) == -1
    assert err.value.startswith(b"grain prior: ") and frames.value == 0
    assert L.g1s_diff_y4m_file_denoised_curve(b"/nonexistent.y4m", b"/nonexistent.tbl", None, None, None, 0, 0, EXAMPLE.encode(), 0, 5, None, err, len(err)) == -1
    assert err.value == b"grain prior: segment 5 is not in the table (1 segments)"
    # a 12-bit clip: refused with the reason when the clip's depth is known, before a device is looked for
    clip12 = tmp_path / "c12.y4m"
    clip12.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono12\nFRAME\n" + bytes(16))
    out = tmp_path / "o.y4m"
    assert L.g1s_denoise_y4m_file_curve(str(clip12).encode(), str(out).encode(), None, 0, 0, EXAMPLE.encode(), 0, -1, err, len(err)) == -1
    assert err.value.startswith(b"a grain prior needs headroom above the clip's bit depth") and not out.exists()


# ------------------------------------------------------------------------------------------------------ what it is for
def test_a_prior_denoises_signal_dependent_grain_better_than_one_strength():
    """10-bit 192 x 96, bands at 140 / 480 / 860 with texture, Gaussian grain of sigma 4 .. 16 following s(v) = round(20 +
    60 v / 1023) (seed 5), the prior that function as two points; A = 3, S = 2, R = 4, h in {1, 1.5, 2, 3, 4, 6}.  Measured:
    plain's best whole-plane MSE 30.26 at h = 4 with 27.92 in the dark band; stabilised 26.29 at h = 3 with 18.36 in the
    dark band (DESIGN 4.10 has every h).  Only the two strict inequalities are asserted."""
    clean, noisy, points = CR.band_content(seed=5)
    assert noisy.shape == (96, 192)
    fwd, inv = CR.curve([points], 10, 4)
    mse = lambda a, b: float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).mean())
    grid = [1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    plain, stab = {}, {}
    for h in grid:
        T, q = R.table_from_formula(10, 2, h)
        p = R.denoise_plane(noisy, 3, 2, T, q)
        s = CR.denoise_luma(noisy, fwd, inv, 3, 2, h)
        plain[h] = (mse(p, clean), mse(p[:, :64], clean[:, :64]), mse(p[:, 128:], clean[:, 128:]))
        stab[h] = (mse(s, clean), mse(s[:, :64], clean[:, :64]), mse(s[:, 128:], clean[:, 128:]))
        print(f"h {h}: plain total {plain[h][0]:.2f} dark {plain[h][1]:.2f} bright {plain[h][2]:.2f}; "
              f"stabilised total {stab[h][0]:.2f} dark {stab[h][1]:.2f} bright {stab[h][2]:.2f}")
    hp, hs = min(grid, key=lambda h: plain[h][0]), min(grid, key=lambda h: stab[h][0])
    print(f"unfiltered total {mse(noisy, clean):.2f} bright {mse(noisy[:, 128:], clean[:, 128:]):.2f}; best plain at h {hp}, best stabilised at h {hs}")
    assert stab[hs][0] < plain[hp][0]
    assert stab[hs][1] < plain[hp][1]


# ---------------------------------------------------------------------------------------- the lane body on the host
def test_the_lane_body_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "curve_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tests", "curve_host.cpp")]
    # (the sanitizer's runtime inside the program where the compiler can do that: it then starts under any preloaded library)
    if subprocess.call(cmd + ["-static-libasan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.split()[0] == "rows" and int(p.stdout.split()[1]) > 30000


# ------------------------------------------------------------------------------------------------------ the commands
def test_commands_refuse_with_one_logged_line(tmp_path, caplog):
    from grav1synth_amd import cli

    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
    src12 = tmp_path / "a12.y4m"
    src12.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono12\nFRAME\n" + bytes(16))
    bad = tmp_path / "bad.tbl"
    bad.write_bytes(b"filmgrn1\nE 0 1 1 1\n")
    out, tbl, keep = tmp_path / "o.y4m", tmp_path / "t.tbl", tmp_path / "k.y4m"

    def one_line(text, call):
        caplog.clear()
        with caplog.at_level("INFO", logger="grav1synth"):
            assert call() == -1
        got = [r.getMessage() for r in caplog.records]
        assert len(got) == 1 and (got[0] == text or (text.endswith("...") and got[0].startswith(text[:-3]))), got

    dn, df = cli.denoise_command, cli.diff_command
    one_line(cli.PRIOR_NEEDS_TABLE, lambda: dn(str(src), str(out), prior_range=2))
    one_line(cli.PRIOR_NEEDS_TABLE, lambda: dn(str(src), str(out), prior_segment=0))
    one_line(cli.PRIOR_NEEDS_TABLE, lambda: df(str(src), None, str(tbl), denoise=True, prior_range=2))
    one_line(cli.PRIOR_NEEDS_TABLE, lambda: df(str(src), None, str(tbl), denoise=True, prior_segment=0))
    one_line(cli.SAME_AS_OUTPUT, lambda: dn(str(src), EXAMPLE, grain_prior=EXAMPLE))
    one_line(cli.SAME_AS_OUTPUT, lambda: df(str(src), None, EXAMPLE, denoise=True, grain_prior=EXAMPLE))
    one_line(cli.SAME_AS_OUTPUT, lambda: df(str(src), None, str(tbl), denoise=True, keep_denoised=EXAMPLE, grain_prior=EXAMPLE))
    one_line("Invalid grain prior: ...", lambda: dn(str(src), str(out), grain_prior=str(bad)))
    one_line("Invalid grain prior: ...", lambda: df(str(src), None, str(tbl), denoise=True, grain_prior=str(tmp_path / "missing.tbl")))
    one_line(cli.PRIOR_BAD_SEGMENT % (1, 1), lambda: dn(str(src), str(out), grain_prior=EXAMPLE, prior_segment=1))
    one_line(cli.PRIOR_BAD_SEGMENT % (-1, 1), lambda: df(str(src), None, str(tbl), denoise=True, grain_prior=EXAMPLE, prior_segment=-1))
    one_line(cli.PRIOR_12_BIT, lambda: dn(str(src12), str(out), grain_prior=EXAMPLE))
    one_line(cli.PRIOR_12_BIT, lambda: df(str(src12), None, str(tbl), denoise=True, keep_denoised=str(keep), grain_prior=EXAMPLE))
    assert not out.exists() and not tbl.exists() and not keep.exists()
    assert open(EXAMPLE, "rb").read().startswith(b"filmgrn1")
    # through main(): a logged line and a normal exit
    assert cli.main(["denoise", str(src), "-o", str(out), "--prior-range", "2"]) == 0 and not out.exists()
    assert cli.main(["diff", str(src), "--denoise", "-o", str(tbl), "--grain-prior", str(bad)]) == 0 and not tbl.exists()


def test_argument_wiring(monkeypatch, tmp_path):
    from grav1synth_amd import cli, denoise, ingest

    p = cli.build_parser()
    a = p.parse_args(["denoise", "in.y4m", "-o", "out.y4m", "--grain-prior", "t.tbl", "--prior-range", "3", "--prior-segment", "2"])
    assert cli._denoise_parameters(a)["grain_prior"] == "t.tbl" and cli._denoise_parameters(a)["prior_range"] == 3 and cli._denoise_parameters(a)["prior_segment"] == 2
    a = p.parse_args(["diff", "s.y4m", "--denoise", "-o", "t.tbl", "--grain-prior", "p.tbl"])
    assert a.grain_prior == "p.tbl" and a.prior_range == 0 and a.prior_segment is None
    a = p.parse_args(["denoise", "in.y4m", "-o", "out.y4m"])
    assert a.grain_prior is None and a.prior_range == 0 and a.prior_segment is None
    for f in (denoise.denoise_y4m_file, ingest.diff_y4m_file_denoised):
        sig = inspect.signature(f).parameters
        assert sig["grain_prior"].default is None and sig["prior_range"].default == 0 and sig["prior_segment"].default is None
        assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("grain_prior", "prior_range", "prior_segment"))
    assert inspect.signature(denoise.Denoiser.__init__).parameters["curve"].default is None
    seen = {}
    monkeypatch.setattr(denoise, "denoise_y4m_file", lambda i, o, **kw: seen.update(denoise=kw) or 3)
    monkeypatch.setattr(ingest, "diff_y4m_file_denoised", lambda s, o, **kw: seen.update(diff=kw) or 3)
    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
    assert cli.main(["denoise", str(src), "-o", str(tmp_path / "o.y4m"), "--grain-prior", EXAMPLE, "--prior-range", "2", "--prior-segment", "0"]) == 0
    assert (seen["denoise"]["grain_prior"], seen["denoise"]["prior_range"], seen["denoise"]["prior_segment"]) == (EXAMPLE, 2, 0)
    assert cli.main(["denoise", str(src), "-o", str(tmp_path / "o2.y4m")]) == 0 and seen["denoise"]["grain_prior"] is None
    assert cli.main(["diff", str(src), "--denoise", "-o", str(tmp_path / "t.tbl"), "--grain-prior", EXAMPLE, "--temporal-radius", "1"]) == 0
    assert seen["diff"]["grain_prior"] == EXAMPLE and seen["diff"]["prior_segment"] is None and seen["diff"]["temporal_radius"] == 1
