"""Coarse levels of `denoise` (rules 25 - 29 of include/g1s_diff.h) without a device: the restatement of
tests/denoise_levels_ref.py against plain loops and its identities, the lane bodies of the three kernels on the host under the
sanitizers, every new refusal on the three ladders and both commands, the command line, wrong restatements that must differ
from the reference on the content the device file uses, and what the levels are for on correlated grain."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from grav1synth_amd import _lib
from grav1synth_amd.denoise import denoise_opts
from tests import denoise_levels_content as LC
from tests import denoise_levels_ref as LR
from tests import denoise_motion_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ rules 25 and 27
@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (5, 1), (2, 2), (3, 5), (8, 6), (17, 9), (16, 16)])
@pytest.mark.parametrize("bd", [8, 12])
def test_merge_against_a_plain_double_loop(w, h, bd):
    rng = np.random.default_rng([w, h, bd])
    top = (1 << bd) - 1
    for trial in range(4):
        v = rng.integers(0, top + 1, (h, w))
        c = rng.integers(0, top + 1, ((h + 1) >> 1, (w + 1) >> 1))
        if trial & 1:  # near the ends of the range: the clip
            v = np.where(rng.random((h, w)) < 0.5, 0, top)
        assert np.array_equal(LR.merge(v, c, bd), LR.merge_loop(v, c, bd)), (w, h, bd, trial)


def test_the_identities():
    rng = np.random.default_rng(3)
    for w, h in ((1, 1), (7, 5), (16, 10), (33, 17)):
        v = rng.integers(0, 1024, (h, w))
        assert np.array_equal(LR.merge(v, M.half(v), 10), v), "d = 0 gives out = v"
        k = np.full((h, w), 517)
        assert np.array_equal(LR.merge(k, M.half(k), 10), k), "a constant plane stays constant"
        for delta in (-3, 4):  # a constant d moves every sample by it
            assert np.array_equal(LR.merge(k, M.half(k) + delta, 10), k + delta)
    frames, bd, ss, kw = LC.basic()
    from grav1synth_amd.denoise import weight_table

    plain = M.denoise_clip(frames, 1, 1, 0, 3, 2, weight_table(bd, 2, 4.0), weight_table(bd, 2, 4.0), 0)
    got = LR.denoise_clip(frames, 1, 1, bd, K=0)
    assert all(np.array_equal(a, b) for f, g in zip(got, plain) for a, b in zip(f, g)), "K = 0 is the filter of rules 1 - 24"
    assert LR.coarse_motion_range(64) == 32 and LR.coarse_motion_range(32) == 16 and LR.coarse_motion_range(2) == 2 and LR.coarse_motion_range(0) == 0
    assert LR.coarse_motion_range(6) == 4 and LR.coarse_motion_range(8) == 4
    assert LR.strengths(4.0, 6.0, 2, 0.5) == [(4.0, 6.0), (2.0, 3.0), (1.0, 1.5)]


@pytest.mark.parametrize("xdec", [0, 1])
def test_the_coarse_frame_is_a_frame(xdec):
    """rule 25: (W' + xdec) >> xdec = (cw + 1) >> 1, which is what coarse_frame() makes of the chroma planes"""
    for W in range(1, 68):
        cw = (W + xdec) >> xdec
        Wc = (W + 1) >> 1
        assert (Wc + xdec) >> xdec == (cw + 1) >> 1, W
        f = LR.coarse_frame([np.zeros((W, W), np.uint8), np.zeros((cw, cw), np.uint8), np.zeros((cw, cw), np.uint8)])
        assert f[0].shape == (Wc, Wc) and f[1].shape == f[2].shape == ((Wc + xdec) >> xdec,) * 2 and f[0].dtype == np.uint8


# ------------------------------------------------------------------------------------------- the lane bodies on the host
def test_the_lane_bodies_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "levels_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tests", "levels_host.cpp")]
    # (the sanitizer's runtime inside the program where the compiler can do that: it then starts under any preloaded library)
    if subprocess.call(cmd + ["-static-libasan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.split()[0] == "planes" and int(p.stdout.split()[1]) > 6000


# ----------------------------------------------------------------------------------------------------------- the refusals
LEVELS = "coarse_levels must be 0..2"
RATIO = "coarse_ratio must be 0.0625..4 (0 = 1)"
NEEDS = "coarse_ratio needs coarse_levels"
BOUND = " must be greater than 0 and at most 1000"
# (name, opts, (coarse_levels, coarse_ratio), other arguments of the constructor, the text)
BAD = [
    ("three levels", {}, (3, 0.0), {}, LEVELS),
    ("a ratio below 1/16", {}, (1, 0.06), {}, RATIO),
    ("a ratio above 4", {}, (2, 4.5), {}, RATIO),
    ("a negative ratio", {}, (1, -1.0), {}, RATIO),
    ("a ratio that is no number", {}, (1, float("nan")), {}, RATIO),
    ("a ratio without a level", {}, (0, 1.0), {}, NEEDS),
    ("level 1 too strong", dict(strength=300.0), (2, 4.0), {}, "level 1 strength" + BOUND),
    ("only level 2 too strong", dict(strength=100.0), (2, 4.0), {}, "level 2 strength" + BOUND),
    ("only level 2's chroma too strong", dict(strength=3.0, chroma_strength=100.0), (2, 4.0), {}, "level 2 chroma_strength" + BOUND),
    ("the default strength at level 2 is fine, 251 is not", dict(strength=251.0), (1, 4.0), {}, "level 1 strength" + BOUND),
    # the order: behind every refusal there was, in front of the device
    ("levels behind the levels' count", {}, (3, 9.0), {}, LEVELS),
    ("the range of the ratio in front of its need", {}, (0, 9.0), {}, RATIO),
    ("behind the search radius", dict(search_radius=8), (3, 0.0), {}, "search_radius must be 1..7"),
    ("behind the motion range", {}, (3, 0.0), dict(D=1, mr=7), "motion_range must be even and 0..64"),
    ("behind the strength of level 0", dict(strength=2000.0), (3, 0.0), {}, "strength" + BOUND),
    ("behind the chroma strength of level 0", dict(chroma_strength=2000.0), (1, 9.0), {}, "chroma_strength" + BOUND),
    ("behind the patch radius", dict(patch_radius=5), (3, 0.0), {}, "patch_radius must be 1..4"),
]


def new_levels(opts, K, rho, D=0, flags=0, mr=0):
    L = _lib.lib()
    h = L.g1s_denoise_new_levels(10, C.byref(opts), D, flags, None, None, mr, None, K, rho)
    text = L.g1s_last_global_error().decode()
    if h:
        L.g1s_denoise_free(h)
    return bool(h), text


@pytest.fixture()
def clip(tmp_path):
    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 C420\nFRAME\n" + bytes(12))
    return str(src).encode()


@pytest.mark.parametrize("name,okw,levels,other,text", BAD, ids=[b[0] for b in BAD])
def test_the_constructor_refuses_without_a_device(name, okw, levels, other, text):
    assert new_levels(denoise_opts(**okw), *levels, **other) == (False, text)


@pytest.mark.parametrize("name,okw,levels,other,text", BAD, ids=[b[0] for b in BAD])
def test_the_denoise_file_rung_refuses_without_a_device(name, okw, levels, other, text, clip, tmp_path):
    L = _lib.lib()
    err = C.create_string_buffer(512)
    out = tmp_path / "o.y4m"
    rc = L.g1s_denoise_y4m_file_levels(clip, str(out).encode(), C.byref(denoise_opts(**okw)), other.get("D", 0), 0, None, 0, -1, other.get("mr", 0), 0, 0, 0, 0,
                                       *levels, err, len(err))
    assert (rc, err.value.decode()) == (-1, text) and not out.exists()


@pytest.mark.parametrize("name,okw,levels,other,text", [b for b in BAD if not b[0].startswith("behind")], ids=[b[0] for b in BAD if not b[0].startswith("behind")])
def test_the_diff_file_rung_refuses_without_a_device(name, okw, levels, other, text, clip, tmp_path):
    """(the generator is made, on a device, before the denoiser: the levels' refusals are looked at with the flags', up front)"""
    L = _lib.lib()
    err, n = C.create_string_buffer(512), C.c_uint64(77)
    out = tmp_path / "o.tbl"
    rc = L.g1s_diff_y4m_file_denoised_levels(clip, str(out).encode(), None, None, C.byref(denoise_opts(**okw)), 0, 0, None, 0, -1, 0, 0, 0, 0, 0, *levels,
                                             C.byref(n), err, len(err))
    assert (rc, err.value.decode(), n.value) == (-1, text, 0) and not out.exists()


def test_the_diff_rung_names_null_paths_and_flags_first(clip, tmp_path):
    L = _lib.lib()
    err, n = C.create_string_buffer(512), C.c_uint64(0)
    call = lambda src, out, flags: (L.g1s_diff_y4m_file_denoised_levels(src, out, None, None, C.byref(denoise_opts()), 0, flags, None, 0, -1, 0, 0, 0, 0, 0, 3, 9.0,  # noqa: E731
                                                                        C.byref(n), err, len(err)), err.value.decode())
    out = str(tmp_path / "o.tbl").encode()
    assert call(None, out, 0) == (-1, "null path") and call(clip, out, 2) == (-1, "unknown denoise flags") and call(clip, out, 0) == (-1, LEVELS)
    # with the levels off, the new rungs are the ones before them
    e2 = C.create_string_buffer(512)
    a = L.g1s_diff_y4m_file_denoised_levels(clip, out, None, None, C.byref(denoise_opts()), 0, 0, b"/nonexistent-dir/p.tbl", 0, -1, 0, 0, 0, 0, 0, 0, 0.0, C.byref(n), err, len(err))
    b = L.g1s_diff_y4m_file_denoised_chroma(clip, out, None, None, C.byref(denoise_opts()), 0, 0, b"/nonexistent-dir/p.tbl", 0, -1, 0, 0, 0, 0, 0, C.byref(n), e2, len(e2))
    assert a == b == -1 and err.value == e2.value == b"grain prior: cannot open /nonexistent-dir/p.tbl"


# (name, opts, (coarse_levels, coarse_ratio), arguments) -> the text the diff rung gives.  The generator is made, on a device, before
# the denoiser, so the denoiser's older parameter refusals come behind a device there (tests/test_denoise_rungs_cpu.py leaves them
# out for that reason) and the levels' refusals, which need none, are looked at up front: on this rung, and on this rung only,
# they come IN FRONT of search_radius, patch_radius, the motion range and the strengths.  Pinned here so that the order is a choice.
DIFF_ORDER = [
    ("in front of the search radius", dict(search_radius=8), (3, 0.0), {}, LEVELS),
    ("in front of the patch radius", dict(patch_radius=5), (1, 9.0), {}, RATIO),
    ("in front of the motion range", {}, (0, 0.5), dict(D=1, mr=7), NEEDS),
    ("in front of a strength rule 3 refuses, over the defaults", dict(strength=2000.0), (3, 0.0), {}, LEVELS),
    ("a strength rule 3 refuses is not scaled", dict(strength=2000.0), (2, 4.0), {}, None),
    ("opts of another size are not read", dict(struct_size=8, strength=300.0), (2, 4.0), {}, None),
    ("behind the flags", {}, (3, 0.0), dict(flags=2), "unknown denoise flags"),
    ("in front of the prior", {}, (3, 0.0), dict(prior=b"/nonexistent-dir/p.tbl"), LEVELS),
    ("in front of the chroma prior's refusals", {}, (3, 0.0), dict(chroma_prior=2), LEVELS),
]


@pytest.mark.parametrize("name,okw,levels,other,text", DIFF_ORDER, ids=[b[0] for b in DIFF_ORDER])
def test_the_order_of_the_diff_rung(name, okw, levels, other, text, clip, tmp_path):
    L = _lib.lib()
    err, n = C.create_string_buffer(512), C.c_uint64(77)
    out = tmp_path / "o.tbl"
    opts = denoise_opts(**{k: v for k, v in okw.items() if k != "struct_size"})
    opts.struct_size = okw.get("struct_size", opts.struct_size)
    rc = L.g1s_diff_y4m_file_denoised_levels(clip, str(out).encode(), None, None, C.byref(opts), other.get("D", 0), other.get("flags", 0), other.get("prior"), 0, -1,
                                             other.get("mr", 0), 0, 0, 0, other.get("chroma_prior", 0), *levels, C.byref(n), err, len(err))
    got = err.value.decode()
    assert rc != 0 and n.value == 0 and not out.exists()
    if text is None:  # no refusal of the levels: what follows is the generator's or the constructor's, never a "level l" text
        assert not got.startswith("level ") and got not in (LEVELS, RATIO, NEEDS), got
    else:
        assert (rc, got) == (-1, text)


def test_python_passes_the_refusals_on(clip, tmp_path):
    from grav1synth_amd.denoise import Denoiser, denoise_y4m_file
    from grav1synth_amd.ingest import diff_y4m_file_denoised

    with pytest.raises(_lib.G1SError) as e:
        Denoiser(8, coarse_levels=3)
    assert LEVELS in str(e.value)
    with pytest.raises(_lib.G1SError) as e:
        Denoiser(8, coarse_ratio=0.5)
    assert NEEDS in str(e.value)
    with pytest.raises(_lib.G1SError) as e:
        denoise_y4m_file(clip.decode(), str(tmp_path / "o.y4m"), coarse_levels=2, coarse_ratio=4.0, strength=100.0)
    assert "level 2 strength" + BOUND in str(e.value)
    with pytest.raises(RuntimeError) as e:
        diff_y4m_file_denoised(clip.decode(), str(tmp_path / "o.tbl"), coarse_levels=1, coarse_ratio=8.0)
    assert RATIO in str(e.value)


# ------------------------------------------------------------------------------------------------------- the command line
def test_the_command_line(tmp_path, caplog):
    from grav1synth_amd import cli

    p = cli.build_parser()
    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
    out, tbl = tmp_path / "o.y4m", tmp_path / "t.tbl"

    def one_line(text, call):
        caplog.clear()
        with caplog.at_level("INFO", logger="grav1synth"):
            assert call() == -1
        got = [r.getMessage() for r in caplog.records]
        assert got == [text], got

    dn, df = cli.denoise_command, cli.diff_command
    for k, r, text in ((3, 0.0, cli.BAD_COARSE_LEVELS), (-1, 0.0, cli.BAD_COARSE_LEVELS), (1, 5.0, cli.BAD_COARSE_RATIO), (2, 0.01, cli.BAD_COARSE_RATIO),
                       (0, 0.5, cli.RATIO_NEEDS_LEVELS)):
        one_line(text, lambda: dn(str(src), str(out), coarse_levels=k, coarse_ratio=r))
        one_line(text, lambda: df(str(src), None, str(tbl), denoise=True, coarse_levels=k, coarse_ratio=r))
    assert not out.exists() and not tbl.exists()
    a = p.parse_args(["denoise", "a.y4m", "-o", "b.y4m", "--coarse-levels", "2", "--coarse-ratio", "0.5"])
    assert cli._denoise_parameters(a)["coarse_levels"] == 2 and cli._denoise_parameters(a)["coarse_ratio"] == 0.5
    a = p.parse_args(["diff", "a.y4m", "--denoise", "-o", "t.tbl", "--coarse-levels", "1"])
    assert cli._denoise_parameters(a)["coarse_levels"] == 1 and cli._denoise_parameters(a)["coarse_ratio"] == 0.0
    a = p.parse_args(["denoise", "a.y4m", "-o", "b.y4m"])
    assert cli._denoise_parameters(a)["coarse_levels"] == 0 and cli._denoise_parameters(a)["coarse_ratio"] == 0.0


# ------------------------------------------------------------------------------------------------ wrong restatements
def differs(case, wrong):
    frames, bd, ss, kw = case
    kw = dict(kw, rho=kw.get("rho", 0.0) or 1.0)
    want = LR.denoise_clip(frames, *LC.SUB[ss], bd, **kw)
    got = LR.denoise_clip(frames, *LC.SUB[ss], bd, wrong=(wrong,), **kw)
    return sum(int((np.asarray(a).astype(np.int64) != np.asarray(b).astype(np.int64)).sum()) for f, g in zip(want, got) for a, b in zip(f, g))


WRONG_ON = [("nearest", LC.basic), ("trunc", LC.basic), ("mirror", LC.basic), ("noclip", LC.clipping), ("coarse_from_output", LC.basic),
            ("merge_before_inverse", LC.with_curve), ("mr_not_halved", lambda: LC.panned(8)), ("mr_not_halved", lambda: LC.panned(6)),
            ("no_rho", lambda: LC.ratio(0.5)), ("no_rho", lambda: LC.ratio(4.0)), ("fine_guide", LC.joint)]


@pytest.mark.parametrize("wrong,case", WRONG_ON, ids=[f"{w}-{k}" for k, (w, _c) in enumerate(WRONG_ON)])
def test_a_wrong_restatement_differs_on_the_content_the_device_file_uses(wrong, case):
    n = differs(case(), wrong)
    print(wrong, "differs in", n, "samples")
    assert n > 0


def test_the_unclipped_sum_leaves_the_range_at_both_ends():
    frames, bd, ss, kw = LC.clipping()
    raw = LR.denoise_clip(frames, 1, 1, bd, wrong=("noclip",), **kw)[0][0]
    assert raw.min() < 0 and raw.max() > (1 << bd) - 1


# ----------------------------------------------------------------------------------------------- what the levels are for
def box_gain(residual, n=8):
    """the variance of the n x n box means of a residual over its own variance, times n^2: 1 for white noise"""
    h, w = residual.shape
    r = residual[:h // n * n, :w // n * n].astype(np.float64)
    r = r - r.mean()
    means = r.reshape(h // n, n, w // n, n).mean((1, 3))
    return float(means.var() * n * n / r.var())


def test_on_correlated_grain_two_levels_leave_less_and_remove_coarser(capsys):
    """160 x 160, 10 bit, a ramp, grain of sigma 16 through a 3 x 3 box, h = 4, A = 3, S = 2, rho = 1 (seeded; direction only)"""
    w = h = 160
    rng = np.random.default_rng(2026)
    clean = np.clip(np.rint(200.0 + 3.5 * np.arange(w)[None, :] + 0.0 * np.arange(h)[:, None]), 0, 1023)
    noisy = np.clip(np.rint(clean + LC.correlated(rng, w, h, 16.0)), 0, 1023).astype(np.uint16)
    left, gain = {}, {}
    for K in (0, 2):
        out = LR.denoise_clip([[noisy]], 1, 1, 10, K=K, rho=1.0)[0][0].astype(np.float64)
        inner = (slice(16, -16), slice(16, -16))
        left[K] = float((out - clean)[inner].std())
        gain[K] = box_gain((noisy.astype(np.float64) - out)[inner])
    own = box_gain((noisy.astype(np.float64) - clean)[16:-16, 16:-16])
    print(f"error left: K = 0 {left[0]:.2f}, K = 2 {left[2]:.2f}; removed residual's 8 x 8 box gain: K = 0 {gain[0]:.2f}, K = 2 {gain[2]:.2f}; the grain's own {own:.2f}")
    assert left[2] < left[0] and gain[2] > gain[0]
