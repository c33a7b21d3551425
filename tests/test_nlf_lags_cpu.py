"""Lagged noise levels without a device: the numpy restatement of rules L1 - L5 (tests/nlf_lags_ref.py) against a plain loop,
its identities, the wrong restatements it must be told apart from, and the host-only sum (g1s_nlf_sum_lags) against it --
through the library and compiled alone under the sanitizers."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import nlf_lags_ref as LG
from tests import nlf_t_ref as T
from tests.nlf_lags_content import SUBSAMPLINGS, ar_clip, clip_frames, gpu_content

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_same(a, b, what):
    for name in LG.NAMES:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f"{what}: {name}\n{x}\n{y}"


def differs(a, b, names):
    return any(not np.array_equal(np.asarray(a[n]), np.asarray(b[n])) for n in names)


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
@pytest.mark.parametrize("size", [(9, 7), (13, 11), (17, 9), (33, 27)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_equals_a_plain_loop(ss, size):
    w, h = size
    subx, suby = SUBSAMPLINGS[ss]
    for bd in (8, 10, 12):
        a, b = clip_frames(w, h, bd, ss, seed=5)
        got = LG.lags_pair(b, a, bd, subx, suby)
        assert_same(got, LG.lags_pair_loop(b, a, bd, subx, suby), f"{w}x{h} {bd} bit {ss}")
        if w >= 33:
            assert got["n"][0].min() > 0 and np.unique(got["r"][0]).size > 40 and np.unique(got["n"][0]).size > 20
            assert ss == "mono" or (got["xn"].min() > 0 and got["ln"] > 0 and got["xr"].any())


@pytest.mark.parametrize("h", [1, 2, 3, 4, 5])
def test_planes_smaller_than_the_window(h):
    """Widths 1 .. 8, heights 1 .. 5: lags that reach past the plane have no pairs."""
    for w in range(1, 9):
        for ss in ("420", "444", "mono", "422"):
            subx, suby = SUBSAMPLINGS[ss]
            a, b = clip_frames(w, h, 10, ss, seed=2, amp=1, fade=0)
            got = LG.lags_pair(b, a, 10, subx, suby)
            assert_same(got, LG.lags_pair_loop(b, a, 10, subx, suby), f"{w}x{h} {ss}")
            for i, (dx, dy) in enumerate(LG.LAGS):
                if abs(dx) > w - 3 or dy > h - 3:
                    assert got["n"][0, i] == 0 and got["r"][0, i] == 0, (w, h, i)


# ------------------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("ss", ["420", "444", "mono"])
def test_identities_with_the_temporal_record(ss):
    subx, suby = SUBSAMPLINGS[ss]
    for bd in (8, 10, 12):
        a, b = clip_frames(41, 29, bd, ss, seed=7)
        lag, t = LG.lags_pair(b, a, bd, subx, suby), T.nlf_pair(b, a, bd, subx, suby)
        for c in range(3):
            assert int(lag["n"][c, 0]) == int(t["n"][c].sum()) and int(lag["r"][c, 0]) == int(t["q"][c].sum()) and int(lag["s"][c]) == int(t["s"][c].sum())
        assert lag["n"][0, 0] > 0


def test_a_pair_against_itself():
    """All r = 0 and s = 0; n is the gate's pair counts, from the gate alone."""
    a = clip_frames(37, 23, 10, "420", seed=4)[0]
    got = LG.lags_pair(a, a, 10, 1, 1)
    assert not got["r"].any() and not got["s"].any() and not got["xr"].any() and got["ls"] == 0 and got["l2"] == 0
    for c in range(3):
        g, _ = LG.gate_and_difference(a[c], a[c], 10)
        for i, (dx, dy) in enumerate(LG.LAGS):
            x, y = LG.overlap(g, g, dx, dy)
            assert int(got["n"][c, i]) == int((x * y).sum())
    assert got["n"][0, 0] > got["n"][0, 45] > 0


def test_frames_swapped():
    """r and n equal, s and ls negated -- except where Round2 of a negated sum differs, which happens on this content."""
    a, b = clip_frames(41, 29, 10, "420", seed=7)
    ab, ba = LG.lags_pair(b, a, 10, 1, 1), LG.lags_pair(a, b, 10, 1, 1)
    for name in ("n", "r", "xn", "ln"):
        assert np.array_equal(ab[name], ba[name]), name
    assert np.array_equal(ab["s"], -ba["s"]) and ab["s"].any()
    # Round2(-S, 2) = -Round2(S, 2) unless S is 2 modulo 4: there the two differ by one, so ls is not simply negated
    g0, e0 = LG.gate_and_difference(b[0], a[0], 10)
    gl, lbar = LG.luma_under(g0, e0, *b[1].shape, 1, 1)
    _, lbar_swapped = LG.luma_under(g0, -e0, *b[1].shape, 1, 1)
    ties = int(((lbar != -lbar_swapped) & (gl == 1)).sum())
    assert ties > 0 and int(ab["ls"]) + int(ba["ls"]) == ties
    assert not np.array_equal(ab["xr"], ba["xr"]) and ab["l2"] != ba["l2"]


@pytest.mark.parametrize("i", range(1, 46, 4))
def test_a_difference_field_moved_by_a_lag_peaks_there(i):
    """Frame t = frame t - 1 + f(p) + f(p - d_i) for sparse f: the products at lag d_i see f twice."""
    dx, dy = LG.LAGS[i]
    rng = np.random.default_rng(i)
    h, w = 40, 48
    f = np.where(rng.random((h, w)) < 0.05, rng.integers(1, 3, (h, w)), 0)
    moved = np.zeros_like(f)
    src, dst = LG.overlap(f, moved, dx, dy)
    dst[...] = src
    before = np.full((h, w), 400, np.uint16)
    cur = (before + f + moved).astype(np.uint16)
    got = LG.lags_pair([cur], [before], 10, 0, 0)
    r = got["r"][0, 1:]
    assert int(np.argmax(r)) + 1 == i and r[i - 1] > 2 * np.partition(r, -2)[-2]


# ---------------------------------------------------------------------------------------------------- wrong restatements
def test_wrong_restatements_differ_on_the_gpu_content():
    frames = gpu_content()
    right = LG.lags_pair(frames[1], frames[0], 10, 1, 1)
    assert differs(LG.lags_pair(frames[1], frames[0], 10, 1, 1, gate_at="p"), right, ("n", "r")), "the gate at p only"
    assert differs(LG.lags_pair(frames[1], frames[0], 10, 1, 1, truncate=True), right, ("xr", "ls", "l2")), "Lbar truncating"
    # The box without the clamp cannot differ: a box that needs the clamp holds a sample of the luma plane's last column or
    # row, which is not interior, so gL = 0 there whatever Lbar is.  Lbar itself does differ there.
    assert not differs(LG.lags_pair(frames[1], frames[0], 10, 1, 1, clamp=False), right, LG.NAMES), "the clamp lies behind gL = 0"
    g0, e0 = LG.gate_and_difference(frames[1][0], frames[0][0], 10)
    (gl, lbar), (gl_n, lbar_n) = LG.luma_under(g0, e0, *frames[1][1].shape, 1, 1), LG.luma_under(g0, e0, *frames[1][1].shape, 1, 1, clamp=False)
    assert (lbar[-1] != lbar_n[-1]).any() and not gl[-1].any() and not gl_n[-1].any()
    assert differs(LG.lags_pair(frames[1], frames[0], 10, 1, 1, first_only=True), right, ("xn", "ln")), "gL from the first sample"
    assert frames[0][0].shape[0] % 2 == 1, "rule 12's clamp takes part: the luma height is odd"


def test_dx_mirrored_differs_on_a_diagonal_tap():
    """C(dx, dy) != C(-dx, dy) for a field with a diagonal tap."""
    rng = np.random.default_rng(11)
    h, w = 60, 70
    z = rng.integers(-3, 4, (h + 1, w + 1))
    e = z[1:, 1:] + z[:-1, :-1]  # e(p) shares a term with e(p + (1, 1)) and none with e(p + (-1, 1))
    before = np.full((h, w), 500, np.uint16)
    cur = (before + e).astype(np.uint16)
    right, wrong = LG.lags_pair([cur], [before], 10, 0, 0), LG.lags_pair([cur], [before], 10, 0, 0, mirror_dx=True)
    i_diag, i_anti = LG.LAGS.index((1, 1)), LG.LAGS.index((-1, 1))
    assert right["r"][0, i_diag] > 10 * abs(int(right["r"][0, i_anti])) and right["r"][0, i_diag] == wrong["r"][0, i_anti]
    assert differs(right, wrong, ("r",))


def test_sums_in_32_bits_differ_at_the_largest_differences():
    """The spikes of tests/test_gpu_nlf_t.py (e = +- 4088 at every third sample, the box sums equal): r[0] leaves 32 bits."""
    w, h = 200, 75
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    spike = (xs % 3 == 1) & (ys % 3 == 1)
    a = np.where(spike, 0, 2048).astype(np.uint16)
    b = np.where(spike, 4088, 2048 - 511).astype(np.uint16)
    right = LG.lags_pair([b], [a], 12, 0, 0)
    assert right["r"][0, 0] > 2 ** 32 and differs(LG.lags_pair([b], [a], 12, 0, 0, wrap32=True), right, ("r",))


def test_no_mean_removal_shows_on_a_fading_clip():
    """s carries the fade: r[0] / n[0] - (s / n[0])^2 is the noise's variance and r[0] / n[0] alone is not."""
    rng = np.random.default_rng(5)
    h, w = 64, 64
    before = (np.full((h, w), 400) + rng.integers(-2, 3, (h, w))).astype(np.uint16)
    cur = (np.full((h, w), 400 + 12) + rng.integers(-2, 3, (h, w))).astype(np.uint16)
    got = LG.lags_pair([cur], [before], 10, 0, 0)
    n, r, s = int(got["n"][0, 0]), int(got["r"][0, 0]), int(got["s"][0])
    assert n > 3000 and r / n > 140 and r / n - (s / n) ** 2 < 6


# ---------------------------------------------------------------------------------------------------------- host functions
def lib():
    from grav1synth_amd import _lib

    return _lib.lib()


def test_struct_layout_and_the_bindings():
    from grav1synth_amd import _lib
    from grav1synth_amd.estimate import NLF_LRECORD

    assert LG.LRECORD.itemsize == C.sizeof(_lib.G1SNlfLRecord) == NLF_LRECORD.itemsize == 8 * (2 * 138 + 3 + 100 + 3)
    for name in LG.NAMES:
        assert LG.LRECORD.fields[name][1] == getattr(_lib.G1SNlfLRecord, name).offset == NLF_LRECORD.fields[name][1], name


def test_sum_lags_against_the_restatement():
    from grav1synth_amd.estimate import NLF_LRECORD, noise_lags_sum

    frames = gpu_content(n=4)
    recs = LG.run_records(frames, 10, 1, 1)
    arr = np.array([LG.to_struct(r, NLF_LRECORD) for r in recs])
    got = noise_lags_sum(arr)
    assert not LG.mismatches(got, LG.sum_records(recs), "sum")
    assert not LG.mismatches(noise_lags_sum(arr[:0]), LG.empty_record(), "empty")


@pytest.mark.parametrize("field", ["n", "r", "s", "xn", "xr", "ln", "ls", "l2"])
def test_sum_lags_refuses_an_overflow_of_every_field(field):
    from grav1synth_amd._lib import G1SError
    from grav1synth_amd.estimate import NLF_LRECORD, noise_lags_sum

    signed = LG.DTYPES[field] is np.int64
    for big in ([2 ** 63 - 1, -(2 ** 63)] if signed else [2 ** 64 - 1]):
        a, b = LG.empty_record(), LG.empty_record()
        for rec, v in ((a, big), (b, -1 if big < 0 else 1)):
            flat = np.asarray(rec[field]).reshape(-1).copy()
            flat[-1] = v
            rec[field] = flat.reshape(LG.SHAPES[field])
        with pytest.raises(OverflowError):
            LG.sum_records([a, b])
        arr = np.array([LG.to_struct(a, NLF_LRECORD), LG.to_struct(b, NLF_LRECORD)])
        with pytest.raises(G1SError):
            noise_lags_sum(arr)
        assert not LG.mismatches(noise_lags_sum(arr[:1]), a, "one record")


def test_null_arguments_are_refused():
    L = lib()
    rec = np.zeros(1, LG.LRECORD)
    assert L.g1s_nlf_sum_lags(None, 1, rec.ctypes.data) != 0 and L.g1s_nlf_sum_lags(rec.ctypes.data, 1, None) != 0
    assert L.g1s_nlf_sum_lags(None, 0, rec.ctypes.data) == 0


def test_the_lag_symbols_are_bound_and_new_lags_refuses_before_a_device_is_looked_for():
    L = lib()
    assert not L.g1s_nlf_new_lags(9, None) and b"bit depths 8, 10 and 12" in L.g1s_last_global_error()
    assert L.g1s_nlf_finish_lags(None, None, 0, None) != 0 and L.g1s_nlf_lag_times(None, None, None, None) != 0


def test_host_functions_alone_under_the_sanitizers(tmp_path):
    """nlf_table.cpp with a host compiler alone, in a stand-alone program (tests/nlf_table_host.cpp) under address and
    undefined-behaviour sanitizers: the sum of records written by this test against the restatement's, the overflow, and the
    AR fit on the sum."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "nlf_table_host")
    src = [os.path.join(ROOT, "tests", "nlf_table_host.cpp")] + [os.path.join(ROOT, "grav1synth_amd", "csrc", f) for f in ("nlf_table.cpp", "fold.cpp")]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe] + src)
    recs = LG.run_records(ar_clip(), 10, 1, 1)
    np.array([LG.to_struct(r) for r in recs]).tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "overflow refused" in out.stdout and f"sizeof {LG.LRECORD.itemsize}" in out.stdout
    got = np.fromfile(str(tmp_path / "out.bin"), LG.LRECORD)
    total = LG.sum_records(recs)
    assert len(got) == 1 and not LG.mismatches(got[0], total, "sum")
    # g1s_nlf_ar on that sum at lag 3 and Nmin 400, printed as hexadecimal floats: the restatement's bit for bit
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("ar ")]
    assert len(lines) == 3
    for c, ln in enumerate(lines):
        x, gain = LG.noise_ar(total, c, 10, 3, 400)
        assert int(ln[1]) == c and [float.fromhex(v) for v in ln[2:-1]] == list(x) + [0.0] * (25 - len(x)) and float.fromhex(ln[-1]) == gain
    assert "refused: too few static sample pairs for a table" in out.stdout
    assert out.stdout.split("report-begin\n")[1].encode() == LG.format_noise_lags(total, len(recs), 10, 3, 3, 400)


# ------------------------------------------------------------------------------------------------- L6 - L7: the AR fit
@pytest.fixture(scope="module")
def ar_total():
    frames = ar_clip()
    total = LG.sum_records(LG.run_records(frames, 10, 1, 1))
    assert total["n"][:, 45].min() > 500 and total["xn"].min() > 500
    return total


@pytest.mark.parametrize("lag", [1, 2, 3])
def test_noise_ar_is_the_restatement_bit_for_bit(ar_total, lag):
    from grav1synth_amd.estimate import NLF_LRECORD, noise_ar

    rec = LG.to_struct(ar_total, NLF_LRECORD)
    for c in range(3):
        x, gain = noise_ar(rec, c, 10, 1, 1, lag, min_count=400)
        want_x, want_gain = LG.noise_ar(ar_total, c, 10, lag, min_count=400)
        assert x.shape == (2 * lag * (lag + 1) + (c > 0),) and x.tobytes() == want_x.tobytes() and gain == want_gain, (c, x, want_x, gain, want_gain)
        assert gain > 1.05 and x[-1 - (c > 0)] > 0.15, "the left neighbour's tap of box-filtered noise, and a gain above 1"
        assert c == 0 or x[-1] > 0.1, "the luma coefficient"
        no_mean = LG.noise_ar(ar_total, c, 10, lag, min_count=400, remove_mean=False)[0]
        assert no_mean.tobytes() != want_x.tobytes()


def test_noise_ar_without_mean_removal_is_wrong_on_a_fade():
    """A fade of 9 code values a frame under white noise: with the mean removed the taps are near zero, without it every
    covariance carries the fade's square."""
    rng = np.random.default_rng(9)
    frames = [[(500 - 9 * t + rng.integers(-3, 4, (64, 96))).astype(np.uint16)] for t in range(3)]
    total = LG.sum_records(LG.run_records(frames, 10, 0, 0))
    right, wrong = LG.noise_ar(total, 0, 10, 1, 400)[0], LG.noise_ar(total, 0, 10, 1, 400, remove_mean=False)[0]
    assert np.abs(right).max() < 0.1 < np.abs(wrong).max()


def test_noise_ar_refusals(ar_total):
    from grav1synth_amd._lib import G1SError
    from grav1synth_amd.estimate import NLF_LRECORD, noise_ar

    def refused(total, c, lag, min_count, text, bd=10):
        with pytest.raises(G1SError) as e:
            noise_ar(LG.to_struct(total, NLF_LRECORD), c, bd, 1, 1, lag, min_count)
        assert text in str(e.value), str(e.value)
        if bd == 10 and lag in (1, 2, 3) and c < 3:
            with pytest.raises(ValueError) as v:
                LG.noise_ar(total, c, 10, lag, min_count)
            assert text in str(v.value)

    refused(ar_total, 1, 3, 0, LG.TOO_FEW)  # the default Nmin of 4096 is above this clip's chroma counts
    n0 = min(int(ar_total["n"][0, LG.lag_index(dx, dy)]) for dy in (0, 1) for dx in range(-2, 3))  # the fewest pairs among lag 1's lags
    refused(ar_total, 0, 1, n0 + 1, LG.TOO_FEW)
    assert len(noise_ar(LG.to_struct(ar_total, NLF_LRECORD), 0, 10, 1, 1, 1, n0)[0]) == 4, "on the count it is fine"
    # a lag only the largest fit needs: n of d = (-6, 3), of (-3, 0) and (3, -3), one below Nmin refuses lag 3 and not lag 2; d = (6, 3)
    # is the difference of no two members (dy = 0 has no dx > 0) and is not looked at
    few = {k: np.array(v, copy=True) for k, v in ar_total.items()}
    few["n"][0, LG.lag_index(6, 3)] = 0
    assert len(noise_ar(LG.to_struct(few, NLF_LRECORD), 0, 10, 1, 1, 3, 400)[0]) == 24
    few["n"][0, LG.lag_index(-6, 3)] = 399
    refused(few, 0, 3, 400, LG.TOO_FEW)
    assert len(noise_ar(LG.to_struct(few, NLF_LRECORD), 0, 10, 1, 1, 2, 400)[0]) == 12
    for name, at in (("xn", (0, 24)), ("xn", (0, 0)), ("ln", ())):
        few = {k: np.array(v, copy=True) for k, v in ar_total.items()}
        few[name][at] = 399
        refused(few, 1, 3, 400, LG.TOO_FEW)
        assert len(noise_ar(LG.to_struct(few, NLF_LRECORD), 0, 10, 1, 1, 3, 400)[0]) == 24, "luma does not look at them"
        if name == "xn":
            assert len(noise_ar(LG.to_struct(few, NLF_LRECORD), 2, 10, 1, 1, 3, 400)[0]) == 25, "nor the other chroma plane"
    # equal frames: every covariance is zero, the luma system is singular -- the fold's own text
    still = {k: np.array(v, copy=True) for k, v in ar_total.items()}
    for name in ("r", "s", "xr", "ls", "l2"):
        still[name] = np.zeros_like(still[name])
    refused(still, 0, 3, 400, LG.SINGULAR_LUMA)
    refused(ar_total, 0, 0, 400, "lag 1 .. 3")
    refused(ar_total, 0, 4, 400, "lag 1 .. 3")
    refused(ar_total, 3, 3, 400, "plane 0 .. 2")
    refused(ar_total, 0, 3, 400, "bit depths 8, 10 and 12", bd=9)


def test_a_singular_chroma_system_takes_the_fallback(ar_total):
    """A chroma plane that did not change: its own covariances are zero, the luma's variance is not: zero coefficients, and
    the luma coefficient b[m] / A[m][m] (here 0 / VL)."""
    from grav1synth_amd.estimate import NLF_LRECORD, noise_ar

    flat = {k: np.array(v, copy=True) for k, v in ar_total.items()}
    flat["r"][1] = 0
    flat["s"][1] = 0
    flat["xr"][0] = 0
    flat["xr"][0, 24] = 12345
    x, gain = noise_ar(LG.to_struct(flat, NLF_LRECORD), 1, 10, 1, 1, 3, 400)
    want_x, want_gain = LG.noise_ar(flat, 1, 10, 3, 400)
    assert x.tobytes() == want_x.tobytes() and gain == want_gain == 1.0 and not x[:24].any() and x[24] > 0


def test_the_fit_finds_a_known_ar_process_and_the_gate_is_what_lets_it_under_a_pan():
    """Luma grain from a known causal lag-1 AR process (taps 0.3 / 0.35 / -0.1 / 0.4), fresh every frame, over a picture of
    bars.  The bound is the sampling error: that of plain Yule-Walker on the pure grain of the same frames, measured here; the
    fit from the gated sums is within twice that, still and under a pan of 2 samples a frame, where the same Yule-Walker on the
    ungated frame difference (mean removed) is not."""
    taps = {(-1, -1): 0.3, (0, -1): 0.35, (1, -1): -0.1, (-1, 0): 0.4}
    h, w, n, pad = 120, 160, 4, 24
    rng = np.random.default_rng(77)
    ys, xs = np.arange(h)[:, None], np.arange(w + 2 * n)[None, :]
    picture = 300 + xs + ys + 160 * ((xs // 40) % 2)  # a slope with a bar edge every 40 columns

    def grain():
        g = np.zeros((h + pad, w + 2 * pad))
        z = rng.standard_normal(g.shape) * 5.0  # (the grain's variance is some 50: rounding to integers adds 1 / 12)
        for y in range(1, h + pad):
            for x in range(1, w + 2 * pad - 1):
                g[y, x] = z[y, x] + sum(a * g[y + dy, x + dx] for (dx, dy), a in taps.items())
        return g[pad:, pad:pad + w]

    grains = [grain() for _ in range(n)]

    def yule_walker(fields):
        """Plain Yule-Walker at lag 1 on the given fields, the mean of each removed."""
        o = LG.causal_offsets(1)
        cov = {}
        for dx in range(-2, 3):
            for dy in range(0, 2):
                a = b = 0.0
                for f in fields:
                    f = f - f.mean()
                    p, q = LG.overlap(f, f, dx, dy)
                    a, b = a + float((p * q).sum()), b + p.size
                cov[(dx, dy)] = cov[(-dx, -dy)] = a / b
        A = [[cov[(oi[0] - oj[0], oi[1] - oj[1])] for oj in o] for oi in o]
        return np.array(LG.gauss_solve(A, [cov[oi] for oi in o]))

    truth = np.array([taps[o] for o in LG.causal_offsets(1)])
    bound = 2 * np.abs(yule_walker(grains) - truth).max()
    print("sampling error of Yule-Walker on the pure grain: %.4f" % (bound / 2))
    assert bound < 0.08
    for pan in (0, 2):
        frames = [[np.clip(np.rint(picture[:, pan * t:pan * t + w] + grains[t]), 0, 1023).astype(np.uint16)] for t in range(n)]
        recs = LG.run_records(frames, 10, 0, 0)
        total = LG.sum_records(recs)
        kept = int(total["n"][0, 0]) / ((n - 1) * (h - 2) * (w - 2))
        gated = np.abs(LG.noise_ar(total, 0, 10, 1, 400)[0] - truth).max()
        diffs = [frames[t][0].astype(np.float64) - frames[t - 1][0] for t in range(1, n)]
        ungated = np.abs(yule_walker(diffs) - truth).max()
        print("pan %d: the gate keeps %.3f, gated error %.4f, ungated error %.4f" % (pan, kept, gated, ungated))
        assert gated <= bound, (pan, gated, bound)
        if pan:
            assert ungated > bound and kept > 0.5, "the gate is the feature"
        else:
            assert kept >= 0.9, "the grain is small enough for the gate to keep nine samples in ten"


# ------------------------------------------------------------------- that it estimates: a table's grain, rendered and found
def _rendered_grain(n, w, h, bd, subx, suby):
    """(the table, its grain alone on n frames): tests/grain_ref.add_noise from a fixed lag-3 table whose three planes differ,
    with luma coefficients in chroma, one flat scaling function for all planes (so that the luma coefficient survives the
    scaling), a new random_seed a frame.  The grain does not depend on the picture under it: it is rendered onto mid grey."""
    import dataclasses

    from tests import grain_ref as G
    from tests.test_gpu_grain import make_segment

    flat = [(0, 44), (255, 44)]
    seg = dataclasses.replace(make_segment(lag=3, seed=4321, scaling_shift=11, ar_shift=7), scaling_points_y=flat, scaling_points_cb=flat,
                              scaling_points_cr=flat)
    assert seg.ar_coeffs_cb[24] != 0 and seg.ar_coeffs_cr[24] != 0 and seg.ar_coeffs_cb != seg.ar_coeffs_cr
    grey = [np.full(s, 1 << (bd - 1), np.uint16) for s in ((h, w), ((h + suby) >> suby, (w + subx) >> subx), ((h + suby) >> suby, (w + subx) >> subx))]
    grains = []
    for t in range(n):
        noisy = G.add_noise(grey, dataclasses.replace(seg, random_seed=1000 + 37 * t), bd, subx, suby)
        grains.append([a.astype(np.int64) - b for a, b in zip(noisy, grey)])
    return seg, grains


def test_the_fit_finds_a_tables_coefficients_still_and_under_a_pan():
    """10-bit 4:2:0, five frames of 256 x 192: a smooth picture (a slope; a bar edge every 64 columns so that a pan shows)
    under a lag-3 table's rendered grain.  The bound is what nobody can beat: the error of ungated Yule-Walker (the same
    equations, every sample counting) on the pure rendered grain of the same frames against the table's coefficients,
    coef / 2^shift, measured here per plane; g1s_nlf_ar on the gated sums of the frames is within twice that on every plane,
    still and under a pan of 2 samples a frame, where the ungated fit on the frame differences is not: the gate is the
    feature."""
    from grav1synth_amd.estimate import NLF_LRECORD, noise_ar

    bd, subx, suby, w, h, n = 10, 1, 1, 256, 192, 5
    seg, grains = _rendered_grain(n, w, h, bd, subx, suby)
    truth = [np.array(co, float) / (1 << seg.ar_coeff_shift) for co in (seg.ar_coeffs_y, seg.ar_coeffs_cb, seg.ar_coeffs_cr)]

    def ungated(fields_per_frame):
        recs = [LG.lags_of_fields([(np.ones(e.shape, np.int64), e) for e in planes], subx, suby) for planes in fields_per_frame]
        total = LG.sum_records(recs)
        return [np.abs(LG.noise_ar(total, c, bd, 3, 1)[0] - truth[c]).max() for c in range(3)]

    sampling = ungated(grains)
    print("error of ungated Yule-Walker on the pure rendered grain, per plane: %.4f %.4f %.4f" % tuple(sampling))
    for pan in (0, 2):
        frames = []
        for t in range(n):
            planes = []
            for c, g in enumerate(grains[t]):
                ph, pw = g.shape
                ys, xs = np.arange(ph)[:, None], np.arange(pw)[None, :] + ((pan * t) >> (subx if c else 0))
                picture = 300 + 40 * c + xs + ys + 120 * ((xs // (64 >> (subx if c else 0))) % 2)
                planes.append((picture + g).astype(np.uint16))
            frames.append(planes)
        total = LG.sum_records(LG.run_records(frames, bd, subx, suby))
        kept = [int(total["n"][c, 0]) / ((n - 1) * (frames[0][c].shape[0] - 2) * (frames[0][c].shape[1] - 2)) for c in range(3)]
        rec = LG.to_struct(total, NLF_LRECORD)
        gated = [np.abs(noise_ar(rec, c, bd, subx, suby, 3)[0] - truth[c]).max() for c in range(3)]
        diffs = [[frames[t][c].astype(np.int64) - frames[t - 1][c] for c in range(3)] for t in range(1, n)]
        plain = ungated(diffs)
        print("pan %d: the gate keeps %.3f %.3f %.3f; gated error %.4f %.4f %.4f; ungated on the differences %.4f %.4f %.4f" % (pan, *kept, *gated, *plain))
        assert min(kept) >= 0.9, "the grain is small enough for the gate to keep nine samples in ten"
        for c in range(3):
            assert gated[c] <= 2 * sampling[c], (pan, c, gated[c], sampling[c])
        if pan:
            assert min(plain[c] / sampling[c] for c in range(3)) > 2, "ungated, the pan is read as grain on every plane"


# ------------------------------------------------------------------------------------------ L8 - L9: the table, closure
CLOSURE_MEASURED = (0.0118, 0.0074, 0.0387)  # Y, Cb, Cr: measured with this test's own run (printed below)
CLOSURE_BOUND = (0.02, 0.02, 0.06)  # 1.5 x that, rounded up to a whole per cent; above 0.10 the units of L7 / L8 would be wrong


@pytest.fixture(scope="module")
def rendered_records():
    bd, subx, suby, w, h, n = 10, 1, 1, 256, 192, 5
    seg, grains = _rendered_grain(n, w, h, bd, subx, suby)
    frames = []
    for t in range(n):
        planes = []
        for c, g in enumerate(grains[t]):
            ph, pw = g.shape
            planes.append((300 + 40 * c + np.arange(pw)[None, :] + np.arange(ph)[:, None] + g).astype(np.uint16))
        frames.append(planes)
    return seg, T.sum_records(T.run_records(frames, bd, subx, suby)), LG.sum_records(LG.run_records(frames, bd, subx, suby))


def test_closure_the_table_renders_the_grain_it_was_made_from(rendered_records):
    """g1s_nlf_table on the records of a lag-3 table's rendered grain over a still slope; the segment it gives and the original,
    each rendered by tests/grain_ref onto flat grey (three frames, seeds of their own): sigma per plane.  There is no numpy
    restatement of the fold's strength solver and quantisation, so the deviation was measured with the library itself:
    1.18 % / 0.74 % / 3.87 % (Y / Cb / Cr); the bound is 1.5 x that, rounded up to a whole per cent."""
    import dataclasses

    from grav1synth_amd.estimate import NLF_LRECORD, NLF_TRECORD, noise_table
    from tests import grain_ref as G

    seg, ttotal, ltotal = rendered_records
    got = noise_table(T.to_struct(ttotal, NLF_TRECORD), LG.to_struct(ltotal, NLF_LRECORD), 10, 1, 1, 3, 3)
    assert got.ar_coeff_lag == 3 and got.random_seed == 10956 and got.start_time == 0 and got.end_time == 2 ** 63 - 1 and got.overlap_flag
    assert len(got.ar_coeffs_y) == 24 and len(got.ar_coeffs_cb) == len(got.ar_coeffs_cr) == 25 and got.ar_coeffs_cb[24] != 0
    assert got.scaling_points_y and got.scaling_points_cb and got.scaling_points_cr
    grey = [np.full(s, 512, np.uint16) for s in ((192, 256), (96, 128), (96, 128))]

    def sigmas(sg):
        per = [[], [], []]
        for t in range(3):
            noisy = G.add_noise(grey, dataclasses.replace(sg, random_seed=500 + t), 10, 1, 1)
            for c in range(3):
                per[c].append((noisy[c].astype(float) - 512).std())
        return [float(np.mean(v)) for v in per]

    want, have = sigmas(seg), sigmas(got)
    dev = [abs(b - a) / a for a, b in zip(want, have)]
    print("closure: sigma of the original %s, of the table made from its grain %s, relative deviation %s" % (want, have, dev))
    for c in range(3):
        assert dev[c] <= CLOSURE_BOUND[c], (c, dev[c])


def test_noise_table_refusals_and_a_plane_without_points(rendered_records):
    from grav1synth_amd._lib import G1SError
    from grav1synth_amd.estimate import NLF_LRECORD, NLF_TRECORD, noise_table

    _, ttotal, ltotal = rendered_records
    t, l = T.to_struct(ttotal, NLF_TRECORD), LG.to_struct(ltotal, NLF_LRECORD)
    for kw, text in ((dict(min_count=10 ** 9), LG.TOO_FEW), (dict(lag=0), "lag 1 .. 3"), (dict(lag=4), "lag 1 .. 3"), (dict(nplanes=2), "1 or 3 planes"),
                     (dict(bit_depth=9), "bit depths 8, 10 and 12")):
        args = dict(bit_depth=10, xdec=1, ydec=1, nplanes=3, lag=3, min_count=0)
        args.update(kw)
        with pytest.raises(G1SError) as e:
            noise_table(t, l, **args)
        assert text in str(e.value), str(e.value)
    empty = T.to_struct(T.empty_record(), NLF_TRECORD)
    with pytest.raises(G1SError) as e:
        noise_table(empty, l, 10, 1, 1, 3, 3)
    assert "no luma bin has enough smooth samples for a prior" in str(e.value)
    no_chroma = {k: np.array(v, copy=True) for k, v in ttotal.items()}
    no_chroma["n"][1] = 0
    got = noise_table(T.to_struct(no_chroma, NLF_TRECORD), l, 10, 1, 1, 3, 3)
    assert got.scaling_points_cb == [] and got.scaling_points_cr and got.scaling_points_y, "a chroma plane without a valid bin gets no points"
    mono = noise_table(t, l, 10, 0, 0, 1, 2)
    assert mono.ar_coeff_lag == 2 and len(mono.ar_coeffs_y) == 12 and mono.scaling_points_cb == [] and mono.scaling_points_cr == []


def test_the_commands_refusals_write_nothing(tmp_path, caplog):
    """Every refusal `estimate --table` makes before it looks for a device, with its text."""
    import logging

    from grav1synth_amd import cli

    src, out, tbl, lag_path = str(tmp_path / "a.y4m"), str(tmp_path / "a.txt"), str(tmp_path / "a.tbl"), str(tmp_path / "a.lags")
    open(src, "wb").write(b"YUV4MPEG2 W8 H8 F24:1 Ip A1:1 C420jpeg\n")
    cases = [(dict(table=src), cli.SAME_TABLE), (dict(table=out), cli.SAME_TABLE), (dict(table=tbl, levels=tbl), cli.SAME_TABLE),
             (dict(table=tbl, levels_temporal=tbl), cli.SAME_TABLE), (dict(table=tbl, table_lag=0), cli.TABLE_BAD_LAG), (dict(table=tbl, table_lag=4), cli.TABLE_BAD_LAG),
             (dict(table_lag=2), cli.TABLE_NEEDS_FLAG), (dict(profile_frames=3), cli.TABLE_NEEDS_FLAG), (dict(levels_min_count=5), cli.TABLE_NEEDS_FLAG),
             (dict(table=tbl, profile_frames=-1), cli.AUTO_BAD_NUMBER), (dict(lags=tbl), cli.TABLE_NEEDS_FLAG), (dict(table=tbl, lags=tbl), cli.SAME_TABLE),
             (dict(table=tbl, lags=out), cli.SAME_TABLE), (dict(table=tbl, lags=src), cli.SAME_TABLE), (dict(table=tbl, lags=lag_path, levels=lag_path), cli.SAME_TABLE)]
    for kw, text in cases:
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="grav1synth"):
            assert cli.estimate_command(src, out, True, **kw) == -1, kw
        assert text in caplog.text, (kw, caplog.text)
        assert not os.path.exists(out) and not os.path.exists(tbl) and not os.path.exists(lag_path)
    args = cli.build_parser().parse_args(["estimate", src, "-o", out, "--table", tbl, "--table-lag", "2", "--profile-frames", "9", "--levels-min-count", "77", "--lags", lag_path])
    assert (args.table, args.table_lag, args.profile_frames, args.levels_min_count, args.lags) == (tbl, 2, 9, 77, lag_path)


# ---------------------------------------------------------------------------------------------------- L10: the report
def test_the_report_byte_for_byte_with_every_dash(ar_total):
    from grav1synth_amd.estimate import NLF_LRECORD, format_noise_lags

    def same(total, pairs, bd, nplanes, lag, nmin):
        got = format_noise_lags(LG.to_struct(total, NLF_LRECORD), pairs, bd, nplanes, lag, nmin)
        want = LG.format_noise_lags(total, pairs, bd, nplanes, lag, nmin)
        assert got == want, (got.decode(), want.decode())
        return got.decode()

    for lag in (1, 2, 3):
        text = same(ar_total, 2, 10, 3, lag, 400)
        m = 2 * lag * (lag + 1)
        assert text.startswith(f"noiselags1\npairs 2 bit_depth 10 planes 3 lag {lag}\nplane 0\nn0 ") and " -\n" not in text, "nothing is refused"
        assert text.count("\nrho ") == 3 * m and text.count("\ncoef ") == 3 * m and text.count("\nluma ") == 2 and text.count("\nplane ") == 3
    assert same(ar_total, 2, 10, 1, 3, 400).count("\nplane ") == 1, "luma only"
    # every "-": the default Nmin of 4096 is above all of chroma's counts here and below luma's
    text = same(ar_total, 2, 10, 3, 3, 0)
    assert " -\n" not in text.split("plane 1\n")[0] and text.split("plane 1\n")[1].startswith(f"n0 {int(ar_total['n'][1, 0])} sigma_t - gain -\nrho 0 -3 -3 -\n")
    # Nmin one above the fewest pairs a lag of Cb's fit has: the fit goes (gain, coef, luma), sigma_t and the near lags' rho stay
    fewest = min(int(ar_total["n"][1, LG.lag_index(dx, dy)]) for dy in range(0, 4) for dx in range(-6, 7) if (dy, dx) != (3, 3) and abs(dx) <= 6 and not (dy == 3 and dx > 2))
    chroma = same(ar_total, 2, 10, 3, 3, fewest + 1).split("plane 1\n")[1].split("plane 2\n")[0]
    assert " gain -\n" in chroma and "coef 0 -\n" in chroma and "luma -\n" in chroma and "sigma_t -" not in chroma and "rho 23 -1 0 -\n" not in chroma
    # one far lag below Nmin: its rho alone, and the fit
    few = {k: np.array(v, copy=True) for k, v in ar_total.items()}
    few["n"][0, LG.lag_index(-3, -3)] = 399
    luma = same(few, 2, 10, 3, 3, 400).split("plane 1\n")[0]
    assert "rho 0 -3 -3 -\n" in luma and "rho 1 -2 -3 -\n" not in luma and " gain -\n" in luma and "coef 23 -\n" in luma
    assert "coef 3 -\n" not in same(few, 2, 10, 3, 1, 400).split("plane 1\n")[0], "lag 1 does not need that lag"
    # n0 below Nmin: everything of the plane; equal frames (C(0) = 0): sigma_t 0, no rho, a singular fit
    none = {k: np.array(v, copy=True) for k, v in ar_total.items()}
    none["n"][2, 0] = 399
    cr = same(none, 2, 10, 3, 3, 400).split("plane 2\n")[1]
    assert cr.startswith("n0 399 sigma_t - gain -\n") and "rho 0 -3 -3 -\n" in cr and "rho 23 -1 0 -\n" in cr and "luma -\n" in cr
    still = {k: np.array(v, copy=True) for k, v in ar_total.items()}
    for name in ("r", "s", "xr", "ls", "l2"):
        still[name] = np.zeros_like(still[name])
    luma = same(still, 2, 10, 3, 3, 400).split("plane 1\n")[0]
    assert " sigma_t 0.0000 gain -\n" in luma and "rho 23 -1 0 -\n" in luma and "coef 0 -\n" in luma
    same(LG.empty_record(), 0, 8, 3, 2, 0)
    same(ar_total, 2, 12, 3, 3, 400)


def test_the_reports_refusals_and_capacity(ar_total):
    from grav1synth_amd import _lib
    from grav1synth_amd.estimate import NLF_LRECORD

    L = _lib.lib()
    rec = LG.to_struct(ar_total, NLF_LRECORD)
    want = LG.format_noise_lags(ar_total, 2, 10, 3, 3, 400)
    buf = C.create_string_buffer(len(want))
    assert L.g1s_format_noise_lags(rec.ctypes.data, 2, 10, 3, 3, 400, buf, len(want)) == len(want) and buf.raw == want
    assert L.g1s_format_noise_lags(rec.ctypes.data, 2, 10, 3, 3, 400, buf, len(want) - 1) == _lib.G1S_ERR_CAPACITY, "one byte short"
    for bd, planes, lag in ((9, 3, 3), (10, 2, 3), (10, 3, 0), (10, 3, 4)):
        assert L.g1s_format_noise_lags(rec.ctypes.data, 2, bd, planes, lag, 400, buf, len(want)) == -1
    assert L.g1s_format_noise_lags(None, 2, 10, 3, 3, 400, buf, len(want)) == -1


def test_the_file_drivers_refusals_before_a_device_is_looked_for(tmp_path):
    """g1s_nlf_y4m_file_table, the new rung of the noise levels' file commands: code and text as literals, nothing written."""
    from grav1synth_amd import _lib

    L = _lib.lib()
    riff, missing, tbl = tmp_path / "riff.y4m", tmp_path / "missing.y4m", tmp_path / "out.tbl"
    riff.write_bytes(b"RIFF....")
    for source, lag, text in ((None, 3, "null path"), (str(missing).encode(), 3, "y4m: cannot open " + str(missing)),
                              (str(riff).encode(), 3, "y4m: not a YUV4MPEG2 stream: " + str(riff)), (str(riff).encode(), 0, "a table's lag is 1, 2 or 3"),
                              (str(riff).encode(), 4, "a table's lag is 1, 2 or 3")):
        err = C.create_string_buffer(512)
        rc = L.g1s_nlf_y4m_file_table(source, str(tbl).encode(), None, None, None, None, 0, lag, 0, None, err, len(err))
        assert (rc, err.value.decode()) == (-1, text) and not tbl.exists()
