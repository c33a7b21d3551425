"""Temporal noise levels (rules T1 - T8) without a device: the numpy restatement against a plain loop over samples, the
identities of a pair, wrong restatements that must differ on the content the device tests use, the host-only entry points
against the restatement byte for byte, the record's layout against the compiler's, every new refusal of the commands and of
both file ladders, and one statistical test of the definition itself."""
from __future__ import annotations

import ctypes as C
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import nlf_ref as R
from tests import nlf_t_ref as T
from tests.test_nlf_cpu import NO_12, SUBSAMPLINGS, smooth_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clip_frames(w, h, bd, ss, seed, n=2, amp=2, fade=1):
    """n frames of one run: smooth_planes' picture (a fifth of it wild: edges), under it fresh noise of +- amp eight-bit code
    values a frame, a fade of `fade` such values a frame (up in the left half, down in the right), and from frame 1 on a block that changes altogether (what moved)."""
    rng = np.random.default_rng([seed, w, h, bd, 77])
    base = smooth_planes(w, h, bd, ss, seed)
    top, up = (1 << bd) - 1, 1 << (bd - 8)
    frames = []
    for t in range(n):
        planes = []
        for p in base:
            ph, pw = p.shape
            q = p.astype(np.int64) + rng.integers(-amp * up, amp * up + 1, (ph, pw)) + t * fade * up * np.where(np.arange(pw) < pw // 2, 1, -1)[None, :]
            if t:
                y0, x0 = (t * 5) % max(ph - 3, 1), (t * 7) % max(pw - 3, 1)
                q[y0:y0 + max(ph // 3, 2), x0:x0 + max(pw // 3, 2)] += 40 * up
            planes.append(np.clip(q, 0, top).astype(p.dtype))
        frames.append(planes)
    return frames


def box_edge_pair(w, h, bd):
    """Luma only: frame t - 1 flat; frame t 16 eight-bit code values above it in the left half, so that the box sums differ by
    144 2^sh exactly, and in the right half one sample of every 3 x 3 box one code value less: 144 2^sh - 1."""
    up = 1 << (bd - 8)
    dt = np.uint8 if bd == 8 else np.uint16
    before = np.full((h, w), 100 * up, dt)
    cur = before + 16 * up
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    cur[(ys % 3 == 1) & (xs % 3 == 1) & (xs >= w // 2)] -= 1
    return [cur.astype(dt)], [before]


def assert_same(a, b, what):
    for name in T.NAMES:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), f"{what}: {name}"


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("ss", ["420", "422", "444", "mono"])
@pytest.mark.parametrize("size", [(1, 1), (3, 3), (5, 4), (9, 7), (13, 11), (33, 27)])
def test_reference_equals_a_plain_loop(ss, size):
    w, h = size
    subx, suby = SUBSAMPLINGS[ss]
    for bd in (8, 10, 12):
        a, b = clip_frames(w, h, bd, ss, seed=5)
        got = T.nlf_pair(b, a, bd, subx, suby)
        assert_same(got, T.nlf_pair_loop(b, a, bd, subx, suby), f"{w}x{h} {bd} bit {ss}")
        if w >= 33:
            assert got["n"][0].sum() > 0 and (ss == "mono" or got["n"][1].sum() > 0), "some samples count"
            assert got["n"][0].sum() < R.nlf_frame(b, bd, subx, suby)["n"][0].sum(), "and fewer than N1's gate alone lets through"
            assert (got["s"][0] > 0).any() and (got["s"][0] < 0).any(), "the fade shows in s, up and down"
    rec = T.nlf_pair(*clip_frames(13, 11, 8, "mono", seed=1)[::-1], 8)
    assert not rec["n"][1:].any() and not rec["q"][1:].any(), "zeros for the planes a frame lacks"


@pytest.mark.parametrize("bd,ss", [(8, "420"), (10, "422"), (12, "444")])
def test_the_identities_of_a_pair(bd, ss):
    subx, suby = SUBSAMPLINGS[ss]
    a, b = clip_frames(61, 47, bd, ss, seed=8)
    # a frame against itself: no difference, and n is N1's count (the box condition holds of itself)
    same = T.nlf_pair(a, a, bd, subx, suby)
    assert not same["s"].any() and not same["q"].any()
    assert np.array_equal(same["n"].sum(axis=1), R.nlf_frame(a, bd, subx, suby)["n"].sum(axis=1))
    # swapped: the gate and the bins are symmetric
    ab, ba = T.nlf_pair(b, a, bd, subx, suby), T.nlf_pair(a, b, bd, subx, suby)
    assert np.array_equal(ab["n"], ba["n"]) and np.array_equal(ab["q"], ba["q"]) and np.array_equal(ab["s"], -ba["s"]) and ab["s"].any()
    # a constant on frame t: s moves by n times it and t_T stays, while the box gate holds (luma: one bin, so that no sample
    # changes its bin; the constant is 2 eight-bit code values, the box sums moved by 18 of 144)
    up = 1 << (bd - 8)
    rng = np.random.default_rng(bd)
    flat = [(np.full((40, 56), 100 * up) + rng.integers(0, 2 * up + 1, (40, 56))).astype(a[0].dtype) for _ in range(2)]
    r0 = T.nlf_pair([flat[1]], [flat[0]], bd, 0, 0)
    r1 = T.nlf_pair([flat[1] + 2 * up], [flat[0]], bd, 0, 0)
    assert np.array_equal(r0["n"], r1["n"]) and np.count_nonzero(r0["n"][0]) == 1 and int(r0["n"][0].sum()) == 38 * 54
    assert np.array_equal(r1["s"][0], r0["s"][0] + 2 * up * r0["n"][0].astype(np.int64))
    assert T.levels(r0, 1) == T.levels(r1, 1) and T.levels(r1, 1) != T.levels(r1, 1, remove_mean=False)


def test_wrong_restatements_differ_on_the_device_tests_content():
    """The gate on one frame only, bins from frame t alone, no mean removal, s^2 wrapped to 64 bits, <= in the box condition:
    each gives another record (or level) on content tests/test_gpu_nlf_t.py measures, so a device that did one of them fails
    there."""
    for bd, ss in ((8, "420"), (10, "422"), (12, "444")):
        subx, suby = SUBSAMPLINGS[ss]
        a, b = clip_frames(150, 90, bd, ss, seed=30)
        right = T.nlf_pair(b, a, bd, subx, suby)
        for c in range(3):
            assert not np.array_equal(T.nlf_pair(b, a, bd, subx, suby, gate="t")["n"][c], right["n"][c]), (bd, c, "gate")
            assert not np.array_equal(T.nlf_pair(b, a, bd, subx, suby, bins="t")["n"][c], right["n"][c]), (bd, c, "bins")
        assert T.levels(right, 64) != T.levels(right, 64, remove_mean=False), "the fade would be read as grain"
        assert sum(t is not None for t in T.levels(right, 64)) > 3
        # |s| passes 2^32 only in a clip's record: this pair 2^30 times over, which T5 sums without an overflow
        clip = {name: (right[name].astype(object) * (1 << 30)).astype(T.DTYPES[name]) for name in T.NAMES}
        assert max(abs(int(v)) for v in clip["s"][0]) > 2 ** 32
        assert T.levels(clip, 64 << 30) == T.levels(right, 64) and T.levels(clip, 64 << 30) != T.levels(clip, 64 << 30, wrap_s2=True)
        cur, before = box_edge_pair(64, 20, bd)
        strict, loose = T.nlf_pair(cur, before, bd, 0, 0), T.nlf_pair(cur, before, bd, 0, 0, box_strict=False)
        assert 0 < int(strict["n"][0].sum()) < int(loose["n"][0].sum()) == 62 * 18


# ------------------------------------------------------------------------------------------------- the host-only calls
def _struct(rec):
    from grav1synth_amd.estimate import NLF_TRECORD

    return T.to_struct(rec, NLF_TRECORD)


def _clip_record(bd=10, ss="420", frames=4, w=96, h=80, amp=2):
    subx, suby = SUBSAMPLINGS[ss]
    return T.run_records(clip_frames(w, h, bd, ss, seed=40, n=frames, amp=amp), bd, subx, suby)


def _record_of(bins, plane=0):
    """A temporal record whose bins of `plane` are {k: (n, sigma, mean difference)} in code values of the depth:
    q = n (2 sigma^2 + d^2), s = n d."""
    rec = T.empty_record()
    for k, (n, sg, d) in bins.items():
        rec["n"][plane, k] = n
        rec["s"][plane, k] = n * d
        rec["q"][plane, k] = int(round(n * (2 * sg * sg + d * d)))
    return rec


def test_sum_and_its_overflow():
    from grav1synth_amd.estimate import NLF_TRECORD, noise_levels_sum_temporal

    recs = _clip_record()
    assert len(recs) == 3
    got = noise_levels_sum_temporal(np.array([_struct(r) for r in recs], NLF_TRECORD))
    assert not T.mismatches(got, T.sum_records(recs), "total")
    assert not T.mismatches(noise_levels_sum_temporal(np.zeros(0, NLF_TRECORD)), T.empty_record(), "no records")
    for name, big, fits in (("n", 2 ** 63, 2 ** 63 - 1), ("q", 2 ** 63, 2 ** 63 - 1), ("s", 2 ** 62, 2 ** 62 - 1), ("s", -2 ** 62 - 1, -2 ** 62 + 1)):
        a, b = T.empty_record(), T.empty_record()
        a[name][2, 31] = big
        b[name][2, 31] = big
        with pytest.raises(OverflowError):
            T.sum_records([a, b])
        with pytest.raises(_lib.G1SError):
            noise_levels_sum_temporal(np.array([_struct(a), _struct(b)], NLF_TRECORD))
        b[name][2, 31] = fits  # the largest sum that fits is taken
        got = noise_levels_sum_temporal(np.array([_struct(a), _struct(b)], NLF_TRECORD))
        assert int(got[name][2, 31]) == big + fits


SIGMA_CASES = {
    "one valid bin": {7: (5000, 2.5, 0)},
    "adjacent bins with a fade": {k: (4096 + k, 1.0 + 0.5 * k, k - 16) for k in range(32)},
    "gaps between valid bins": {2: (9000, 4.0, 3), 3: (100, 90.0, 0), 11: (4096, 1.0, -200), 12: (4095, 50.0, 0), 30: (70000, 2.0, 1)},
    "a bin without noise but with a flicker": {9: (5000, 0.0, 37), 20: (5000, 3.0, 0)},
    "nothing but constant differences": {9: (5000, 0.0, -4), 10: (6000, 0.0, 4000)},
    "the ends": {0: (5000, 1.0, 0), 31: (5000, 7.0, 0)},
}


@pytest.mark.parametrize("name", list(SIGMA_CASES))
@pytest.mark.parametrize("bd", [8, 10])
def test_sigma_and_prior_equal_the_restatement(name, bd):
    from grav1synth_amd.estimate import noise_chroma_sigma, noise_prior, noise_sigma

    rec = _record_of(SIGMA_CASES[name])
    got, want = noise_sigma(_struct(rec), bd, temporal=True), T.sigma(rec, bd)
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    if name == "one valid bin":
        assert (got == 255).all()
    if name == "nothing but constant differences":
        assert (got == 1).all(), "the mean is removed: no noise at all"
    if name == "gaps between valid bins":
        assert T.levels(rec)[11] == 256, "a mean of -200 on sigma 1"
    fwd, inv = noise_prior(_struct(rec), bd, temporal=True)
    wf, wi = R.curve_from_s(want, bd)
    assert np.array_equal(fwd, wf) and np.array_equal(inv, wi)
    # N9 on t_T: the two chroma planes pooled, at B = 8 whatever the depth
    pooled = _record_of(SIGMA_CASES[name], 1)
    other = _record_of({k: (n // 2, sg * 2, -d) for k, (n, sg, d) in SIGMA_CASES[name].items()}, 2)
    for f in T.NAMES:
        pooled[f][2] = other[f][2]
    gc = noise_chroma_sigma(_struct(pooled), temporal=True)
    assert gc.shape == (256,) and np.array_equal(gc, T.chroma_sigma(pooled))


def test_min_count_and_refusals_of_the_prior():
    from grav1synth_amd.estimate import noise_chroma_sigma, noise_sigma

    rec = _record_of({4: (300, 2.0, 1), 9: (299, 9.0, 0)})
    with pytest.raises(_lib.G1SError) as e:
        noise_sigma(_struct(rec), 10, temporal=True)  # the default, 4096: no valid bin
    assert "no luma bin has enough smooth samples for a prior" in str(e.value)
    with pytest.raises(ValueError):
        T.sigma(rec, 10)
    with pytest.raises(_lib.G1SError):
        noise_sigma(_struct(rec), 10, min_count=301, temporal=True)
    on = noise_sigma(_struct(rec), 10, min_count=300, temporal=True)  # on bin 4's n and one above bin 9's: one valid bin
    assert (on == 255).all() and np.array_equal(on, T.sigma(rec, 10, 300))
    both = noise_sigma(_struct(rec), 10, min_count=299, temporal=True)
    assert np.array_equal(both, T.sigma(rec, 10, 299)) and both[0] == 56 and both[-1] == 255
    with pytest.raises(_lib.G1SError) as e:
        noise_chroma_sigma(_struct(rec), temporal=True)
    assert "no chroma bin has enough smooth samples for a prior" in str(e.value)
    for bd, text in ((12, NO_12), (9, "a grain prior is defined for bit depths 8 and 10")):
        with pytest.raises(_lib.G1SError) as e:
            noise_sigma(_struct(_record_of({4: (5000, 2.0, 0)})), bd, temporal=True)
        assert text in str(e.value)
    over = T.empty_record()
    over["n"][1, 3] = over["n"][2, 3] = 2 ** 63
    with pytest.raises(_lib.G1SError) as e:
        noise_chroma_sigma(_struct(over), temporal=True)
    assert T.SUMS_LEAVE_64 in str(e.value)
    with pytest.raises(ValueError):
        T.chroma_sigma(over)


def test_strength_and_its_refusals():
    from grav1synth_amd.estimate import auto_strength

    L = _lib.lib()
    for bd in (8, 10, 12):
        for recs in (_clip_record(bd, "420"), _clip_record(bd, "mono", amp=5), _clip_record(bd, "444", amp=1)):
            total = T.sum_records(recs)
            hl, hc = auto_strength(_struct(total), bd, 256, temporal=True)
            assert hl == T.strength(total, bd, 256, 0) and hc == T.strength(total, bd, 256, 1)
            assert hl is not None and (hc is None) == (not total["n"][1:].any())
    # grain of sigma = 3 ten-bit code values under a fade of 5: h = sqrt(2) x 3 / 4 whatever the fade
    rec = _record_of({k: (1000, 3.0, 5) for k in range(8)})
    assert auto_strength(_struct(rec), 10, temporal=True)[0] == np.sqrt(43.0 - 25.0) / 4.0
    h = C.c_double(-1.0)

    def refused(text, rec_, bd, min_count, cls):
        assert L.g1s_nlf_strength_temporal(_struct(rec_).ctypes.data, bd, min_count, cls, C.byref(h)) == -1 and h.value == -1.0
        assert L.g1s_last_global_error().decode() == text

    refused("too few smooth samples for a strength", _record_of({3: (4095, 2.0, 0)}), 10, 0, 0)
    refused("too few smooth samples for a strength", _record_of({3: (500, 2.0, 0)}), 10, 501, 0)
    refused("too few smooth samples for a strength", _record_of({3: (5000, 2.0, 0)}), 10, 0, 1)
    refused("the measured strength is outside 0 < h <= 1000", _record_of({3: (5000, 0.0, 9)}), 10, 0, 0)
    refused("the measured strength is outside 0 < h <= 1000", _record_of({3: (5000, 800.0, 0)}), 8, 0, 0)
    refused("noise levels are defined for bit depths 8, 10 and 12", _record_of({3: (5000, 2.0, 0)}), 9, 0, 0)
    refused("plane_class is 0 (luma) or 1 (chroma)", _record_of({3: (5000, 2.0, 0)}), 10, 0, 2)
    assert L.g1s_nlf_strength_temporal(_struct(_record_of({3: (500, 2.0, 0)})).ctypes.data, 10, 500, 0, C.byref(h)) == 0 and h.value > 0
    with pytest.raises(_lib.G1SError) as e:
        auto_strength(_struct(T.empty_record()), 10, temporal=True)
    assert "too few smooth samples" in str(e.value)


def test_the_report_byte_for_byte():
    from grav1synth_amd.estimate import NLF_RECORD, format_noise_levels_temporal

    for bd, ss in ((10, "420"), (8, "mono"), (12, "444"), (8, "422")):
        nplanes = 1 if ss == "mono" else 3
        subx, suby = SUBSAMPLINGS[ss]
        frames = clip_frames(96, 80, bd, ss, seed=40, n=4)
        total = T.sum_records(T.run_records(frames, bd, subx, suby))
        later = R.sum_records([R.nlf_frame(f, bd, subx, suby) for f in frames[1:]])
        for min_count in (0, 256, 10 ** 9):
            text = format_noise_levels_temporal(_struct(total), 3, bd, nplanes, min_count, ordinary=R.to_struct(later, NLF_RECORD))
            assert text == T.format_noise_levels_temporal(total, 3, bd, nplanes, min_count, later), text.decode()
        assert text.startswith(b"noiselevels_t1\npairs 3 bit_depth %d planes %d\nplane 0\nbin " % (bd, nplanes))
        assert text.endswith(b"auto_strength_t - -\n") and text.count(b"plane_sigma_t ") == text.count(b"ratio ") == nplanes
        assert b"ratio -" not in text
        fine = format_noise_levels_temporal(_struct(total), 3, bd, nplanes, 256).splitlines()
        assert fine == T.format_noise_levels_temporal(total, 3, bd, nplanes, 256).splitlines()
        assert fine[-1].split()[1] != b"-" and (fine[-1].split()[2] == b"-") == (ss == "mono") and fine.count(b"ratio -") == nplanes, "no ordinary record"
    # every "-": no counting sample; an ordinary record without one; an ordinary record without noise
    empty = format_noise_levels_temporal(_struct(T.empty_record()), 0, 8, 1)
    assert empty == b"noiselevels_t1\npairs 0 bit_depth 8 planes 1\nplane 0\nplane_sigma_t -\nratio -\nauto_strength_t - -\n"
    one = _record_of({5: (5000, 2.0, 0)})
    flat = R.empty_record()
    for ordinary in (R.empty_record(), flat):
        text = format_noise_levels_temporal(_struct(one), 1, 8, 3, ordinary=R.to_struct(ordinary, NLF_RECORD))
        assert text == T.format_noise_levels_temporal(one, 1, 8, 3, 0, ordinary)
        assert text == (b"noiselevels_t1\npairs 1 bit_depth 8 planes 3\nplane 0\nbin 5 5000 2.0000\nplane_sigma_t 2.0000\nratio -\n"
                        b"plane 1\nplane_sigma_t -\nratio -\nplane 2\nplane_sigma_t -\nratio -\nauto_strength_t 2.8284 -\n")
        flat["n"][0, 5] = 100  # (counting samples, q = 0: plane_sigma is 0 and the ratio undefined)
    # a capacity one byte short
    assert format_noise_levels_temporal(_struct(T.empty_record()), 0, 8, 1, cap=len(empty)) == empty
    with pytest.raises(_lib.G1SError) as e:
        format_noise_levels_temporal(_struct(T.empty_record()), 0, 8, 1, cap=len(empty) - 1)
    assert e.value.code == _lib.G1S_ERR_CAPACITY
    for bd, nplanes in ((9, 1), (8, 2), (8, 0)):
        with pytest.raises(_lib.G1SError) as e:
            format_noise_levels_temporal(_struct(T.empty_record()), 0, bd, nplanes)
        assert e.value.code == -1


def test_the_host_only_half_builds_with_a_host_compiler_and_has_the_headers_layout(tmp_path):
    from grav1synth_amd.estimate import NLF_TRECORD

    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "nlf_t_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tests", "nlf_t_host.cpp")]
    # (the sanitizer's runtime inside the program where the compiler can do that: it then starts under any preloaded library)
    if subprocess.call(cmd + ["-static-libasan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok"
    size, off_n, off_s, off_q = (int(v) for v in lines[0].split())
    assert size == C.sizeof(_lib.G1SNlfTRecord) == NLF_TRECORD.itemsize == 8 * 3 * 96
    for f, off in zip(T.NAMES, (off_n, off_s, off_q)):
        assert off == getattr(_lib.G1SNlfTRecord, f).offset == NLF_TRECORD.fields[f][1], f
    assert NLF_TRECORD.fields["s"][0].base == np.dtype("<i8")


def test_the_file_commands_record_arithmetic_under_the_sanitizers(tmp_path):
    """tests/nlf_file_host.cpp: a total taken batch by batch, and the total less the first frame's record."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "nlf_file_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(ROOT, "tests", "nlf_file_host.cpp")]
    if subprocess.call(cmd + ["-static-libasan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.splitlines()[-1] == "ok"


# ------------------------------------------------------------------------------------------------------------ refusals
def test_no_gpu_means_the_temporal_meter_refuses():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from grav1synth_amd.estimate import NoiseLevelMeter

    L = _lib.lib()
    assert not L.g1s_nlf_new_temporal(10, None)
    assert L.g1s_last_global_error().decode() == "no HIP device available: noise levels has no CPU fallback"
    with pytest.raises(_lib.G1SError) as e:
        NoiseLevelMeter(10, temporal=True)
    assert "noise levels has no CPU fallback" in str(e.value)


def test_bad_bit_depth_and_options_are_refused_before_a_device_is_looked_for():
    L = _lib.lib()
    assert not L.g1s_nlf_new_temporal(9, None)
    assert L.g1s_last_global_error().decode() == "noise levels are defined for bit depths 8, 10 and 12"
    bad = _lib.G1SNlfOpts(4, -1, 0)
    assert not L.g1s_nlf_new_temporal(10, C.byref(bad))
    assert "struct_size" in L.g1s_last_global_error().decode()
    assert L.g1s_nlf_cut(None) == -1 and L.g1s_nlf_finish_temporal(None, None, 0, None) == -1


def _one_line(caplog, text, call):
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="grav1synth"):
        assert call() == -1
    got = [r.getMessage() for r in caplog.records]
    assert got == [text], got


def test_estimate_levels_temporal_refuses_like_the_other_outputs(tmp_path, caplog, monkeypatch):
    from grav1synth_amd import cli, estimate

    a, out, lev, tlev = (str(tmp_path / n) for n in ("a.y4m", "out.txt", "levels.txt", "tlevels.txt"))
    open(a, "wb").write(b"x")
    _one_line(caplog, cli.SAME_AS_OUTPUT, lambda: cli.estimate_command(a, out, levels_temporal=a))
    _one_line(caplog, cli.SAME_LEVELS_TEMPORAL, lambda: cli.estimate_command(a, out, levels_temporal=out))
    _one_line(caplog, cli.SAME_LEVELS_TEMPORAL, lambda: cli.estimate_command(a, out, levels=lev, levels_temporal=str(tmp_path) + "//levels.txt"))
    open(tlev, "wb").write(b"kept")
    _one_line(caplog, cli.NOT_OVERWRITING, lambda: cli.estimate_command(a, out, levels_temporal=tlev, confirm=lambda *_: False))
    assert open(tlev, "rb").read() == b"kept" and not os.path.exists(out)
    # the wiring: --levels-temporal reaches estimate_y4m_file, and without it the call is the one it was
    seen = []
    monkeypatch.setattr(estimate, "estimate_y4m_file", lambda s, o, **kw: seen.append(kw) or 2)
    assert cli.main(["estimate", a, "-o", out, "--levels-temporal", tlev, "-y"]) == 0 and seen[-1] == dict(device=-1, levels=None, levels_temporal=tlev)
    assert cli.main(["estimate", a, "-o", out, "--levels", lev, "--levels-temporal", tlev, "-y"]) == 0
    assert seen[-1] == dict(device=-1, levels=lev, levels_temporal=tlev)
    assert cli.main(["estimate", a, "-o", out, "--levels", lev, "-y"]) == 0 and seen[-1] == dict(device=-1, levels=lev)


def test_auto_temporal_refuses_with_one_logged_line(tmp_path, caplog, monkeypatch):
    from grav1synth_amd import cli, denoise, ingest

    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
    out, tbl = tmp_path / "o.y4m", tmp_path / "t.tbl"
    dn = lambda **kw: cli.denoise_command(str(src), str(out), **kw)  # noqa: E731
    df = lambda **kw: cli.diff_command(str(src), None, str(tbl), denoise=True, **kw)  # noqa: E731
    for run in (dn, df):
        _one_line(caplog, cli.AUTO_TEMPORAL_NEEDS_FLAG, lambda: run(auto_temporal=True))
        _one_line(caplog, cli.AUTO_TEMPORAL_NEEDS_FLAG, lambda: run(auto_temporal=True, strength=3.0))
        _one_line(caplog, cli.AUTO_TEMPORAL_NEEDS_TWO, lambda: run(auto_temporal=True, auto_strength=True, profile_frames=1))
        _one_line(caplog, cli.AUTO_STRENGTH_AND_STRENGTH, lambda: run(auto_temporal=True, auto_strength=True, strength=3.0))
    assert not out.exists() and not tbl.exists()
    # the wiring: the flag reaches both file calls, and a job without it makes the call it made
    a = cli.build_parser().parse_args(["diff", "s.y4m", "--denoise", "-o", "t.tbl", "--auto-strength", "--auto-temporal"])
    assert cli._denoise_parameters(a)["auto_temporal"] is True and cli._denoise_parameters(a)["auto_strength"] is True
    a = cli.build_parser().parse_args(["denoise", "in.y4m", "-o", "out.y4m", "--auto-prior"])
    assert "auto_temporal" not in cli._denoise_parameters(a)
    seen = []
    monkeypatch.setattr(denoise, "denoise_y4m_file", lambda i, o, **kw: seen.append(kw) or 2)
    monkeypatch.setattr(ingest, "diff_y4m_file_denoised", lambda s, o, **kw: seen.append(kw) or 2)
    assert cli.main(["denoise", str(src), "-o", str(out), "--auto-strength", "--auto-temporal"]) == 0 and seen[-1]["auto_temporal"] is True
    assert cli.main(["diff", str(src), "--denoise", "-o", str(tbl), "--auto-prior", "--auto-temporal"]) == 0 and seen[-1]["auto_temporal"] is True
    assert cli.main(["denoise", str(src), "-o", str(out), "--auto-strength"]) == 0 and "auto_temporal" not in seen[-1]


def test_the_new_rungs_refuse_before_they_look_for_a_device_and_zero_is_the_rung_below(tmp_path):
    from grav1synth_amd.denoise import denoise_opts

    L = _lib.lib()
    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(8))
    example = os.path.join(ROOT, "tests", "golden", "reference-example-table.tbl").encode()
    out, tbl = str(tmp_path / "o.y4m").encode(), str(tmp_path / "t.tbl").encode()
    err = C.create_string_buffer(512)
    frames = C.c_uint64(7)
    g = _lib.G1SOpts(C.sizeof(_lib.G1SOpts), -1, 3, 0, 0, 0)

    def new_rungs(opts, prior, auto, temporal):
        a = L.g1s_denoise_y4m_file_auto_temporal(str(src).encode(), out, C.byref(opts), 0, 0, prior, 0, -1, 0, auto, 0, 0, 0, 0, 0.0, temporal, err, len(err))
        ta = err.value.decode()
        b = L.g1s_diff_y4m_file_denoised_auto_temporal(str(src).encode(), tbl, None, C.byref(g), C.byref(opts), 0, 0, prior, 0, -1, 0, auto, 0, 0, 0, 0, 0.0,
                                                       temporal, C.byref(frames), err, len(err))
        return (a, ta), (b, err.value.decode())

    def rungs_below(opts, prior, auto):
        a = L.g1s_denoise_y4m_file_levels(str(src).encode(), out, C.byref(opts), 0, 0, prior, 0, -1, 0, auto, 0, 0, 0, 0, 0.0, err, len(err))
        ta = err.value.decode()
        b = L.g1s_diff_y4m_file_denoised_levels(str(src).encode(), tbl, None, C.byref(g), C.byref(opts), 0, 0, prior, 0, -1, 0, auto, 0, 0, 0, 0, 0.0,
                                                C.byref(frames), err, len(err))
        return (a, ta), (b, err.value.decode())

    def both(text, opts, prior, auto, temporal):
        for rc, got in new_rungs(opts, prior, auto, temporal):
            assert rc == -1 and got == text, (rc, got)
        assert frames.value == 0

    both("auto_temporal is 0 or 1", denoise_opts(), None, _lib.G1S_AUTO_STRENGTH, 2)
    both("auto_temporal is 0 or 1", denoise_opts(), None, 0, 0xFFFFFFFF)
    both("temporal noise levels need an auto flag (an auto prior or an auto strength)", denoise_opts(), None, 0, 1)
    both("temporal noise levels need an auto flag (an auto prior or an auto strength)", denoise_opts(), example, 0, 1)
    for auto in (4, 8):  # the bits of auto_flags stay as they are
        both("unknown auto flags", denoise_opts(), None, auto, 1)
        both("unknown auto flags", denoise_opts(), None, auto, 0)
    both("an auto prior does not combine with a grain prior table", denoise_opts(), example, _lib.G1S_AUTO_PRIOR, 1)
    both("an auto strength does not combine with a given strength", denoise_opts(strength=2.0), None, _lib.G1S_AUTO_STRENGTH, 1)
    # auto_temporal = 0: what the rung below answers, refusal or not (without a device: that there is none)
    for opts, prior, auto in ((denoise_opts(), None, 0), (denoise_opts(), None, _lib.G1S_AUTO_STRENGTH), (denoise_opts(strength=2.0), None, 3),
                              (denoise_opts(), example, _lib.G1S_AUTO_PRIOR), (denoise_opts(), example, 0)):
        for p in (out, tbl):
            if os.path.exists(p):
                os.remove(p)
        below = rungs_below(opts, prior, auto)
        made = [os.path.exists(p) and open(p, "rb").read() for p in (out, tbl)]
        for p in (out, tbl):
            if os.path.exists(p):
                os.remove(p)
        assert new_rungs(opts, prior, auto, 0) == below
        assert [os.path.exists(p) and open(p, "rb").read() for p in (out, tbl)] == made


# -------------------------------------------------------------------------------------- the definition, statistically
def _still_picture(w=200, h=200):
    """10 bit: a ramp with a weak texture, an edge box and a fine checker of +- 2 (it passes N1's gate: a strong one would be
    read as noise by the Laplacian mask whatever the grain)."""
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    pic = 200.0 + 500.0 * xs / w + 100.0 * ys / h + 12.0 * np.sin(xs / 3.0) * np.cos(ys / 4.0)
    pic[60:110, 40:90] += 250.0
    pic[150:180, 120:170] += np.where((xs[:, 120:170] + ys[150:180]) & 1, 2.0, -2.0)
    return pic


def _grain(rng, shape, sigma, box):
    g = rng.standard_normal((shape[0] + box - 1, shape[1] + box - 1))
    if box > 1:
        c = np.cumsum(np.cumsum(np.pad(g, ((1, 0), (1, 0))), axis=0), axis=1)
        g = c[box:, box:] - c[:-box, box:] - c[box:, :-box] + c[:-box, :-box]
    else:
        g = g[:shape[0], :shape[1]]
    return g * (sigma / g.std())


def _noisy(pic, grain):
    return np.clip(np.rint(pic + grain), 0, 1023).astype(np.uint16)


def test_the_definition_holds_on_correlated_grain():
    """Reference only.  A still 200 x 200 10-bit picture, two frames under Gaussian grain of sigma 16 (4 eight-bit code
    values); the truth is the sample standard deviation of the grain as it was added (both frames pooled).

    What the rules give (seed 20): white grain: plane_sigma_t 16.001 of 16.000 (N8's plane_sigma 16.021), on the pan of 2
    samples 16.234; 3 x 3 box-filtered grain: plane_sigma_t 15.827 of 16.000, while N8's plane_sigma reads 3.672 (0.23 of it),
    on the pan 16.058.  The pan adds little here: over a ramp it is a constant difference, which T6 removes, and what is left
    is the texture's.  The margin of 5 % is the one the N rules' statistical test uses; the pan is checked for direction only."""
    pic = _still_picture(204, 200)
    results = {}
    for name, box in (("white", 1), ("box3", 3)):
        rng = np.random.default_rng(20)
        g0, g1 = (_grain(rng, (200, 200), 16.0, box) for _ in range(2))
        truth = float(np.concatenate([g0.ravel(), g1.ravel()]).std())
        still = [[_noisy(pic[:, :200], g0)], [_noisy(pic[:, :200], g1)]]
        rec = T.nlf_pair(still[1], still[0], 10, 0, 0)
        st = T.plane_sigma_t(rec, 0)
        so = T.plane_sigma(R.nlf_frame(still[1], 10, 0, 0), 0)
        pan = T.nlf_pair([_noisy(pic[:, 2:202], g1)], still[0], 10, 0, 0)
        results[name] = (st, so, T.plane_sigma_t(pan, 0), truth)
        print(f"{name}: plane_sigma_t {st:.3f} plane_sigma {so:.3f} pan {results[name][2]:.3f} truth {truth:.3f}")
        assert int(rec["n"][0].sum()) > 10000
        assert abs(st - truth) < 0.05 * truth, (name, st, truth)
        assert results[name][2] > st, "motion adds to the temporal estimate"
    st, so, _pan, truth = results["box3"]
    assert so < 0.4 * truth, (so, truth)
    assert abs(results["white"][1] - results["white"][3]) < 0.05 * results["white"][3], "on white grain the two estimates meet"
