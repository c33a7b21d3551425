"""The exported ladders of `denoise` without a device: every rung of g1s_denoise_new*, g1s_denoise_y4m_file* and
g1s_diff_y4m_file_denoised* refuses a bad call with the code and the text the last rung gives for the same arguments
padded with the defaults, and where two things are wrong at once each entry point names the one it has always named.
Only refusals that come before a device is looked for, so a machine with one and a machine without read the same."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

from grav1synth_amd import _lib
from grav1synth_amd.denoise import denoise_opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "tests", "golden", "reference-example-table.tbl").encode()
JOINT, AUTO_PRIOR, AUTO_STRENGTH = _lib.G1S_DENOISE_JOINT_CHROMA, _lib.G1S_AUTO_PRIOR, _lib.G1S_AUTO_STRENGTH
STRUCT_SIZE = "g1s_denoise_opts_t.struct_size mismatch"

# what a rung takes beyond the paths and the opts: the first `k` of the last rung's arguments; the rest are these defaults
FILE_TAIL = ("D", "flags", "prior_tbl", "prior_range", "prior_segment", "motion_range", "auto_flags", "profile_frames", "min_count", "chroma_prior")
FILE_DEFAULTS = dict(D=0, flags=0, prior_tbl=None, prior_range=0, prior_segment=-1, motion_range=0, auto_flags=0, profile_frames=0, min_count=0, chroma_prior=0)
FILE_RUNGS = (("", 0), ("_temporal", 1), ("_ex", 2), ("_curve", 5), ("_motion", 6), ("_auto", 9), ("_chroma", 10))
NEW_TAIL = ("D", "flags", "fwd", "inv", "motion_range", "gain")
NEW_DEFAULTS = dict(D=0, flags=0, fwd=None, inv=None, motion_range=0, gain=None)
NEW_RUNGS = (("", 0), ("_temporal", 1), ("_ex", 2), ("_curve", 4), ("_motion", 5), ("_gain", 6))


def bad_opts(**kw):
    o = denoise_opts(**{k: v for k, v in kw.items() if k != "struct_size"})
    if "struct_size" in kw:
        o.struct_size = kw["struct_size"]
    return o


@pytest.fixture()
def clip(tmp_path):
    src = tmp_path / "a.y4m"
    src.write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 C420\nFRAME\n" + bytes(12))
    return str(src).encode()


def call_new(suffix, k, bit_depth, opts, tail):
    L = _lib.lib()
    h = getattr(L, "g1s_denoise_new" + suffix)(bit_depth, C.byref(opts), *[tail[n] for n in NEW_TAIL[:k]])
    text = L.g1s_last_global_error().decode()
    if h:
        L.g1s_denoise_free(h)
    return bool(h), text


def call_denoise_file(suffix, k, src, out, opts, tail):
    err = C.create_string_buffer(512)
    rc = getattr(_lib.lib(), "g1s_denoise_y4m_file" + suffix)(src, out, C.byref(opts), *[tail[n] for n in FILE_TAIL[:k]], err, len(err))
    return int(rc), err.value.decode()


def call_diff_file(suffix, k, src, out, dopts, tail):
    err, n = C.create_string_buffer(512), C.c_uint64(77)
    rc = getattr(_lib.lib(), "g1s_diff_y4m_file_denoised" + suffix)(src, out, None, None, C.byref(dopts), *[tail[n_] for n_ in FILE_TAIL[:k]], C.byref(n), err,
                                                                   len(err))
    return int(rc), err.value.decode(), int(n.value)


def rungs_that_take(rungs, names, changed):
    """the rungs whose own arguments hold everything the bad call changes"""
    last = max((names.index(n) + 1 for n in changed), default=0)
    return [(s, k) for s, k in rungs if k >= last]


# ------------------------------------------------------------------------------------------------------- g1s_denoise_new*
NEW_BAD = [
    ("wrong struct_size", dict(struct_size=8), {}, STRUCT_SIZE),
    ("unknown flags", {}, dict(flags=2), "unknown denoise flags"),
    ("search_radius 8", dict(search_radius=8), {}, "search_radius must be 1..7"),
    ("temporal_radius 4", {}, dict(D=4), "temporal_radius must be 0..3"),
    ("odd motion range", {}, dict(D=1, motion_range=7), "motion_range must be even and 0..64"),
    ("motion range above 64", {}, dict(D=1, motion_range=66), "motion_range must be even and 0..64"),
    ("motion range without radius", {}, dict(motion_range=8), "motion_range needs a temporal radius"),
    ("a gain without joint chroma", {}, dict(gain=True), "a chroma gain needs joint chroma"),
    ("patch_radius 5", dict(patch_radius=5), {}, "patch_radius must be 1..4"),
    # two at once: the order of the checks
    ("struct_size and flags", dict(struct_size=8), dict(flags=2), STRUCT_SIZE),
    ("search_radius and temporal_radius", dict(search_radius=8), dict(D=4), "search_radius must be 1..7"),
    ("temporal_radius and flags", {}, dict(D=4, flags=2), "temporal_radius must be 0..3"),
    ("flags and motion range", {}, dict(flags=2, motion_range=7), "unknown denoise flags"),
]


@pytest.mark.parametrize("name,okw,changed,text", NEW_BAD, ids=[b[0] for b in NEW_BAD])
def test_every_rung_of_the_constructors_says_what_the_last_rung_says(name, okw, changed, text):
    gain = np.full(256, 256, np.uint16)
    fwd, inv = np.zeros(1 << 10, np.uint16), np.zeros(4096, np.uint16)
    tail = dict(NEW_DEFAULTS, **changed)
    if tail["gain"] is True:
        tail["gain"] = gain.ctypes.data
    ran = 0
    for suffix, k in rungs_that_take(NEW_RUNGS, NEW_TAIL, changed):
        t = dict(tail)
        if suffix == "_curve":  # (the one rung that always has a curve: the same pair to both)
            t["fwd"], t["inv"] = fwd.ctypes.data, inv.ctypes.data
        got = call_new(suffix, k, 10, bad_opts(**okw), t)
        want = call_new("_gain", 6, 10, bad_opts(**okw), t)
        assert got == want == (False, text), (suffix, got, want)
        ran += 1
    assert ran


# -------------------------------------------------------------------------------------------------- g1s_denoise_y4m_file*
MISSING = b"/nonexistent-dir/prior.tbl"
FILE_BAD = [
    ("wrong struct_size", dict(struct_size=8), {}, {}),
    ("unknown flags", {}, dict(flags=2), {}),
    ("search_radius 8", dict(search_radius=8), {}, {}),
    ("temporal_radius 4", {}, dict(D=4), {}),
    ("odd motion range", {}, dict(D=1, motion_range=7), {}),
    ("motion range without radius", {}, dict(motion_range=8), {}),
    ("a missing prior file", {}, dict(prior_tbl=MISSING), {}),
    ("a prior segment out of range", {}, dict(prior_tbl=EXAMPLE, prior_segment=99), {}),
    ("a null input path", {}, {}, dict(src=None)),
    ("a null output path", {}, {}, dict(out=None)),
    ("an input that does not exist", {}, {}, dict(src=b"/nonexistent-dir/a.y4m")),
    ("unknown auto flags", {}, dict(auto_flags=8), {}),
    ("an auto prior beside a table", {}, dict(prior_tbl=EXAMPLE, auto_flags=AUTO_PRIOR), {}),
    ("an auto strength beside a strength", dict(strength=3.0), dict(auto_flags=AUTO_STRENGTH), {}),
    ("chroma_prior 2", {}, dict(flags=JOINT, prior_tbl=EXAMPLE, chroma_prior=2), {}),
]
# (what the texts are, where they hold no path of this run)
FILE_TEXT = {
    "wrong struct_size": STRUCT_SIZE, "unknown flags": "unknown denoise flags", "search_radius 8": "search_radius must be 1..7",
    "temporal_radius 4": "temporal_radius must be 0..3", "odd motion range": "motion_range must be even and 0..64",
    "motion range without radius": "motion_range needs a temporal radius", "a missing prior file": "grain prior: cannot open /nonexistent-dir/prior.tbl",
    "a null input path": "null path", "a null output path": "null path", "unknown auto flags": "unknown auto flags",
    "an auto prior beside a table": "an auto prior does not combine with a grain prior table",
    "an auto strength beside a strength": "an auto strength does not combine with a given strength", "chroma_prior 2": "chroma_prior is 0 or 1",
}


@pytest.mark.parametrize("name,okw,changed,paths", FILE_BAD, ids=[b[0] for b in FILE_BAD])
def test_every_rung_of_the_denoise_file_command_says_what_the_last_rung_says(name, okw, changed, paths, clip, tmp_path):
    src, out = paths.get("src", clip), paths.get("out", str(tmp_path / "o.y4m").encode())
    tail = dict(FILE_DEFAULTS, **changed)
    ran = 0
    for suffix, k in rungs_that_take(FILE_RUNGS, FILE_TAIL, changed):
        got = call_denoise_file(suffix, k, src, out, bad_opts(**okw), tail)
        want = call_denoise_file("_chroma", 10, src, out, bad_opts(**okw), tail)
        assert got == want and got[0] == -1, (suffix, got, want)
        assert name not in FILE_TEXT or got[1] == FILE_TEXT[name], (suffix, got)
        ran += 1
    assert ran and not (tmp_path / "o.y4m").exists()


# --------------------------------------------------------------------------------------------- g1s_diff_y4m_file_denoised*
# (the generator is made, on a device, before the denoiser's own parameters are looked at: those refusals are not here)
DIFF_BAD = [b for b in FILE_BAD if b[0] in ("unknown flags", "a missing prior file", "a prior segment out of range", "a null input path", "a null output path",
                                            "an input that does not exist", "unknown auto flags", "an auto prior beside a table",
                                            "an auto strength beside a strength", "chroma_prior 2")]
DIFF_BAD.append(("struct_size under an auto flag", dict(struct_size=8), dict(auto_flags=AUTO_PRIOR), {}))
DIFF_TEXT = dict(FILE_TEXT, **{"struct_size under an auto flag": STRUCT_SIZE})


@pytest.mark.parametrize("name,okw,changed,paths", DIFF_BAD, ids=[b[0] for b in DIFF_BAD])
def test_every_rung_of_the_diff_file_command_says_what_the_last_rung_says(name, okw, changed, paths, clip, tmp_path):
    src, out = paths.get("src", clip), paths.get("out", str(tmp_path / "o.tbl").encode())
    tail = dict(FILE_DEFAULTS, **changed)
    ran = 0
    for suffix, k in rungs_that_take(FILE_RUNGS, FILE_TAIL, changed):
        got = call_diff_file(suffix, k, src, out, bad_opts(**okw), tail)
        want = call_diff_file("_chroma", 10, src, out, bad_opts(**okw), tail)
        assert got == want and got[0] == -1 and got[2] == 0, (suffix, got, want)
        assert name not in DIFF_TEXT or got[1] == DIFF_TEXT[name], (suffix, got)
        ran += 1
    assert ran and not (tmp_path / "o.tbl").exists()


# ------------------------------------------------------------------------------- two things wrong at once, per entry point
def test_the_denoise_motion_rung_loads_the_prior_first_and_leaves_struct_size_to_the_constructor(clip, tmp_path):
    out = str(tmp_path / "o.y4m").encode()
    missing_prior = dict(FILE_DEFAULTS, prior_tbl=MISSING)
    # the prior before the paths
    assert call_denoise_file("_motion", 6, None, out, bad_opts(), missing_prior) == (-1, "grain prior: cannot open /nonexistent-dir/prior.tbl")
    # struct_size behind the prior, behind the null path and behind the input's opening; in front of the other parameters
    assert call_denoise_file("_motion", 6, clip, out, bad_opts(struct_size=8), missing_prior) == (-1, "grain prior: cannot open /nonexistent-dir/prior.tbl")
    assert call_denoise_file("_motion", 6, None, out, bad_opts(struct_size=8), FILE_DEFAULTS) == (-1, "null path")
    rc, text = call_denoise_file("_motion", 6, b"/nonexistent-dir/a.y4m", out, bad_opts(struct_size=8), FILE_DEFAULTS)
    assert rc == -1 and text != STRUCT_SIZE and "/nonexistent-dir/a.y4m" in text
    assert call_denoise_file("_motion", 6, clip, out, bad_opts(struct_size=8, search_radius=8), dict(FILE_DEFAULTS, flags=2)) == (-1, STRUCT_SIZE)


@pytest.mark.parametrize("suffix,k,extra", [("_auto", 9, {}), ("_chroma", 10, dict(flags=JOINT, chroma_prior=1))])
def test_auto_and_chroma_check_struct_size_up_front_only_under_their_flag(suffix, k, extra, clip, tmp_path):
    out, nowhere = str(tmp_path / "o.y4m").encode(), b"/nonexistent-dir/a.y4m"
    on = dict(FILE_DEFAULTS, auto_flags=AUTO_PRIOR, **extra)
    # under the flag: in front of the input, the pre-pass and the prior
    assert call_denoise_file(suffix, k, nowhere, out, bad_opts(struct_size=8), on) == (-1, STRUCT_SIZE)
    assert call_denoise_file(suffix, k, None, out, bad_opts(struct_size=8), on) == (-1, STRUCT_SIZE)
    assert call_diff_file(suffix, k, nowhere, str(tmp_path / "o.tbl").encode(), bad_opts(struct_size=8), on) == (-1, STRUCT_SIZE, 0)
    # without it the rung is the motion rung: the prior and the input first
    off = dict(FILE_DEFAULTS, prior_tbl=MISSING)
    assert call_denoise_file(suffix, k, nowhere, out, bad_opts(struct_size=8), off) == (-1, "grain prior: cannot open /nonexistent-dir/prior.tbl")
    rc, text = call_denoise_file(suffix, k, nowhere, out, bad_opts(struct_size=8), FILE_DEFAULTS)
    assert rc == -1 and text != STRUCT_SIZE and "/nonexistent-dir/a.y4m" in text


@pytest.mark.parametrize("suffix,k,extra", [("_motion", 6, {}), ("_auto", 9, dict(auto_flags=AUTO_PRIOR)), ("_chroma", 10, dict(chroma_prior=2))])
def test_the_diff_rungs_check_null_paths_and_flags_before_anything_else(suffix, k, extra, clip, tmp_path):
    out = str(tmp_path / "o.tbl").encode()
    tail = dict(FILE_DEFAULTS, prior_tbl=MISSING, **extra)
    assert call_diff_file(suffix, k, None, out, bad_opts(struct_size=8), tail) == (-1, "null path", 0)
    assert call_diff_file(suffix, k, clip, None, bad_opts(struct_size=8), tail) == (-1, "null path", 0)
    assert call_diff_file(suffix, k, clip, out, bad_opts(struct_size=8), dict(tail, flags=2)) == (-1, "unknown denoise flags", 0)
    assert call_diff_file(suffix, k, None, out, bad_opts(), dict(tail, flags=2)) == (-1, "null path", 0)
    # (the denoise ladder's motion rung has them the other way round)
    assert call_denoise_file("_motion", 6, None, out, bad_opts(), dict(FILE_DEFAULTS, prior_tbl=MISSING, flags=2))[1].startswith("grain prior: cannot open")


def test_chroma_checks_the_chroma_prior_before_struct_size(clip, tmp_path):
    out = str(tmp_path / "o").encode()
    for tail, text in ((dict(flags=JOINT, prior_tbl=EXAMPLE, chroma_prior=2), "chroma_prior is 0 or 1"),
                       (dict(flags=JOINT, chroma_prior=1), "a chroma prior needs a grain prior (a table or the clip's own levels)"),
                       (dict(prior_tbl=EXAMPLE, chroma_prior=1), "a chroma gain needs joint chroma")):
        t = dict(FILE_DEFAULTS, **tail)
        assert call_denoise_file("_chroma", 10, clip, out, bad_opts(struct_size=8), t) == (-1, text)
        assert call_diff_file("_chroma", 10, clip, out, bad_opts(struct_size=8), t) == (-1, text, 0)
    # struct_size then, in front of the pre-pass's own refusals and the prior
    t = dict(FILE_DEFAULTS, flags=JOINT, prior_tbl=MISSING, auto_flags=8, chroma_prior=1)
    assert call_denoise_file("_chroma", 10, clip, out, bad_opts(struct_size=8), t) == (-1, STRUCT_SIZE)
    assert call_diff_file("_chroma", 10, clip, out, bad_opts(struct_size=8), t) == (-1, STRUCT_SIZE, 0)
    # and the pre-pass's refusals in front of the prior's
    assert call_denoise_file("_chroma", 10, clip, out, bad_opts(), t) == (-1, "unknown auto flags")
    assert call_diff_file("_chroma", 10, clip, out, bad_opts(), t) == (-1, "unknown auto flags", 0)
