"""The two-clip file commands (`measure`, `check`, `diff` and the sharded `diff`) where their read loops differ from a plain
run: a clip pair of 5 and 3 frames with batch_frames = 2, so that the clip ends inside a batch with a batch boundary before
it, and the same pair with the shorter file cut in the middle of its last frame.  What a command writes for the unequal pair
is, byte for byte, what it writes for the 3-frame prefixes; what it computes there is checked against the references
elsewhere (tests/test_gpu_measure*.py, tests/test_gpu_parity.py)."""
from __future__ import annotations

from fractions import Fraction

import pytest

from grav1synth_amd import _lib
from tests import content as CT
from tests.test_gpu_grain import make_segment

pytestmark = pytest.mark.gpu

FPS = Fraction(24, 1)
REPORTS = ("plain", "temporal", "cross", "scales")
INVALID = -1


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """Per size: source (5 frames), denoised (3), the 3-frame source prefix and the denoised file cut inside frame 2."""
    from grav1synth_amd.diff import write_tbl
    from grav1synth_amd.ingest import write_y4m
    from grav1synth_amd.synth import SynthSpec, make_pair

    d = tmp_path_factory.mktemp("file_commands")

    def put(tag, src, den):
        paths = {k: str(d / f"{tag}_{k}.y4m") for k in ("src", "den", "src3", "cut")}
        write_y4m(paths["src"], src, 8, 1, 1, FPS)
        write_y4m(paths["den"], den[:3], 8, 1, 1, FPS)
        write_y4m(paths["src3"], src[:3], 8, 1, 1, FPS)
        data = open(paths["den"], "rb").read()
        frame = sum(int(p.shape[0]) * int(p.shape[1]) for p in den[0]) + len(b"FRAME\n")
        assert (len(data) - frame * 3) < 100, "the header and three frames"
        open(paths["cut"], "wb").write(data[:len(data) - frame // 2])
        return paths

    small = [CT.make_frames("distinct", 64, 64, 8, 1, 1, frame=k) for k in range(5)]
    spec = SynthSpec(320, 192, 8)
    big = [make_pair(spec, k, device="cpu") for k in range(5)]
    # two segments, the second from frame 2 on (a frame's time: its index in units of 1e-7 s)
    at2 = 2 * 10000000 * FPS.denominator // FPS.numerator
    first, second = make_segment(3, 11), make_segment(2, 12)
    first.end_time, second.start_time = at2, at2
    table = str(d / "two.tbl")
    write_tbl(table, [first, second])
    return dict(small=put("small", [p[0] for p in small], [p[1] for p in small]), big=put("big", [p[0] for p in big], [p[1] for p in big]), table=table,
                dir=d)


def _report_paths(d, tag):
    return {k: str(d / f"{tag}_{k}.txt") for k in REPORTS}


def _measure(c, den, src, tag):
    from grav1synth_amd.measure import measure_y4m_files

    out = _report_paths(c["dir"], tag)
    got = measure_y4m_files(c["small"][src], c["small"][den], out["plain"], batch_frames=2, temporal_output=out["temporal"], cross_output=out["cross"],
                            scales_output=out["scales"])
    return got, [open(out[k], "rb").read() for k in REPORTS]


def _check(c, den, src, tag):
    from grav1synth_amd.measure import check_y4m_files

    out = _report_paths(c["dir"], tag)
    got = check_y4m_files(c["small"][src], c["small"][den], c["table"], out["plain"], batch_frames=2, temporal_output=out["temporal"],
                          cross_output=out["cross"], scales_output=out["scales"])
    return got, [open(out[k], "rb").read() for k in REPORTS]


def _diff(c, den, src, tag, devices=None):
    from grav1synth_amd.ingest import diff_y4m_files

    out = str(c["dir"] / f"{tag}.tbl")
    got = diff_y4m_files(c["big"][src], c["big"][den], out, batch_frames=2, devices=devices)
    return got, [open(out, "rb").read()]


def _diff_sharded(c, den, src, tag):
    return _diff(c, den, src, tag, devices=[0, 0])


COMMANDS = dict(measure=_measure, check=_check, diff=_diff, diff_sharded=_diff_sharded)


@pytest.mark.parametrize("name", list(COMMANDS))
def test_unequal_lengths_stop_at_the_shorter_clip_with_the_prefixes_bytes(clips, name):
    run = COMMANDS[name]
    got, files = run(clips, "den", "src", name + "_unequal")
    assert got == (3, True)
    want, prefix_files = run(clips, "den", "src3", name + "_prefix")
    assert want == (3, False)
    assert all(f for f in files) and files == prefix_files
    if name == "check":
        assert b"\n" in files[0] and files[0] != _measure(clips, "den", "src3", "check_plain")[1][0], "two value columns: the table rendered"


# what a command answers when the shorter file ends inside its frame 2: the code and the text ({cut}: the file's path)
TRUNCATED = dict(
    measure=(INVALID, "frame 2: y4m: truncated frame 2"),
    check=(INVALID, "frame 2: y4m: truncated frame 2"),
    diff=(INVALID, "frame 2: denoised reader failed (y4m: truncated frame 2)"),
    diff_sharded=(INVALID, "frame 2: denoised reader failed (y4m: truncated frame 2)"),
)


@pytest.mark.parametrize("name", list(COMMANDS))
def test_a_truncated_clip_is_a_read_error_with_its_frame(clips, name):
    import ctypes as C

    L = _lib.lib()
    err = C.create_string_buffer(512)
    unequal, frames = C.c_int(0), C.c_uint64(0)
    d = clips["dir"]
    out = [str(d / f"{name}_cut_{k}").encode() for k in REPORTS]
    which = "small" if name in ("measure", "check") else "big"
    src, cut = clips[which]["src"].encode(), clips[which]["cut"].encode()
    if name == "measure":
        mo = _lib.G1SMeasureOpts(C.sizeof(_lib.G1SMeasureOpts), -1, 2)
        rc = L.g1s_measure_y4m_files_scales(src, cut, *out, C.byref(mo), C.byref(unequal), err, len(err))
    elif name == "check":
        mo = _lib.G1SMeasureOpts(C.sizeof(_lib.G1SMeasureOpts), -1, 2)
        rc = L.g1s_check_y4m_files_scales(src, cut, clips["table"].encode(), *out, C.byref(mo), None, C.byref(unequal), err, len(err))
    else:
        o = _lib.G1SOpts(C.sizeof(_lib.G1SOpts), -1, 3, 0, 2, 0)
        if name == "diff":
            rc = L.g1s_diff_y4m_files_filtered(src, cut, out[0], C.byref(o), None, C.byref(frames), C.byref(unequal), err, len(err))
        else:
            devices = (C.c_int32 * 2)(0, 0)
            rc = L.g1s_diff_y4m_files_sharded(src, cut, out[0], C.byref(o), None, devices, 2, C.byref(frames), C.byref(unequal), err, len(err))
    print(name, rc, err.value.decode())
    code, text = TRUNCATED[name]
    assert (rc, err.value.decode()) == (code, text.format(cut=cut.decode()))
    assert unequal.value == 0
