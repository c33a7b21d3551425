"""The refusals a file command makes before it asks for a device: for every exported file command (the last rung of a
ladder stands for the ladder) the return code and the text, as literals.  Each fails the same way with and without a GPU.
What tests/test_denoise_rungs_cpu.py pins for the two `denoise` ladders (null paths, a missing input, a missing prior
table, the option refusals) and tests/test_ingest_cpu.py for the reader is not repeated here."""
import ctypes as C
import os

import pytest

from grav1synth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "reference-example-table.tbl").encode()
INVALID, DIM_MISMATCH = -1, -2
CROSS_NEEDS_CHROMA = "--cross compares chroma with luma: the clip has no chroma planes"
CLIPS_DIFFER = "the two clips differ in geometry or bit depth"
NO_TABLE_HEADER = "missing filmgrn1 header"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("file_commands")

    def put(name, data):
        (d / name).write_bytes(data)
        return str(d / name).encode()

    class F:
        clip = put("clip.y4m", b"YUV4MPEG2 W16 H8 F24:1 Ip A1:1 C420\nFRAME\n" + bytes(16 * 8 * 3 // 2))
        wide = put("wide.y4m", b"YUV4MPEG2 W32 H8 F24:1 Ip A1:1 C420\nFRAME\n" + bytes(32 * 8 * 3 // 2))
        deep = put("deep.y4m", b"YUV4MPEG2 W16 H8 F24:1 Ip A1:1 C420p10\nFRAME\n" + bytes(16 * 8 * 3))
        mono = put("mono.y4m", b"YUV4MPEG2 W16 H8 F24:1 Ip A1:1 Cmono\nFRAME\n" + bytes(16 * 8))
        riff = put("riff.y4m", b"RIFF....")
        bad_table = put("bad.tbl", b"garbage\n")
        missing = str(d / "missing.y4m").encode()
        missing_table = str(d / "missing.tbl").encode()
        out = [str(d / ("out%d" % k)).encode() for k in range(4)]

    return F


def _refused(call, code, text, outputs=()):
    err = C.create_string_buffer(512)
    rc = call(err, len(err))
    assert (rc, err.value.decode()) == (code, text)
    for p in outputs:
        assert p is None or not os.path.exists(p), p


def _reader_refusals(f):
    """(input, text) for an input a reader does not open"""
    return ((None, "y4m: null path"), (f.missing, "y4m: cannot open " + f.missing.decode()), (f.riff, "y4m: not a YUV4MPEG2 stream: " + f.riff.decode()))


def test_diff_refuses(files):
    f, L = files, _lib.lib()
    frames, unequal = C.c_uint64(), C.c_int()
    devices = (C.c_int32 * 2)(0, 0)

    def plain(s, d, chain=None):
        return lambda err, cap: L.g1s_diff_y4m_files_filtered(s, d, f.out[0], None, chain, C.byref(frames), C.byref(unequal), err, cap)

    def sharded(s, d, chain=None, devs=devices, n=2):
        return lambda err, cap: L.g1s_diff_y4m_files_sharded(s, d, f.out[0], None, chain, devs, n, C.byref(frames), C.byref(unequal), err, cap)

    for command in (plain, sharded):
        for bad, text in _reader_refusals(f):
            _refused(command(bad, f.clip), INVALID, text, f.out[:1])
            _refused(command(f.clip, bad), INVALID, text, f.out[:1])
        # the chain is looked at before either file is opened
        _refused(command(f.missing, f.missing, b"nonsense"), INVALID, 'Invalid filter chain: Invalid filter syntax in "nonsense"')
        _refused(command(f.clip, f.clip, b"crop=1:2:3"), INVALID, 'Invalid filter chain: Unrecognized filter "crop=1"', f.out[:1])
    # and the devices before the chain
    _refused(sharded(f.missing, f.missing, b"nonsense", None, 2), INVALID, "no devices")
    _refused(sharded(f.clip, f.clip, None, devices, 0), INVALID, "no devices", f.out[:1])


def test_the_denoise_ladders_refuse_a_file_that_is_no_clip_and_a_table_that_does_not_parse(files):
    f, L = files, _lib.lib()
    frames = C.c_uint64(7)

    def denoise(src, prior=None):
        return lambda err, cap: L.g1s_denoise_y4m_file_auto_temporal(src, f.out[0], None, 0, 0, prior, 0, -1, 0, 0, 0, 0, 0, 0, 0.0, 0, err, cap)

    def diff(src, prior=None):
        return lambda err, cap: L.g1s_diff_y4m_file_denoised_auto_temporal(src, f.out[0], f.out[1], None, None, 0, 0, prior, 0, -1, 0, 0, 0, 0, 0, 0, 0.0, 0,
                                                                         C.byref(frames), err, cap)

    for command in (denoise, diff):
        _refused(command(f.riff), INVALID, "y4m: not a YUV4MPEG2 stream: " + f.riff.decode(), f.out[:2])
        # the table comes before the clip
        _refused(command(f.riff, f.bad_table), INVALID, "grain prior: " + NO_TABLE_HEADER, f.out[:2])
        _refused(command(f.clip, f.bad_table), INVALID, "grain prior: " + NO_TABLE_HEADER, f.out[:2])
    assert frames.value == 0


def test_noise_levels_refuse(files):
    f, L = files, _lib.lib()
    for bad, text in ((None, "null path"),) + _reader_refusals(f)[1:]:
        _refused(lambda err, cap: L.g1s_nlf_y4m_file_temporal(bad, f.out[0], f.out[1], None, 0, None, None, err, cap), INVALID, text, f.out[:2])
        _refused(lambda err, cap: L.g1s_nlf_y4m_file(bad, f.out[0], None, 0, None, err, cap), INVALID, text, f.out[:1])


def test_render_refuses(files):
    f, L = files, _lib.lib()

    def render(src, tbl, out):
        return lambda err, cap: L.g1s_grain_y4m_file(src, tbl, out, None, err, cap)

    for paths in ((None, TABLE, f.out[0]), (f.clip, None, f.out[0]), (f.clip, TABLE, None)):
        _refused(render(*paths), INVALID, "null path", f.out[:1])
    # the table comes before the clip
    _refused(render(f.missing, f.missing_table, f.out[0]), INVALID, "cannot open " + f.missing_table.decode(), f.out[:1])
    _refused(render(f.missing, f.bad_table, f.out[0]), INVALID, "grain table: " + NO_TABLE_HEADER, f.out[:1])
    for bad, text in _reader_refusals(f)[1:]:
        _refused(render(bad, TABLE, f.out[0]), INVALID, text, f.out[:1])


def test_measure_refuses(files):
    f, L = files, _lib.lib()
    unequal = C.c_int(5)

    def measure(a, b, out=f.out[0], cross=None):
        return lambda err, cap: L.g1s_measure_y4m_files_scales(a, b, out, f.out[1], cross, f.out[3], None, C.byref(unequal), err, cap)

    for paths in ((None, f.clip, f.out[0]), (f.clip, None, f.out[0]), (f.clip, f.clip, None)):
        _refused(measure(*paths), INVALID, "null path", f.out)
        assert unequal.value == 0
    for bad, text in _reader_refusals(f)[1:]:
        _refused(measure(bad, f.clip), INVALID, text, f.out)
        _refused(measure(f.clip, bad), INVALID, text, f.out)
    for other in (f.wide, f.deep, f.mono):
        _refused(measure(f.clip, other), DIM_MISMATCH, CLIPS_DIFFER, f.out)
        _refused(measure(other, f.clip, cross=f.out[2]), DIM_MISMATCH, CLIPS_DIFFER, f.out)
    _refused(measure(f.mono, f.mono, cross=f.out[2]), INVALID, CROSS_NEEDS_CHROMA, f.out)


def test_check_refuses(files):
    f, L = files, _lib.lib()
    unequal = C.c_int(5)

    def check(s, d, tbl=TABLE, out=f.out[0], cross=None):
        return lambda err, cap: L.g1s_check_y4m_files_scales(s, d, tbl, out, f.out[1], cross, f.out[3], None, None, C.byref(unequal), err, cap)

    for paths in ((None, f.clip, TABLE, f.out[0]), (f.clip, None, TABLE, f.out[0]), (f.clip, f.clip, None, f.out[0]), (f.clip, f.clip, TABLE, None)):
        _refused(check(*paths), INVALID, "null path", f.out)
        assert unequal.value == 0
    # the table comes before the clips
    _refused(check(f.missing, f.missing, f.missing_table), INVALID, "cannot open " + f.missing_table.decode(), f.out)
    _refused(check(f.missing, f.missing, f.bad_table), INVALID, "grain table: " + NO_TABLE_HEADER, f.out)
    for bad, text in _reader_refusals(f)[1:]:
        _refused(check(bad, f.clip), INVALID, text, f.out)
        _refused(check(f.clip, bad), INVALID, text, f.out)
    for other in (f.wide, f.deep, f.mono):
        _refused(check(f.clip, other), DIM_MISMATCH, CLIPS_DIFFER, f.out)
        _refused(check(other, f.clip, cross=f.out[2]), DIM_MISMATCH, CLIPS_DIFFER, f.out)
    _refused(check(f.mono, f.mono, cross=f.out[2]), INVALID, CROSS_NEEDS_CHROMA, f.out)
