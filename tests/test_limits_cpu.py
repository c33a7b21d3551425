"""What `diff` can address, without a GPU: the predicate of csrc/frame_op.h (diff_size_ok, diff_plane_extent, diff_reach)
built with a host compiler (tests/diff_reach_host.cpp) and walked over the boundary values tests/test_gpu_limits.py uses."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY, STREAM, REFUSED, REFUSED_STRIDE = 0, 1, 2, 3
MAX_STRIDE = 0xffffffff // 36  # 119 304 647: 36 tile rows of it fit 32 bits


@pytest.fixture(scope="module")
def reach(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("reach") / "diff_reach_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "diff_reach_host.cpp")])

    def ask(w, h, bps, xdec, ydec, nplanes, strides):
        strides = list(strides) + [0] * (3 - len(strides))
        out = subprocess.run([str(exe)] + [str(v) for v in (w, h, bps, xdec, ydec, nplanes, *strides)], capture_output=True, text=True, check=True)
        v = [int(x) for x in out.stdout.split()]
        return bool(v[0]), v[1:4], v[4]

    return ask


@pytest.mark.parametrize("w,h,ok", [(131072, 64, True), (131073, 64, False), (131072 + 32, 64, False), (64, 131072, True), (64, 131073, False),
                                    (131072, 131072, True), (131073, 131073, False), (1, 1, True), (0, 64, False), (64, 0, False),
                                    (0xffffffff, 1, False)])
def test_a_frame_is_at_most_131072_samples_a_side(reach, w, h, ok):
    assert reach(w, h, 1, 1, 1, 1, [max(w, 1)])[0] == ok


def extent(stride, rows, row_bytes):
    return stride * (rows - 1) + row_bytes  # (python integers: no width to overflow)


@pytest.mark.parametrize("rows", [40, 160])
@pytest.mark.parametrize("bps,want_extent,want", [(1, (1 << 31) - 1, ANY), (1, 1 << 31, STREAM), (1, (1 << 32) - 1, STREAM), (1, 1 << 32, REFUSED),
                                                  (2, (1 << 31) - 2, ANY), (2, 1 << 31, STREAM), (2, (1 << 32) - 2, STREAM), (2, 1 << 32, REFUSED)])
def test_luma_extent_on_either_side_of_2_gib_and_4_gib(reach, bps, want_extent, want, rows):
    """stride * (rows - 1) + row bytes in 64 bits: a plane of 2^31 - 1 bytes runs either chain, 2^31 .. 2^32 - 1 the stream
    chain, 2^32 is refused (rows of 2-byte samples have even extents).  40 rows: the largest strides that pass the stride bound
    at these extents; the row is as long as it takes for the extent to come out to the byte."""
    stride = (want_extent - 256 * bps) // (rows - 1) // bps * bps
    row = want_extent - stride * (rows - 1)
    assert row % bps == 0 and 256 * bps <= row <= stride <= MAX_STRIDE
    ok, ext, r = reach(row // bps, rows, bps, 0, 0, 1, [stride])
    assert ok and ext[0] == extent(stride, rows, row) == want_extent and r == want


@pytest.mark.parametrize("pitch,want", [(1 << 24, STREAM), ((1 << 24) + 16, STREAM), (1 << 25, REFUSED), ((1 << 25) + 48, REFUSED), (1 << 23, ANY),
                                        (0xffffffff, REFUSED_STRIDE)])
def test_the_pitches_of_the_device_tests(reach, pitch, want):
    """256 x 160 8-bit luma under the pitches of tests/test_gpu_limits.py: 2^24 puts the last row 2.5 GiB from the first."""
    ok, ext, r = reach(256, 160, 1, 1, 1, 1, [pitch])
    assert ok and ext[0] == pitch * 159 + 256 and r == want


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("cpitch,want", [(((1 << 31) - 1 - 128) // 79, ANY), (-(-((1 << 31) - 128) // 79), STREAM), (-(-((1 << 32) - 128) // 79), REFUSED)])
def test_a_420_chroma_plane_is_the_one_that_crosses(reach, c, cpitch, want):
    """256 x 160 4:2:0: luma rows tight, one chroma plane (128 x 80 samples) under a pitch that takes its last row across
    2^31 or 2^32; the frame's reach is the furthest plane's, and a luma-only reader does not judge the chroma planes."""
    strides = [256, 128, 128]
    strides[c] = cpitch
    ok, ext, r = reach(256, 160, 1, 1, 1, 3, strides)
    assert ok and ext[0] == 256 * 159 + 256 < 1 << 31 and ext[c] == cpitch * 79 + 128 and ext[3 - c] == 128 * 80
    assert r == want and (ext[c] >= 1 << 31) == (want != ANY) and (ext[c] >= 1 << 32) == (want == REFUSED)
    assert reach(256, 160, 1, 1, 1, 1, strides)[2] == ANY


def test_the_product_does_not_wrap_at_the_largest_stride_and_height(reach):
    ok, ext, r = reach(131072, 131072, 2, 0, 0, 1, [0xfffffffe])
    assert ok and ext[0] == 0xfffffffe * 131071 + 262144 and r == REFUSED_STRIDE
    ok, ext, r = reach(131072, 131072, 2, 0, 0, 1, [MAX_STRIDE - 1])
    assert ok and ext[0] == (MAX_STRIDE - 1) * 131071 + 262144 and r == REFUSED


@pytest.mark.parametrize("rows,stride,want", [(2, MAX_STRIDE, ANY), (2, MAX_STRIDE + 1, REFUSED_STRIDE), (18, MAX_STRIDE, ANY), (19, MAX_STRIDE, STREAM),
                                              (32, MAX_STRIDE & ~15, STREAM), (32, 1 << 27, REFUSED_STRIDE), (2, (1 << 32) - 513, REFUSED_STRIDE),
                                              (36, MAX_STRIDE, STREAM), (37, MAX_STRIDE, REFUSED), (2, 1 << 31, REFUSED_STRIDE)])
def test_a_stride_is_at_most_a_36th_of_2_to_the_32(reach, rows, stride, want):
    """The accumulation kernels form (tile row) * stride in 32 bits for up to 36 rows of a tile, rows below a short plane
    included: a plane of few rows under a huge stride has a small extent and is refused all the same.  256 x 32 under a pitch of
    2^27 (extent 3.9 GiB) is the case of tests/test_gpu_limits.py; under 119 304 640 it is the stream chain's."""
    assert 36 * MAX_STRIDE < 1 << 32 <= 36 * (MAX_STRIDE + 1)
    ok, ext, r = reach(256, rows, 1, 0, 0, 1, [stride])
    assert ok and ext[0] == stride * (rows - 1) + 256 and r == want


def test_a_chroma_stride_is_judged_like_a_luma_stride(reach):
    assert reach(256, 32, 1, 1, 1, 3, [256, 128, MAX_STRIDE + 1])[2] == REFUSED_STRIDE
    assert reach(256, 32, 1, 1, 1, 3, [256, MAX_STRIDE, 128])[2] == ANY       # 15 x the stride: 1.7 GiB
    assert reach(256, 60, 1, 1, 1, 3, [256, MAX_STRIDE, 128])[2] == STREAM    # 29 x: 3.2 GiB
    assert reach(256, 80, 1, 1, 1, 3, [256, MAX_STRIDE, 128])[2] == REFUSED   # 39 x: past 4 GiB
