"""Decoder surfaces without a device: the numpy reference (tests/surface_ref.py) against a plain double loop and its exact
identities, g1s_surface_t's layout against the C compiler's, the refusals of the host-only predicate (csrc/frame_op.h
check_surface_pair, built with a host compiler: tests/surface_check_host.cpp) one value below, on and above each bound, and
the loud failure without a device."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from grav1synth_amd import _lib
from tests import surface_ref as R
from tests.surface_cases import LAYOUTS, random_frame, random_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, MISMATCH = -1, -2


def loop_unpack(surface, bd, msb):
    sh = 16 - bd if msb else 0
    h, w = surface[0].shape
    out = [np.zeros((h, w), surface[0].dtype)]
    for y in range(h):
        for x in range(w):
            out[0][y, x] = int(surface[0][y, x]) >> sh
    if len(surface) == 2:
        ch, cw2 = surface[1].shape
        out += [np.zeros((ch, cw2 // 2), surface[0].dtype) for _ in range(2)]
        for y in range(ch):
            for x in range(cw2 // 2):
                out[1][y, x] = int(surface[1][y, 2 * x]) >> sh
                out[2][y, x] = int(surface[1][y, 2 * x + 1]) >> sh
    elif len(surface) == 3:
        for c in (1, 2):
            out.append(np.zeros(surface[c].shape, surface[c].dtype))
            for y in range(surface[c].shape[0]):
                for x in range(surface[c].shape[1]):
                    out[c][y, x] = int(surface[c][y, x]) >> sh
    return out


def loop_pack(frame, bd, msb, interleaved):
    sh = 16 - bd if msb else 0
    top = 0xffff if frame[0].dtype == np.uint16 else 0xff
    word = lambda v: (int(v) << sh) & top  # noqa: E731
    out = [np.zeros(frame[0].shape, frame[0].dtype)]
    for y in range(frame[0].shape[0]):
        for x in range(frame[0].shape[1]):
            out[0][y, x] = word(frame[0][y, x])
    if len(frame) == 3:
        ch, cw = frame[1].shape
        if interleaved:
            out.append(np.zeros((ch, 2 * cw), frame[0].dtype))
        else:
            out += [np.zeros((ch, cw), frame[0].dtype) for _ in range(2)]
        for y in range(ch):
            for x in range(cw):
                for c in (1, 2):
                    if interleaved:
                        out[1][y, 2 * x + c - 1] = word(frame[c][y, x])
                    else:
                        out[c][y, x] = word(frame[c][y, x])
    return out


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (3, 2), (5, 5), (8, 1), (1, 4)])
def test_reference_equals_a_double_loop(name, size):
    w, h = size
    bd, nplanes, msb, _xdec, _ydec = LAYOUTS[name]
    s = random_surface(name, w, h, seed=3)
    assert same(R.unpack(s, bd, msb), loop_unpack(s, bd, msb))
    f = random_frame(name, w, h, seed=4)
    assert same(R.pack(f, bd, msb, nplanes == 2), loop_pack(f, bd, msb, nplanes == 2))


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_exact_identities(name):
    bd, nplanes, msb, _xdec, _ydec = LAYOUTS[name]
    sh = R.shift(bd, msb)
    w, h = 13, 7
    f = random_frame(name, w, h, seed=5)
    assert all(int(p.max()) == (1 << bd) - 1 and int(p.min()) == 0 for p in f)
    assert same(R.unpack(R.pack(f, bd, msb, nplanes == 2), bd, msb), f)
    s = random_surface(name, w, h, seed=6)
    clean = [p & np.asarray((0xffff << sh) & 0xffff if p.dtype == np.uint16 else 0xff, p.dtype) for p in s]
    assert same(R.pack(R.unpack(clean, bd, msb), bd, msb, nplanes == 2), clean)
    # the low sh bits are ignored: two surfaces that differ only there give one frame
    other = [p | np.asarray((1 << sh) - 1, p.dtype) for p in clean]
    assert same(R.unpack(other, bd, msb), R.unpack(clean, bd, msb))
    assert sh == 0 or not same(other, clean)
    # pack of a sample above the depth keeps the word's 16 bits (rule 4's mask)
    if sh:
        big = [np.full((1, 2), 0xffff, np.uint16)] * (3 if nplanes > 1 else 1)
        assert all(int(p.max()) == (0xffff << sh) & 0xffff for p in R.pack(big, bd, msb, nplanes == 2))


def test_surface_and_options_have_the_headers_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = ["width", "height", "bytes_per_sample", "xdec", "ydec", "nplanes", "bit_depth", "msb_aligned", "data", "stride_bytes", "on_device"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "g1s_diff.h"', "int main(void) {",
           '  printf("%zu %zu %zu %d\\n", sizeof(g1s_surface_t), sizeof(g1s_surface_opts_t), sizeof(g1s_frame_t), G1S_ABI_VERSION);']
    src += [f'  printf("%zu\\n", offsetof(g1s_surface_t, {f}));' for f in fields]
    src += ['  printf("%zu\\n", offsetof(g1s_surface_opts_t, batch_frames));', "  return 0;", "}"]
    (tmp_path / "s.c").write_text("\n".join(src))
    subprocess.check_call([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    out = subprocess.check_output([str(tmp_path / "s")], text=True).split()
    assert int(out[0]) == C.sizeof(_lib.G1SSurface) and int(out[1]) == C.sizeof(_lib.G1SSurfaceOpts)
    assert int(out[2]) == C.sizeof(_lib.G1SFrame) and int(out[3]) == 1, "g1s_frame_t and the ABI version stay as they were"
    for f, off in zip(fields, out[4:4 + len(fields)]):
        assert int(off) == getattr(_lib.G1SSurface, f).offset, f
    assert int(out[4 + len(fields)]) == _lib.G1SSurfaceOpts.batch_frames.offset


# ---- the host-only predicate ---------------------------------------------------------------------------------------------------

FAR = 1 << 40  # the planes' bases lie this far apart: no extent below reaches the next


def base(bd=10, w=64, h=48, xdec=1, ydec=1, snp=2, msb=None):
    """A valid pair as NAME=VALUE fields: rows without padding, five planes at FAR-apart bases."""
    bps = 1 if bd == 8 else 2
    ch, cw = R.chroma_shape(h, w, xdec, ydec)
    fnp = 1 if snp == 1 else 3
    d = {"s.width": w, "s.height": h, "s.bps": bps, "s.xdec": xdec, "s.ydec": ydec, "s.nplanes": snp, "s.depth": bd,
         "s.msb": int(bd > 8 and snp == 2 if msb is None else msb),
         "f.width": w, "f.height": h, "f.bps": bps, "f.xdec": xdec, "f.ydec": ydec, "f.nplanes": fnp}
    srow = [w * bps] + {1: [], 2: [2 * cw * bps], 3: [cw * bps] * 2}[snp]
    for c, r in enumerate(srow):
        d[f"s.data{c}"], d[f"s.stride{c}"] = (1 + c) * FAR, r
    for c, r in enumerate([w * bps] + [cw * bps] * (fnp - 1)):
        d[f"f.data{c}"], d[f"f.stride{c}"] = (4 + c) * FAR, r
    return d


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("surface") / "surface_check_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "surface_check_host.cpp")])

    def ask(fields, bd=10, unpack=True, **change):
        d = dict(fields)
        d.update({k.replace("_", ".", 1): v for k, v in change.items()})
        out = subprocess.run([str(exe), str(bd), str(int(unpack))] + [f"{k}={v}" for k, v in d.items()], capture_output=True, text=True, check=True)
        code, _, text = out.stdout.rstrip("\n").partition(" ")
        return int(code), text

    return ask


@pytest.mark.parametrize("unpack", [True, False])
def test_valid_pairs_pass(check, unpack):
    for bd, snp, xdec, ydec in ((10, 2, 1, 1), (8, 2, 1, 1), (16, 2, 1, 0), (10, 3, 0, 0), (12, 1, 0, 0), (8, 1, 1, 1), (9, 3, 1, 1)):
        assert check(base(bd, 64, 48, xdec, ydec, snp), bd, unpack) == (0, ""), (bd, snp)
    assert check(base(10, 63, 47), 10, unpack) == (0, "")
    b = base()
    b.pop("s.data2", None)
    assert check(b, 10, unpack, s_stride2=1)[0] == 0, "data[2] and its stride are ignored for two planes"


@pytest.mark.parametrize("unpack", [True, False])
def test_sample_size_depth_and_alignment(check, unpack):
    b = base()
    for change in (dict(s_bps=1), dict(f_bps=1), dict(s_bps=1, f_bps=1)):
        code, text = check(b, 10, unpack, **change)
        assert code == INVALID and "bytes_per_sample does not match the bit depth" in text
    assert check(base(8), 8, unpack, s_bps=2, f_bps=2)[0] == INVALID
    code, text = check(b, 10, unpack, s_depth=12)
    assert code == INVALID and "bit_depth is not the one given to g1s_surface_new" in text
    code, text = check(base(8), 8, unpack, s_msb=1)
    assert code == INVALID and text == "msb_aligned needs two-byte samples"
    assert check(b, 10, unpack, s_msb=0)[0] == 0


@pytest.mark.parametrize("unpack", [True, False])
def test_plane_counts(check, unpack):
    b = base()
    code, text = check(b, 10, unpack, f_nplanes=2)
    assert code == INVALID and "a frame has 1 or 3 planes" in text
    for n in (0, 4):
        assert check(b, 10, unpack, s_nplanes=n) == (INVALID, "a surface has 1, 2 or 3 planes")
    for snp, fnp in ((1, 3), (2, 1), (3, 1)):
        code, text = check(base(snp=3), 10, unpack, s_nplanes=snp, f_nplanes=fnp)
        assert code == MISMATCH and "do not correspond" in text, (snp, fnp)


@pytest.mark.parametrize("unpack", [True, False])
def test_geometry(check, unpack):
    b = base()
    for change in (dict(f_width=65), dict(f_height=47), dict(s_width=66), dict(f_xdec=0, f_ydec=0), dict(s_ydec=0)):
        code, text = check(b, 10, unpack, **change)
        assert code == MISMATCH and text == "surface and frame geometry differ", change
    for change in (dict(s_width=0, f_width=0), dict(s_height=0, f_height=0), dict(s_xdec=2, f_xdec=2), dict(s_xdec=0, f_xdec=0)):  # (the last: ydec 1 > xdec 0)
        code, text = check(b, 10, unpack, **change)
        assert code == INVALID and "unsupported surface geometry" in text, change
    for w, h, want in ((65535, 2, 0), (65536, 2, 0), (65537, 2, INVALID), (2, 65535, 0), (2, 65536, 0), (2, 65537, INVALID)):
        assert check(base(10, w, h), 10, unpack)[0] == want, (w, h)
        assert check(base(8, w, h, 0, 0, 1), 8, unpack)[0] == want, (w, h)


@pytest.mark.parametrize("unpack", [True, False])
def test_pointers_and_strides(check, unpack):
    b = base()  # P010 64 x 48: the interleaved row is 2 x 32 x 2 = 128 bytes
    for k in ("s_data0", "s_data1", "f_data0", "f_data1", "f_data2"):
        code, text = check(b, 10, unpack, **{k: 0})
        assert code == INVALID and text == f"bad {'surface' if k[0] == 's' else 'frame'} plane pointer or row stride", k
    for stride, want in ((126, INVALID), (127, INVALID), (128, 0), (129, INVALID), (130, 0), (0xfffffffe, 0), (0xffffffff, INVALID), (1 << 32, INVALID)):
        assert check(b, 10, unpack, s_stride1=stride)[0] == want, stride
    for stride, want in ((62, INVALID), (64, 0), (65, INVALID), (66, 0)):
        assert check(b, 10, unpack, f_stride2=stride)[0] == want, stride
    n = base(8)  # NV12 64 x 48: 64 bytes, and an odd stride is fine
    for stride, want in ((63, INVALID), (64, 0), (65, 0), (0xffffffff, 0), (1 << 32, INVALID)):
        assert check(n, 8, unpack, s_stride1=stride)[0] == want, stride
    o = base(10, 63, 47)  # cw = 32 all the same: (63 + 1) >> 1
    assert check(o, 10, unpack, s_stride1=126)[0] == INVALID and check(o, 10, unpack, s_stride1=128)[0] == 0
    assert check(o, 10, unpack, s_stride0=124)[0] == INVALID and check(o, 10, unpack, s_stride0=126)[0] == 0


@pytest.mark.parametrize("unpack", [True, False])
def test_overlap_by_one_byte(check, unpack):
    b = base()
    s0, s1 = b["s.data0"], b["s.data1"]
    luma, pairs, chroma = 128 * 48, 128 * 24, 64 * 24  # extents: rows without padding
    text = "surface and frame planes overlap: a converter needs distinct buffers"
    assert check(b, 10, unpack, f_data0=s0 + luma) == (0, "") and check(b, 10, unpack, f_data0=s0 + luma - 1) == (INVALID, text)
    assert check(b, 10, unpack, f_data0=s0 - luma) == (0, "") and check(b, 10, unpack, f_data0=s0 - luma + 1) == (INVALID, text)
    assert check(b, 10, unpack, f_data2=s1 + pairs) == (0, "") and check(b, 10, unpack, f_data2=s1 + pairs - 1) == (INVALID, text)
    assert check(b, 10, unpack, f_data1=s0 - chroma) == (0, "") and check(b, 10, unpack, f_data1=s0 - chroma + 1) == (INVALID, text)
    assert check(b, 10, unpack, f_data0=s0) == (INVALID, text)
    # under a pitch the extent runs to the end of the last row, not of the last pitch
    assert check(b, 10, unpack, s_stride0=256, f_data0=s0 + 256 * 47 + 128) == (0, "")
    assert check(b, 10, unpack, s_stride0=256, f_data0=s0 + 256 * 47 + 127) == (INVALID, text)


# ---- the library without a device ----------------------------------------------------------------------------------------------

def test_bad_bit_depth_and_options_are_refused_before_a_device_is_looked_for():
    L = _lib.lib()
    for bd in (0, 7, 17, 32):
        assert not L.g1s_surface_new(bd, None)
        assert L.g1s_last_global_error().decode() == "a surface converter takes bit depths 8 to 16"
    bad = _lib.G1SSurfaceOpts(4, -1, 0)
    assert not L.g1s_surface_new(10, C.byref(bad))
    assert "struct_size" in L.g1s_last_global_error().decode()


def test_no_gpu_means_the_converter_refuses():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from grav1synth_amd.surface import SurfaceConverter

    L = _lib.lib()
    assert not L.g1s_surface_new(10, None)
    assert L.g1s_last_global_error().decode() == "no HIP device available: the surface converter has no CPU fallback"
    with pytest.raises(_lib.G1SError) as e:
        SurfaceConverter(10)
    assert "has no CPU fallback" in str(e.value)
