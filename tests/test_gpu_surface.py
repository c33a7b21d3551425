"""The surface converter on the device against tests/surface_ref.py, bit for bit (array_equal everywhere): widths round the
16-byte lane and the 32-byte interleaved load in every layout and both directions, planes as views with a pitch, an odd base
and a hostile margin (tests/views.py: the per-row choice between the two paths, and rule 5), the nine combinations of memory
kinds, batches, mixed directions and layouts on one converter, planes gigabytes long, the size limits, every refusal through
the C call, and the chains decode -> diff and render -> encode end to end."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import surface_ref as R
from tests.surface_cases import LAYOUTS, frame_shapes, random_frame, random_surface, surface_shapes
from tests.views import contiguous, device_view, far_view

pytestmark = pytest.mark.gpu
INVALID, MISMATCH = -1, -2
WIDTHS = {1: (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65), 2: (1, 7, 8, 9, 15, 16, 17, 33)}
HEIGHTS = (1, 2, 3, 5)
TESTED = ["nv12", "p010", "p012", "p016", "nv16", "p210", "nv24", "p410", "planar444_msb10", "mono12_msb", "mono8"]


def to_np(planes):
    return [p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p) for p in planes]


def same(got, want, what):
    got = to_np(got)
    assert len(got) == len(want), what
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what} plane {c}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what} plane {c}: {len(bad)} samples differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]:#x} vs {b[tuple(bad[0])]:#x}"


def chroma_differs(frame):
    return len(frame) == 1 or not np.array_equal(frame[1], frame[2])


@pytest.fixture(scope="module")
def convs():
    from grav1synth_amd.surface import SurfaceConverter

    made = {}

    def get(bd, batch=0):
        if (bd, batch) not in made:
            made[(bd, batch)] = SurfaceConverter(bd, batch_frames=batch)
        return made[(bd, batch)]

    yield get
    for c in made.values():
        c.close()


def surface_of(name, planes):
    from grav1synth_amd.surface import Surface

    bd, _np, msb, xdec, ydec = LAYOUTS[name]
    return Surface(planes, bd, xdec, ydec, msb)


def unpack(conv, name, planes, out=None, sync=True):
    return conv.unpack(surface_of(name, planes), out=out, sync=sync)


def pack(conv, name, planes, out=None, sync=True):
    _bd, nplanes, msb, xdec, ydec = LAYOUTS[name]
    return conv.pack(planes, xdec, ydec, interleaved=nplanes == 2, msb_aligned=msb, out=out, sync=sync).planes


def want_unpack(name, s):
    bd, _np, msb, _x, _y = LAYOUTS[name]
    return R.unpack(s, bd, msb)


def want_pack(name, f):
    bd, nplanes, msb, _x, _y = LAYOUTS[name]
    return R.pack(f, bd, msb, nplanes == 2)


# ---- widths and heights, every layout, both directions ------------------------------------------------------------------------

@pytest.mark.parametrize("name", TESTED)
def test_widths_round_the_lane_and_the_interleaved_load(convs, name):
    bd = LAYOUTS[name][0]
    conv = convs(bd)
    odd_cw = odd_ch = False
    for w in WIDTHS[1 if bd == 8 else 2]:
        for h in HEIGHTS:
            s = random_surface(name, w, h, seed=1)
            want = want_unpack(name, s)
            assert chroma_differs(want), "Cb equals Cr: a swap would not show"
            same(unpack(conv, name, [contiguous(p) for p in s]), want, f"{name} unpack {w}x{h}")
            f = random_frame(name, w, h, seed=2)
            # both ends of the range in every plane that has two samples, and in the frame as a whole (a plane of one sample holds one end)
            assert chroma_differs(f) and all(int(p.max()) == (1 << bd) - 1 and int(p.min()) == 0 for p in f if p.size > 1)
            assert max(int(p.max()) for p in f) == (1 << bd) - 1 and (min(int(p.min()) for p in f) == 0 or sum(p.size for p in f) == 1)
            same(pack(conv, name, [contiguous(p) for p in f]), want_pack(name, f), f"{name} pack {w}x{h}")
            if len(f) == 3:
                odd_cw, odd_ch = odd_cw or f[1].shape[1] & 1 == 1, odd_ch or f[1].shape[0] & 1 == 1
    assert len(frame_shapes(name, 1, 1)) == 1 or (odd_cw and odd_ch)


# ---- views: a pitch, an odd base, a hostile margin; the per-row choice between the two paths ----------------------------------

def _placements(isz):
    """name -> (pitch from the row's bytes, base offset): rows that are all aligned, rows that are aligned in turn (a pitch that is no
    multiple of 16: per row the wave takes the one path or the other), a base that never is."""
    up = lambda row: (row + 15) // 16 * 16  # noqa: E731
    return {"pitch": (lambda row: up(row) + 32, 0), "pitch_per_row": (lambda row: up(row) + 8, 0), "odd_base": (lambda row: up(row) + 16, 16 - isz),
            "odd_base_and_pitch": (lambda row: row + isz, 3 * isz)}


def _views(planes, place, bd, seed, blank=False):
    """Device views of `planes` (blank: of planes of one value, as outputs) under placement `place`, or contiguous tensors for None;
    `place` may be a list, one entry a plane."""
    views, guards = [], []
    for c, p in enumerate(planes):
        pl = place[c] if isinstance(place, list) else place
        src = np.full(p.shape, 0x5A if p.dtype == np.uint8 else 0x5A5A, p.dtype) if blank else p
        if pl is None:
            views.append(contiguous(src))
            continue
        pitch_of, base = _placements(p.dtype.itemsize)[pl]
        v, g = device_view(src, pitch_bytes=pitch_of(p.shape[1] * p.dtype.itemsize), base_offset_bytes=base, max_code=(1 << (8 * p.dtype.itemsize)) - 1, seed=seed + c)
        views.append(v), guards.append(g)
    return views, guards


def run_views(conv, name, w, h, s_place, f_place, what):
    """Both directions with the surface's planes under s_place and the frame's under f_place: each is the input of one and the
    output of the other."""
    bd = LAYOUTS[name][0]
    for direction in ("unpack", "pack"):
        in_place, out_place = (s_place, f_place) if direction == "unpack" else (f_place, s_place)
        src = random_surface(name, w, h, seed=5) if direction == "unpack" else random_frame(name, w, h, seed=6)
        want = want_unpack(name, src) if direction == "unpack" else want_pack(name, src)
        vin, gin = _views(src, in_place, bd, 10)
        vout, gout = _views(want, out_place, bd, 20, blank=True)
        got = unpack(conv, name, vin, out=vout) if direction == "unpack" else pack(conv, name, vin, out=vout)
        same(got, want, f"{name} {direction} {w}x{h} {what}")
        for c, g in enumerate(gin):
            g.assert_unchanged(f"{name} {direction} {what}: input plane {c}")
        for c, g in enumerate(gout):
            g.assert_margin_intact(f"{name} {direction} {what}: output plane {c}")


@pytest.mark.parametrize("side", ["surface", "frame", "both"])
@pytest.mark.parametrize("name", ["nv12", "p010", "nv24", "p210", "planar444_msb10", "mono12_msb"])
def test_views_with_a_pitch_an_odd_base_and_a_hostile_margin(convs, name, side):
    bd = LAYOUTS[name][0]
    w, h = (65, 5) if bd == 8 else (33, 5)  # two 16-byte steps and a ragged end in the luma row and in the chroma rows
    for pl in _placements(1):
        run_views(convs(bd), name, w, h, pl if side != "frame" else None, pl if side != "surface" else None, f"{side}: {pl}")
    if side == "both":
        run_views(convs(bd), name, w, h, "pitch", "odd_base", "surface: pitch, frame: odd_base")
        run_views(convs(bd), name, w, h, "odd_base_and_pitch", "pitch_per_row", "surface: odd_base_and_pitch, frame: pitch_per_row")


@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_one_plane_aligned_and_the_other_not(convs, name):
    """The luma plane on the fast path and the CbCr plane sample by sample, and the other way round, on either side."""
    bd = LAYOUTS[name][0]
    w, h = (67, 6) if bd == 8 else (35, 6)
    for luma, chroma in (("pitch", "odd_base"), ("odd_base", "pitch")):
        run_views(convs(bd), name, w, h, [luma, chroma], None, f"surface: luma {luma}, CbCr {chroma}")
        run_views(convs(bd), name, w, h, None, [luma, chroma, chroma], f"frame: luma {luma}, chroma {chroma}")
        run_views(convs(bd), name, w, h, [luma, chroma], [chroma, luma, chroma], f"both: luma {luma}, CbCr {chroma} against the reverse and a mixed pair")


# ---- memory kinds and batches -----------------------------------------------------------------------------------------------

def _c_pair(name, splanes, fplanes, skind, fkind, keep):
    """(g1s_surface_t, g1s_frame_t) for planes of the kinds named: "host" (numpy), "pinned" (on_device = 2), "device"."""
    from grav1synth_amd.diff import Frame
    from grav1synth_amd.surface import Surface

    bd, _np, msb, xdec, ydec = LAYOUTS[name]
    s = Surface(splanes, bd, xdec, ydec, msb).to_c(keep)
    f = Frame(fplanes, xdec, ydec).to_c(keep)
    s.on_device, f.on_device = {"host": 0, "pinned": 2, "device": 1}[skind], {"host": 0, "pinned": 2, "device": 1}[fkind]
    return s, f


def _as_kind(planes, kind):
    import torch

    if kind == "host":
        return [np.ascontiguousarray(p) for p in planes]
    if kind == "pinned":
        return [torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in planes]
    return [contiguous(p) for p in planes]


KINDS = ("host", "pinned", "device")


@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_host_pinned_and_device_memory_in_all_nine_combinations(convs, name):
    """All nine (in, out) kinds in one batch, both directions: frames of different kinds inside a batch as well."""
    from grav1synth_amd import _lib

    L = _lib.lib()
    bd = LAYOUTS[name][0]
    conv = convs(bd, 16)
    w, h = 37, 7
    for direction in ("unpack", "pack"):
        keep, outs, wants = [], [], []
        for k, (ik, ok) in enumerate((a, b) for a in KINDS for b in KINDS):
            src = random_surface(name, w, h, seed=30 + k) if direction == "unpack" else random_frame(name, w, h, seed=30 + k)
            want = want_unpack(name, src) if direction == "unpack" else want_pack(name, src)
            vin, vout = _as_kind(src, ik), _as_kind([np.zeros_like(p) for p in want], ok)
            if direction == "unpack":
                s, f = _c_pair(name, vin, vout, ik, ok, keep)
                rc = L.g1s_surface_unpack(conv._h, C.byref(s), C.byref(f))
            else:
                s, f = _c_pair(name, vout, vin, ok, ik, keep)
                rc = L.g1s_surface_pack(conv._h, C.byref(f), C.byref(s))
            assert rc == 0, L.g1s_surface_last_error(conv._h).decode()
            if ik == "host":
                for p in vin:
                    p[...] = 0  # (a host input is the caller's again when the call returns)
            outs.append(vout), wants.append(want)
        conv.sync()
        for k, (got, want) in enumerate(zip(outs, wants)):
            same(got, want, f"{name} {direction} in {KINDS[k // 3]} out {KINDS[k % 3]}")


@pytest.mark.parametrize("n", [1, 4, 5])
def test_batches_of_one_a_whole_one_and_one_more(convs, n):
    conv = convs(10, 4)
    for direction in ("unpack", "pack"):
        srcs = [random_surface("p010", 41, 9, seed=40 + k) if direction == "unpack" else random_frame("p010", 41, 9, seed=40 + k) for k in range(n)]
        if direction == "unpack":
            outs = [unpack(conv, "p010", [contiguous(p) for p in s], sync=False) for s in srcs]
        else:
            outs = [pack(conv, "p010", [contiguous(p) for p in s], sync=False) for s in srcs]
        conv.sync()
        for k, (got, s) in enumerate(zip(outs, srcs)):
            same(got, want_unpack("p010", s) if direction == "unpack" else want_pack("p010", s), f"{direction} frame {k} of {n}")


def test_unpack_and_pack_alternate_and_geometry_and_layout_change_in_mid_queue(convs):
    """One converter, nothing waited for until the end: every change of direction, geometry or layout drains what was queued,
    complete and right."""
    conv = convs(10, 8)
    plan = [("unpack", "p010", 33, 5), ("unpack", "p010", 33, 5), ("pack", "p010", 33, 5), ("unpack", "p010", 33, 5), ("unpack", "p010", 48, 6),
            ("unpack", "p210", 48, 6), ("unpack", "planar444_msb10", 48, 6), ("pack", "planar444_msb10", 48, 6), ("pack", "planar420_lsb10", 48, 6),
            ("pack", "p010", 48, 6), ("unpack", "mono12_lsb", 17, 3), ("pack", "p010", 17, 3)]
    from grav1synth_amd.surface import Surface

    outs, wants = [], []
    for k, (direction, name, w, h) in enumerate(plan):
        _bd, nplanes, msb, xdec, ydec = LAYOUTS[name]  # (the layout at the converter's 10 bits)
        rng = np.random.default_rng([50, k])
        if direction == "unpack":
            s = [rng.integers(0, 65536, sh).astype(np.uint16) for sh in surface_shapes(name, w, h)]
            outs.append(conv.unpack(Surface([contiguous(p) for p in s], 10, xdec, ydec, msb), sync=False))
            wants.append(R.unpack(s, 10, msb))
        else:
            f = [rng.integers(0, 1024, sh).astype(np.uint16) for sh in frame_shapes(name, w, h)]
            outs.append(conv.pack([contiguous(p) for p in f], xdec, ydec, interleaved=nplanes == 2, msb_aligned=msb, sync=False).planes)
            wants.append(R.pack(f, 10, msb, nplanes == 2))
    conv.sync()
    for k, (got, want) in enumerate(zip(outs, wants)):
        same(got, want, f"call {k}: {plan[k]}")


# ---- planes gigabytes long ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["unpack", "pack"])
def test_far_views_hold_the_64_bit_row_offset(convs, direction):
    """P010 256 x 160, every plane on either side under a pitch of 2^24 bytes: the luma planes' last rows lie 2.5 GiB from their first."""
    import torch

    from tests.test_gpu_limits import _need

    pitch, w, h = 1 << 24, 256, 160
    _need(pitch * (h + h // 2 + h + h // 2 + h // 2))
    src = random_surface("p010", w, h, seed=60) if direction == "unpack" else random_frame("p010", w, h, seed=61)
    want = want_unpack("p010", src) if direction == "unpack" else want_pack("p010", src)
    vin, gin, vout, gout = [], [], [], []
    for c, p in enumerate(src):
        v, g = far_view(p, pitch_bytes=pitch, base_offset_bytes=0 if c == 0 else 32, seed=c)
        vin.append(v), gin.append(g)
    for c, p in enumerate(want):
        v, g = far_view(np.full(p.shape, 0x5A5A, p.dtype), pitch_bytes=pitch, base_offset_bytes=16 if c == 0 else 0, seed=10 + c)
        vout.append(v), gout.append(g)
    assert vin[0][h - 1:].data_ptr() - vin[0].data_ptr() == pitch * (h - 1) > 1 << 31
    assert vout[0][h - 1:].data_ptr() - vout[0].data_ptr() == pitch * (h - 1) > 1 << 31
    conv = convs(10)
    got = unpack(conv, "p010", vin, out=vout) if direction == "unpack" else pack(conv, "p010", vin, out=vout)
    same(got, want, f"far {direction}")
    for c, g in enumerate(gin):
        g.assert_unchanged(f"far {direction}: input plane {c}")
    for c, g in enumerate(gout):
        g.assert_margin_intact(f"far {direction}: output plane {c}")
    del vin, vout, gin, gout, got
    torch.cuda.empty_cache()


# ---- size limits ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,w,h", [("nv12", 65536, 2), ("p010", 2, 65536), ("p010", 65536, 2), ("nv12", 2, 65536)])
def test_65536_samples_a_side_are_right(convs, name, w, h):
    conv = convs(LAYOUTS[name][0])
    s = random_surface(name, w, h, seed=70)
    same(unpack(conv, name, [contiguous(p) for p in s]), want_unpack(name, s), f"{name} unpack {w}x{h}")
    f = random_frame(name, w, h, seed=71)
    same(pack(conv, name, [contiguous(p) for p in f]), want_pack(name, f), f"{name} pack {w}x{h}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def _valid(name="p010", w=34, h=6):
    """Device planes of a valid pair and a function that makes the two C structs of them."""
    s = [contiguous(p) for p in random_surface(name, w, h, seed=80)]
    f = [contiguous(np.zeros(sh, s[0].cpu().numpy().dtype)) for sh in frame_shapes(name, w, h)]
    return s, f


REFUSALS = [
    # (what, change(s, f), code, fragment of the text)
    ("bytes_per_sample of the surface", lambda s, f: setattr(s, "bytes_per_sample", 1), INVALID, "bytes_per_sample does not match the bit depth"),
    ("bytes_per_sample of the frame", lambda s, f: setattr(f, "bytes_per_sample", 1), INVALID, "bytes_per_sample does not match the bit depth"),
    ("another depth", lambda s, f: setattr(s, "bit_depth", 12), INVALID, "bit_depth is not the one given to g1s_surface_new"),
    ("two planes on the frame side", lambda s, f: setattr(f, "nplanes", 2), INVALID, "a frame has 1 or 3 planes"),
    ("no planes", lambda s, f: setattr(s, "nplanes", 0), INVALID, "a surface has 1, 2 or 3 planes"),
    ("1 against 3", lambda s, f: setattr(s, "nplanes", 1), MISMATCH, "do not correspond"),
    ("2 against 1", lambda s, f: setattr(f, "nplanes", 1), MISMATCH, "do not correspond"),
    ("another width", lambda s, f: setattr(f, "width", 32), MISMATCH, "surface and frame geometry differ"),
    ("another height", lambda s, f: setattr(s, "height", 4), MISMATCH, "surface and frame geometry differ"),
    ("another subsampling", lambda s, f: setattr(f, "ydec", 0), MISMATCH, "surface and frame geometry differ"),
    ("width 0", lambda s, f: (setattr(s, "width", 0), setattr(f, "width", 0)), INVALID, "unsupported surface geometry"),
    ("height 0", lambda s, f: (setattr(s, "height", 0), setattr(f, "height", 0)), INVALID, "unsupported surface geometry"),
    ("width 65537", lambda s, f: (setattr(s, "width", 65537), setattr(f, "width", 65537)), INVALID, "up to 65536 x 65536"),
    ("height 65537", lambda s, f: (setattr(s, "height", 65537), setattr(f, "height", 65537)), INVALID, "up to 65536 x 65536"),
    ("xdec 2", lambda s, f: (setattr(s, "xdec", 2), setattr(f, "xdec", 2)), INVALID, "unsupported surface geometry"),
    ("ydec above xdec", lambda s, f: (setattr(s, "xdec", 0), setattr(f, "xdec", 0)), INVALID, "unsupported surface geometry"),
    ("a null surface plane", lambda s, f: s.data.__setitem__(1, None), INVALID, "bad surface plane pointer or row stride"),
    ("a null frame plane", lambda s, f: f.data.__setitem__(2, None), INVALID, "bad frame plane pointer or row stride"),
    ("an interleaved stride of one plane's row", lambda s, f: s.stride_bytes.__setitem__(1, 34), INVALID, "bad surface plane pointer or row stride"),
    ("an interleaved stride a sample short", lambda s, f: s.stride_bytes.__setitem__(1, 66), INVALID, "bad surface plane pointer or row stride"),
    ("an odd stride", lambda s, f: f.stride_bytes.__setitem__(0, 69), INVALID, "bad frame plane pointer or row stride"),
    ("a stride above 32 bits", lambda s, f: s.stride_bytes.__setitem__(0, 1 << 32), INVALID, "bad surface plane pointer or row stride"),
    ("overlap", lambda s, f: f.data.__setitem__(1, s.data[1] + 68 * 3 - 2), INVALID, "surface and frame planes overlap"),
]


@pytest.mark.parametrize("direction", ["unpack", "pack"])
@pytest.mark.parametrize("case", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals_have_a_code_and_a_text_and_are_sticky(case, direction):
    from grav1synth_amd import _lib
    from grav1synth_amd.surface import SurfaceConverter

    _what, change, code, fragment = case
    L = _lib.lib()
    splanes, fplanes = _valid()
    keep = []
    s, f = _c_pair("p010", splanes, fplanes, "device", "device", keep)
    ok_s, ok_f = _c_pair("p010", splanes, fplanes, "device", "device", keep)
    change(s, f)
    conv = SurfaceConverter(10)
    try:
        call = (lambda a, b: L.g1s_surface_unpack(conv._h, C.byref(a), C.byref(b))) if direction == "unpack" else (lambda a, b: L.g1s_surface_pack(conv._h, C.byref(b), C.byref(a)))
        assert call(ok_s, ok_f) == 0 and L.g1s_surface_sync(conv._h) == 0
        assert call(s, f) == code
        assert fragment in L.g1s_surface_last_error(conv._h).decode()
        assert call(ok_s, ok_f) == code and L.g1s_surface_sync(conv._h) == code, "the refusal is sticky"
        assert fragment in L.g1s_surface_last_error(conv._h).decode()
    finally:
        conv.close()


def test_msb_aligned_bytes_and_bad_depths_are_refused():
    from grav1synth_amd import _lib
    from grav1synth_amd.surface import SurfaceConverter

    L = _lib.lib()
    for bd in (7, 17):
        with pytest.raises(_lib.G1SError) as e:
            SurfaceConverter(bd)
        assert "bit depths 8 to 16" in str(e.value)
    splanes, fplanes = _valid("nv12")
    keep = []
    s, f = _c_pair("nv12", splanes, fplanes, "device", "device", keep)
    s.msb_aligned = 1
    conv = SurfaceConverter(8)
    try:
        assert L.g1s_surface_unpack(conv._h, C.byref(s), C.byref(f)) == INVALID
        assert L.g1s_surface_last_error(conv._h).decode() == "msb_aligned needs two-byte samples"
    finally:
        conv.close()


@pytest.mark.parametrize("w,h", [(65537, 2), (2, 65537)])
def test_65537_is_refused(w, h):
    """(The planes behind the pointers are one row long: a refused frame is never read.)"""
    from grav1synth_amd import _lib
    from grav1synth_amd.surface import SurfaceConverter

    row = contiguous(np.zeros((1, 2 * 65537), np.uint8))
    keep = []
    s, f = _c_pair("mono8", [row], [contiguous(np.zeros((1, 2 * 65537), np.uint8))], "device", "device", keep)
    for x in (s, f):
        x.width, x.height = w, h
        x.stride_bytes[0] = w
    conv = SurfaceConverter(8)
    try:
        with pytest.raises(_lib.G1SError) as e:
            conv._check(_lib.lib().g1s_surface_unpack(conv._h, C.byref(s), C.byref(f)))
        assert e.value.code == INVALID and "up to 65536 x 65536" in str(e.value)
    finally:
        conv.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------

def test_p010_surfaces_through_unpack_and_diff_give_the_planar_table(convs):
    """decode -> diff with nothing leaving the device: P010 surfaces of a source / denoised pair, unpacked into device tensors, give
    the .tbl bytes of the planar originals."""
    from grav1synth_amd.diff import DiffGenerator, format_tbl
    from tests import content as CT

    w, h, bd, n = 64, 64, 10, 3
    pairs = [CT.make_frames("distinct", w, h, bd, 1, 1, frame=k) for k in range(n)]
    conv = convs(bd)

    def table(frames):
        g = DiffGenerator(Fraction(24, 1), bd, bd, batch_frames=n)
        try:
            for s, d in frames:
                g.diff_frame(s, d, 1, 1)
            return format_tbl(g.finish())
        finally:
            g.close()

    want = table([([contiguous(p) for p in s], [contiguous(p) for p in d]) for s, d in pairs])
    rng = np.random.default_rng(90)
    unpacked = []
    for s, d in pairs:
        sides = []
        for planes in (s, d):
            p010 = R.pack(planes, bd, True)
            p010 = [p | rng.integers(0, 64, p.shape).astype(np.uint16) for p in p010]  # (what a decoder leaves in the low bits is its own business)
            sides.append(unpack(conv, "p010", [contiguous(p) for p in p010], sync=False))
        unpacked.append(tuple(sides))
    conv.sync()  # (the converter's stream is its own: the frames go on only after this)
    for (s, d), (us, ud) in zip(pairs, unpacked):
        same(us, s, "source"), same(ud, d, "denoised")
    got = table(unpacked)
    assert got == want and len(want) > 40, got.decode()


def test_rendered_frames_packed_to_p010_equal_the_reference(convs):
    """render -> encode: GrainSynthesizer's device output goes into P010 surfaces without leaving the device."""
    from grav1synth_amd.grain import GrainSynthesizer
    from tests import content as CT
    from tests.test_gpu_grain import make_segment

    w, h, bd = 64, 64, 10
    conv = convs(bd)
    syn = GrainSynthesizer(bd)
    try:
        for k in range(3):
            _src, den = CT.make_frames("distinct", w, h, bd, 1, 1, frame=k)
            grainy = syn.apply([contiguous(p) for p in den], make_segment(2, 100 + k), 1, 1)  # (waited for: sync = True)
            got = pack(conv, "p010", grainy)
            want = R.pack(to_np(grainy), bd, True)
            same(got, want, f"frame {k}")
            assert not np.array_equal(to_np(grainy)[0], den[0]), "the synthesizer added no grain"
    finally:
        syn.close()
