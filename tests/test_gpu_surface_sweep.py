"""A seeded, edge-weighted sweep of the surface converter in the manner of tests/sweep.py (which is not edited).  The case
list (tests/surface_cases.py) is fixed, and its SHA-256 is printed and pinned here; every case is compared in both directions
with tests/surface_ref.py, its planes on either side views at the case's base offset and pitch (tests/views.py), the margins
looked at afterwards."""
from __future__ import annotations

import numpy as np
import pytest

from tests import surface_cases as SC
from tests import surface_ref as R
from tests.views import device_view

DIGEST = "cc9d4d676d4e73cc7a157cb12863c30efb3381752dad15766cc3fe2cf228ec9a"


def test_the_case_list_is_fixed_and_covers_its_axes():
    cl = SC.cases()
    print("surface sweep: %d cases, sha256 %s" % (len(cl), SC.digest(cl)))
    assert len(cl) == SC.N == 96 and cl == SC.cases() and eval(repr(cl[17])) == cl[17]
    assert SC.digest(cl) == DIGEST, SC.digest(cl)
    assert {c["layout"] for c in cl} == set(SC.LAYOUTS) and {c["pitch"] for c in cl} == set(SC.PITCHES)
    assert {1, 2, 3, 4, 5, 47, 48, 49} == {c["h"] for c in cl} and {0, 1, 8, 14, 15} <= {c["base"] for c in cl}
    for bps, unit in ((1, 16), (1, 32), (2, 16), (2, 32)):  # rows one sample below, on and above 16 and 32 bytes
        widths = {c["w"] * bps for c in cl if (SC.LAYOUTS[c["layout"]][0] > 8) == (bps == 2)}
        assert any(w % unit == unit - bps for w in widths) and any(w % unit == 0 for w in widths) and any(w % unit == bps for w in widths), (bps, unit)


def _place(planes, c, seed, blank=False):
    views, guards = [], []
    for k, p in enumerate(planes):
        isz = p.dtype.itemsize
        src = np.full(p.shape, 0xC3 if isz == 1 else 0xC3C3, p.dtype) if blank else p
        v, g = device_view(src, pitch_bytes=SC.pitch_of(c["pitch"], p.shape[1] * isz, isz), base_offset_bytes=c["base"], seed=seed + k)
        views.append(v), guards.append(g)
    return views, guards


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(SC.CHUNKS))
def test_sweep_equals_the_reference(chunk):
    from grav1synth_amd.surface import Surface, SurfaceConverter

    convs = {}
    try:
        for c in SC.cases()[chunk::SC.CHUNKS]:
            bd, nplanes, msb, xdec, ydec = SC.LAYOUTS[c["layout"]]
            conv = convs.get(bd) or convs.setdefault(bd, SurfaceConverter(bd, batch_frames=2))
            for direction in ("unpack", "pack"):
                if direction == "unpack":
                    src = SC.random_surface(c["layout"], c["w"], c["h"], seed=c["i"])
                    want = R.unpack(src, bd, msb)
                else:
                    src = SC.random_frame(c["layout"], c["w"], c["h"], seed=c["i"])
                    want = R.pack(src, bd, msb, nplanes == 2)
                vin, gin = _place(src, c, 100)
                vout, gout = _place(want, c, 200, blank=True)
                if direction == "unpack":
                    got = conv.unpack(Surface(vin, bd, xdec, ydec, msb), out=vout)
                else:
                    got = conv.pack(vin, xdec, ydec, interleaved=nplanes == 2, msb_aligned=msb, out=vout).planes
                for k, (a, b) in enumerate(zip(got, want)):
                    assert np.array_equal(a.cpu().numpy(), b), f"{c!r} {direction} plane {k}"
                for k, g in enumerate(gin):
                    g.assert_unchanged(f"{c!r} {direction}: input plane {k}")
                for k, g in enumerate(gout):
                    g.assert_margin_intact(f"{c!r} {direction}: output plane {k}")
    finally:
        for conv in convs.values():
            conv.close()
