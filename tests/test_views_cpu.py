"""tests/views.py without a GPU: the view a case asks for is the view it gets, and the guard sees a byte written where none
may be; the arithmetic of the alternating job of tests/test_gpu_views.py."""
import numpy as np
import pytest

from tests.views import GAP, device_view, far_view


@pytest.mark.parametrize("dtype,top", [(np.uint8, 255), (np.uint16, 1023)])
@pytest.mark.parametrize("extra,off", [(6, 2), (16, 8), (0, 12), (24, 0), (176, 128)])
@pytest.mark.parametrize("fill", ["random", "max", 7])
def test_view_has_the_pitch_the_base_and_the_margin_asked_for(dtype, top, extra, off, fill):
    plane = (np.arange(9 * 21).reshape(9, 21) * 5 % (top + 1)).astype(dtype)
    pitch = 21 * plane.itemsize + extra
    v, g = device_view(plane, pitch_bytes=pitch, base_offset_bytes=off, fill=fill, max_code=top, device="cpu")
    assert v.data_ptr() & 15 == off & 15 and v.stride(1) == 1 and v.stride(0) * v.element_size() == pitch
    assert np.array_equal(v.numpy(), plane)
    margin = g.buffer.numpy()[~g.inside]
    assert g.inside.sum() == plane.nbytes and margin.size >= 4 * pitch
    if fill == "random":
        assert len(set(margin.tolist())) > 16, "a hostile margin is not a constant"
    elif plane.itemsize == 1:
        assert (margin == (top if fill == "max" else fill)).all()
    g.assert_unchanged("fresh")
    g.assert_margin_intact("fresh")
    v[3, 4] = v[3, 4] ^ 1                    # a write inside the view: an output's business, an input's damage
    g.assert_margin_intact("inside")
    assert g.changed_bytes().size == 1
    g.buffer[int(np.flatnonzero(~g.inside)[-1])] ^= 1   # one byte of the margin
    assert g.changed_margin_bytes().size == 1
    with pytest.raises(AssertionError):
        g.assert_margin_intact("margin")


def test_view_refuses_what_no_tensor_can_be():
    p16 = np.zeros((4, 8), np.uint16)
    for pitch, off in ((14, 0), (17, 0), (16, 1), (16, 256)):
        with pytest.raises(ValueError):
            device_view(p16, pitch_bytes=pitch, base_offset_bytes=off, device="cpu")


def test_alternating_job_takes_every_slot_through_both_chains():
    from tests.test_gpu_views import alternation_covers_every_slot

    assert alternation_covers_every_slot()


@pytest.mark.parametrize("dtype,top,off", [(np.uint8, 255, 0), (np.uint16, 4095, 48)])
def test_far_view_places_every_row_by_its_pitch_and_guards_both_ends_of_the_gap(dtype, top, off):
    """The builder of the gigabyte pitches at a pitch a host can hold: 1 MiB + 16."""
    plane = (np.arange(5 * 21).reshape(5, 21) * 37 % (top + 1)).astype(dtype)
    pitch = (1 << 20) + 16
    v, g = far_view(plane, pitch_bytes=pitch, base_offset_bytes=off, max_code=top, device="cpu")
    assert v.data_ptr() % 256 == off and v.stride(0) * v.element_size() == pitch and np.array_equal(v.numpy(), plane)
    assert v[4:].data_ptr() - v.data_ptr() == 4 * pitch
    g.assert_unchanged("fresh")
    row = 21 * plane.itemsize
    lead = v.data_ptr() - g.buffer.data_ptr()
    assert g.buffer[lead + row + GAP] == 0xA5 and len(set(g.buffer[lead + row:lead + row + GAP].tolist())) > 16
    v[2, 3] ^= 1
    g.assert_margin_intact("inside")
    with pytest.raises(AssertionError):
        g.assert_unchanged("inside")
    g.buffer[lead + 3 * pitch - 1] ^= 1        # the last byte in front of row 3
    with pytest.raises(AssertionError):
        g.assert_margin_intact("margin")
    with pytest.raises(ValueError):
        far_view(plane, pitch_bytes=row + GAP, base_offset_bytes=0, device="cpu")
