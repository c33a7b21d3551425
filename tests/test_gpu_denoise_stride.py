"""The job stride of `denoise`'s filter forms on the device.  The host fills the widest job a frame and uploads the part the
form's kernels index, so a wrong stride shows from the second frame of a batch on, in a form whose job is not the widest.
A 72 x 50 4:2:0 clip (luma: two ragged tile columns, two tile rows; chroma: one tile) of three distinct frames in batches of
two, so a batch of two and a batch of one; without and with a luma curve, whose launch has a job array of its own.  Every
output plane byte for byte against the operation's numpy reference.

The rows that a test with more than one frame a batch and a reference had already are not repeated here:
  temporal, planes           tests/test_gpu_denoise_temporal.py::test_grainy_moving_clips_equal_the_reference (8, 10 bit)
  motion, planes             tests/test_gpu_denoise_motion.py::test_every_format_and_depth (8, 10 bit)
  plain and temporal, joint  tests/test_gpu_denoise_joint.py::test_chroma_sizes_around_the_tile_and_below_the_window (8, 10 bit)
  motion, joint, 10 bit      tests/test_gpu_denoise_motion.py::test_joint_chroma_and_a_grain_prior_with_motion
  plain and temporal, gain   tests/test_gpu_denoise_gain.py::test_chroma_sizes_around_the_tile (8, 10 bit)
  motion, gain, 10 bit       tests/test_gpu_denoise_gain.py::test_motion_on_a_pan_with_and_without_a_luma_curve"""
from __future__ import annotations

import pytest

from tests import sweep as SW
from tests.test_denoise_curve_cpu import segment
from tests.test_gpu_denoise_gain import random_gain
from tests.test_gpu_denoise_gain import reference as gain_reference
from tests.test_gpu_denoise_motion import reference as motion_reference
from tests.test_gpu_denoise_temporal import assert_clips_equal
from tests.test_gpu_grain import _to_dev

pytestmark = pytest.mark.gpu

W, H, SS, SUB, FRAMES, BATCH = 72, 50, "420", (1, 1), 3, 2
ROWS = [("plain planes", 8, dict()), ("plain planes", 10, dict()),
        ("motion joint", 8, dict(temporal_radius=1, motion_range=4, joint_chroma=True)),
        ("motion joint gain", 8, dict(temporal_radius=1, motion_range=4, joint_chroma=True, chroma_gain=True))]


@pytest.mark.parametrize("form,bd,kw", ROWS, ids=[f"{r[0]}, {r[1]} bit" for r in ROWS])
def test_every_frame_of_a_batch_reads_its_own_job(form, bd, kw):
    from grav1synth_amd.denoise import Denoiser, grain_curve

    D, mr, joint = kw.get("temporal_radius", 0), kw.get("motion_range", 0), kw.get("joint_chroma", False)
    frames = SW.denoise_frames(SW._dnt(W, H, bd, SS, 3, 2, D, FRAMES, BATCH, "b+1"), FRAMES)
    assert all((a != b).any() for f, g in zip(frames, frames[1:]) for a, b in zip(f, g)), "three distinct frames"
    gain = random_gain(bd) if kw.get("chroma_gain") else None
    for curve in (None, grain_curve([segment([(0, 24), (255, 180)])], bd, 4)):  # a two-point table
        dn = Denoiser(bd, batch_frames=BATCH, curve=curve, **dict(kw, chroma_gain=gain))
        try:
            got = dn.denoise_clip([_to_dev(f, bd) for f in frames], *SUB)
        finally:
            dn.close()
        if gain is not None:
            want = gain_reference(frames, bd, SUB, gain, D, mr=mr, curve=curve)
        else:
            want = motion_reference(frames, bd, SS, D, mr, joint=joint, curve=curve)
        assert_clips_equal(got, want, f"{form}, {bd} bit, curve {curve is not None}")
