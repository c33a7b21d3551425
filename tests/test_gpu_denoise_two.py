"""Two denoisers at work in one process at the same time: their parameters differ, so their workgroups ask for different
amounts of LDS and leave different bytes in it, and their launches share the compute units.  Every frame of both is the
reference's, byte for byte.  (What a tile does with LDS it has not written itself is checked deterministically on the host,
tests/test_denoise_schedule_cpu.py; this is the arrangement on a device that the other files do not have.)"""
from __future__ import annotations

import pytest

from tests.test_gpu_denoise_joint import reference as joint_reference
from tests.test_gpu_denoise_temporal import assert_clips_equal, gradient_clip
from tests.test_gpu_denoise_temporal import reference as temporal_reference
from tests.test_gpu_grain import _to_dev, assert_planes_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("joint", [False, True], ids=["independent", "joint-chroma"])
def test_two_denoisers_with_different_lds_footprints_interleaved(joint):
    """131 x 97 4:2:0 10 bit, 5 frames a clip, D = 1, (A, S) = (3, 2) against (7, 1); batches of 2, so launches of both are
    in flight while frames are still handed over, one frame to each in turn."""
    from grav1synth_amd.denoise import Denoiser

    bd, sub, D = 10, (1, 1), 1
    params = [dict(search_radius=3, patch_radius=2), dict(search_radius=7, patch_radius=1)]
    clips = [gradient_clip(5, 131, 97, bd, *sub, seed=11 + k, amp=6) for k in range(2)]
    dev = [[_to_dev(f, bd) for f in c] for c in clips]
    dns = [Denoiser(bd, batch_frames=2, temporal_radius=D, joint_chroma=joint, **kw) for kw in params]
    try:
        outs = [[], []]
        for t in range(5):
            for k in (0, 1):
                outs[k].append(dns[k].apply(dev[k][t], *sub, sync=False))
        for dn in dns:
            dn.sync()
    finally:
        for dn in dns:
            dn.close()
    for k, kw in enumerate(params):
        A, S = kw["search_radius"], kw["patch_radius"]
        want = joint_reference(clips[k], bd, sub, D, A, S) if joint else temporal_reference(clips[k], bd, D, A, S)
        assert_clips_equal(outs[k], want, f"denoiser {k}: A {A} S {S}")
        for t, (d, planes) in enumerate(zip(dev[k], clips[k])):
            assert_planes_equal(d, planes, f"denoiser {k}: input frame {t} after the run")
