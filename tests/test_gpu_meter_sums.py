"""The summing launches and the frame before, which `measure` and the noise levels drive through one host engine
(grav1synth_amd/csrc/meter_op.h): each of the five record kinds bit for bit against its restatement, at unit counts round
the summing kernel's group count, in runs of three frames at batch_frames = 2 whose second frame -- the last of the first batch -- is a device
frame that is overwritten at the first moment the meter's contract lets go of it.  There is no tolerance anywhere."""
from __future__ import annotations

import numpy as np
import pytest

from tests import measure_ref as R
from tests import measure_s_ref as S
from tests import measure_t_ref as T
from tests import measure_x_ref as X
from tests import nlf_ref as NR
from tests import nlf_t_ref as NT
from tests.test_gpu_grain import _to_dev
from tests.test_measure_cpu import SUBSAMPLINGS, planes_of
from tests.test_nlf_t_cpu import clip_frames

pytestmark = pytest.mark.gpu
TW, TH, SW = 64, 128, 512               # km_measure's tile; the strip of a workgroup of km_measure_s
STRIP_COLS, STRIP_ROWS, WAVES = 496, 32, 4  # k_nlf's strip of a wave, the waves of a workgroup


def ceil_div(a, b):
    return -(-a // b)


# (w, h), the luma tiles and the chroma tiles at 4:2:0: against km_tail<3>'s 4 groups and km_tail<4>'s 2; km_tail_s's one group
# adds a plane's strips, SW x TH each: 1, 3 and 2 in luma
MEASURE_SIZES = [((64, 128), 1, 1), ((130, 260), 9, 4), ((257, 129), 10, 3)]
LUMA_STRIPS = {(64, 128): 1, (130, 260): 3, (257, 129): 2}


@pytest.mark.parametrize("bd,ss", [(8, "444"), (10, "420")])
@pytest.mark.parametrize("size,luma_tiles,chroma_tiles_420", MEASURE_SIZES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else None)
def test_measure_all_four_kinds_over_a_batch_boundary(bd, ss, size, luma_tiles, chroma_tiles_420):
    import torch

    from grav1synth_amd.measure import GrainMeter

    (w, h), (subx, suby) = size, SUBSAMPLINGS[ss]
    assert ceil_div(w, TW) * ceil_div(h, TH) == luma_tiles and ceil_div(w, SW) * ceil_div(h, TH) == LUMA_STRIPS[size]
    assert ceil_div((w + 1) >> 1, TW) * ceil_div((h + 1) >> 1, TH) == chroma_tiles_420
    pairs = [planes_of(w, h, bd, ss, seed=40 + k, amp=60) for k in range(3)]
    m = GrainMeter(bd, batch_frames=2, temporal=True, cross=True, scales=True)
    m.measure(pairs[0][0], pairs[0][1], subx, suby)
    last = [_to_dev(planes, bd) for planes in pairs[1]]
    m.measure(last[0], last[1], subx, suby)  # the batch goes out
    # a temporal meter's pair is the caller's again at a hand-over, which keeps a copy of it
    ordinary = [m.finish()]
    for planes in last:
        for p in planes:
            p.fill_(7)
    torch.cuda.synchronize()
    m.measure(pairs[2][0], pairs[2][1], subx, suby)
    tgot, xgot, sgot = m.finish_temporal(), m.finish_cross(), m.finish_scales()
    ordinary.append(m.finish())
    m.close()
    got = np.concatenate(ordinary)
    assert len(got) == 3 and len(tgot) == 2 and len(xgot) == 3 and len(sgot) == 3
    bad = []
    for k, (noisy, clean) in enumerate(pairs):
        bad += R.mismatches(got[k], R.measure_frame(noisy, clean, bd, subx, suby), f"pair {k}")
        bad += X.mismatches(xgot[k], X.cross_frame(noisy, clean, bd, subx, suby), f"cross, pair {k}")
        bad += S.mismatches(sgot[k], S.scale_frame(noisy, clean, bd, subx, suby), f"scales, pair {k}")
    for k, want in enumerate(T.run_records(pairs, bd, subx, suby)):
        bad += T.mismatches(tgot[k], want, f"temporal, pair {k + 1} against pair {k}")
    assert not bad, "\n".join(bad)


# (w, h), bit depth, the workgroups of luma and of a 4:2:0 chroma plane: against k_nlf_tail's 4 groups
NLF_SIZES = [((2, 40), 8, 0, 0), ((499, 36), 10, 1, 1), ((1000, 260), 10, 7, 2)]


def nlf_workgroups(pw, ph):
    return ceil_div(ceil_div(pw - 1, STRIP_COLS) * ceil_div(ph - 2, STRIP_ROWS), WAVES) if pw >= 3 and ph >= 3 else 0


@pytest.mark.parametrize("size,bd,luma_wgs,chroma_wgs", NLF_SIZES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else None)
def test_noise_levels_and_their_temporal_records_over_a_batch_boundary(size, bd, luma_wgs, chroma_wgs):
    import torch

    from grav1synth_amd.estimate import NoiseLevelMeter

    w, h = size
    assert nlf_workgroups(w, h) == luma_wgs and nlf_workgroups((w + 1) >> 1, (h + 1) >> 1) == chroma_wgs
    frames = clip_frames(w, h, bd, "420", seed=62, n=3)
    m = NoiseLevelMeter(bd, batch_frames=2, temporal=True)
    m.frame([p.copy() for p in frames[0]], 1, 1)
    last = _to_dev(frames[1], bd)
    m.frame(last, 1, 1)  # the batch has gone out, behind it the copy of its last frame: the planes are the caller's again
    for p in last:
        p.fill_((1 << bd) - 1)
    torch.cuda.synchronize()
    m.frame([p.copy() for p in frames[2]], 1, 1)
    got, tgot = m.finish(), m.finish_temporal()
    m.close()
    assert len(got) == 3 and len(tgot) == 2
    bad = []
    for k, planes in enumerate(frames):
        bad += NR.mismatches(got[k], NR.nlf_frame(planes, bd, 1, 1), f"frame {k}")
    for k, want in enumerate(NT.run_records(frames, bd, 1, 1)):
        bad += NT.mismatches(tgot[k], want, f"frame {k + 1} against frame {k}")
    assert not bad, "\n".join(bad)
    if not luma_wgs:
        assert not any(np.asarray(got[k][name]).any() for k in range(3) for name in NR.NAMES), "no workgroup in any plane: a record of zeros"
